"""Duplicated-object groups of the rearrange envs: the greedy matching of interchangeable objects to goals inside ra_post_step_kernel (ra_group_match,
robogym_amd/csrc/ra_env_kernel.h), group sampling on the host recipe and in ra_recipe_kernel, and the blocks_duplicate entry point -- against
tests/golden/rearrange_groups.npz, which tools/gen_golden_rearrange_groups.py records from the reference's own source of `ObjectStateGoal.relative_goal /
goal_distance`, `_calculate_num_success` and `sample_group_counts`.  The same checks run on the CPU against the kernel SOURCE (fiber-emulation harness) and, under
`-m gpu`, on the MI355X."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import blocks, blocks_duplicate
from robogym_amd.envs.rearrange.blocks import OBS_KEYS, BatchedBlockRearrangeEnv, greedy_group_match, group_ids, sample_group_counts

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FAST = dict(n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
# the goal layer's tolerances without groups (tests/test_rearrange_env.py _env_kernel_goal_layer): rel pos, rel rot as Euler angles away from the gimbal lock, rel rot
# as a quaternion, the two summed distances together
TOL_REL_POS, TOL_REL_ROT, TOL_REL_QUAT, TOL_DIST = 2e-6, 2e-5, 2e-6, 5e-5


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "rearrange_groups.npz"))


def _env(lib, device, B, N, **kw):
    args = dict(FAST) if lib is not None else {}
    args.update(kw)
    if lib is not None:
        args["lib"] = lib
    if N == 8:      # the shipped 8-object world
        from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv
        return BatchedYcbRearrangeEnv(B, device=device, num_objects=8, **args)
    return BatchedBlockRearrangeEnv(B, device=device, num_objects=N, **args)


def _launch(env, groups):
    """One ra_env_post_step (a scored step: frozen NULL) from zeroed trackers, with `groups` [B, N] as the env's group rows or None for a NULL pointer."""
    for f in (env.t, env.steps, env.ssl, env.successes, env.consecutive, env.prev_nsucc):
        f.zero_()
    env.prev_valid.fill_(1)                                  # reward[1] = the success count itself
    if groups is None:
        env.post.obj_group = None
    else:
        env.obj_group.copy_(torch.as_tensor(np.ascontiguousarray(groups), dtype=torch.int32, device=env.device))
        env.post.obj_group = env.obj_group.data_ptr()
    env._post()
    env.sync()
    keep = dict(packed=env.packed, reward=env.reward, goal_dist=env.goal_dist, done=env.done, goal_reset=env.goal_reset, trial_success=env.trial_success,
                sub_goal_ok=env.sub_goal_ok, prev_nsucc=env.prev_nsucc, successes=env.successes, consecutive=env.consecutive, ssl=env.ssl, steps=env.steps, t=env.t)
    return {k: v.clone() for k, v in keep.items()}


def _matching_against_golden(g, lib, device):
    from oracle import rearrange_oracle as RO

    seen = 0
    for N in (2, 5, 8):
        cases = np.nonzero(g["n"] == N)[0]
        B = len(cases)
        seen += B
        env = _env(lib, device, B, N, object_groups="single")
        cur_pos, goal_pos, cur_rot, goal_rot = (g[k][cases, :N] for k in ("cur_pos", "goal_pos", "cur_rot", "goal_rot"))
        quat, gq = RO.euler2quat(cur_rot), RO.euler2quat(goal_rot)
        for i, qa in enumerate(env.obj_q):
            env.sim.qpos[:, qa:qa + 7] = torch.tensor(np.concatenate([cur_pos[:, i], quat[:, i]], -1).astype(np.float32), device=env.device)
        env.goal[:] = torch.tensor(np.concatenate([goal_pos, gq], -1).astype(np.float32), device=env.device)
        env.goal_rot[:] = torch.tensor(goal_rot.astype(np.float32), device=env.device)
        env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
        groups = g["groups"][cases, :N]
        out = _launch(env, groups)
        assert int(env.sim.status.max()) == 0
        obs = env.observe(out["packed"])
        rp, rr = obs["rel_goal_obj_pos"].cpu().numpy().astype(np.float64), obs["rel_goal_obj_rot"].cpu().numpy().astype(np.float64)
        op = obs["obj_pos"].cpu().numpy().astype(np.float64)
        assert np.array_equal(op.astype(np.float32), cur_pos.astype(np.float32))       # (a free body's frame origin IS its qpos: the tie cases rely on it)
        # the goal entries stay indexed by goal
        assert np.abs(obs["goal_obj_pos"].cpu().numpy() - goal_pos).max() < 1e-6 and np.abs(obs["goal_obj_rot"].cpu().numpy() - goal_rot).max() < 1e-6
        # the match: the one goal of the object's group that the relative position points at
        match = np.zeros((B, N), dtype=np.int64)
        for b in range(B):
            for i in range(N):
                err = np.abs(goal_pos[b] - cur_pos[b, i] - rp[b, i]).max(-1)
                err[groups[b] != groups[b, i]] = np.inf
                assert (err < TOL_REL_POS).sum() == 1, (N, b, i, err)
                match[b, i] = int(np.argmin(err))
            assert np.array_equal(greedy_group_match(cur_pos[b], goal_pos[b], groups[b]), g["match"][cases[b], :N])      # (the host restatement)
        assert np.array_equal(match, g["match"][cases, :N]), (N, np.nonzero((match != g["match"][cases, :N]).any(1))[0])
        ref_rr = g["rel_rot"][cases, :N]
        e_rr = np.abs(RO.normalize_angles(rr - ref_rr))
        q_k, q_g = RO.euler2quat(rr), RO.euler2quat(ref_rr)
        e_q = np.minimum(np.abs(q_k - q_g).max(-1), np.abs(q_k + q_g).max(-1))
        lock = np.abs(np.abs(ref_rr[..., 1]) - np.pi / 2) < 0.05
        e_d = np.abs(out["goal_dist"][:, 0].cpu().numpy() - g["dist_pos"][cases, :N].sum(-1)) + np.abs(out["goal_dist"][:, 1].cpu().numpy() - g["dist_rot"][cases, :N].sum(-1))
        print("N = %d, %d cases: rel pos %.1e, rel rot (Euler, away from gimbal lock) %.1e, rel rot as a quaternion %.1e, summed distances %.1e" % (
            N, B, np.abs(rp - g["rel_pos"][cases, :N]).max(), e_rr[~lock].max(), e_q.max(), e_d.max()))
        assert np.abs(rp - g["rel_pos"][cases, :N]).max() < TOL_REL_POS and e_rr[~lock].max() < TOL_REL_ROT and e_q.max() < TOL_REL_QUAT and e_d.max() < TOL_DIST
        # the success count (reward[1] from a zero count, and the stored count), is_goal_achieved
        nsucc = g["num_success"][cases]
        assert np.array_equal(out["reward"][:, 1].cpu().numpy(), nsucc.astype(np.float32)) and np.array_equal(out["prev_nsucc"].cpu().numpy(), nsucc.astype(np.float32))
        assert np.array_equal(obs["is_goal_achieved"][:, 0].cpu().numpy(), (nsucc == N).astype(np.float32))
        assert np.array_equal(out["sub_goal_ok"].cpu().numpy().astype(bool), nsucc == N)
        # an explicit all-singleton table = no table, bit for bit
        a, b_ = _launch(env, np.tile(np.arange(N), (B, 1))), _launch(env, None)
        for k in a:
            assert torch.equal(a[k].view(torch.uint8) if a[k].dtype == torch.bool else a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                               b_[k].view(torch.uint8) if b_[k].dtype == torch.bool else b_[k].view(torch.int32) if b_[k].dtype == torch.float32 else b_[k]), k
    assert seen == len(g["n"]) >= 90


def _swapped_pair(g, lib, device):
    """Two blocks, each exactly on the other's goal: achieved when the two are duplicates of one another, not achieved when they are distinct."""
    from oracle import rearrange_oracle as RO

    t_grouped, t_distinct = np.nonzero(g["kind"] == "swapped")[0]
    assert list(g["groups"][t_grouped, :2]) == [0, 0] and list(g["groups"][t_distinct, :2]) == [0, 1]
    assert int(g["num_success"][t_grouped]) == 2 and int(g["num_success"][t_distinct]) == 0
    env = blocks_duplicate.make_simple_env(batch_size=1, device=device, **(dict(lib=lib, **FAST) if lib is not None else {}))
    assert env.N == 2 and env.obj_group is not None and env.obj_group.tolist() == [[0, 0]]
    quat, gq = RO.euler2quat(g["cur_rot"][t_grouped, :2]), RO.euler2quat(g["goal_rot"][t_grouped, :2])
    for i, qa in enumerate(env.obj_q):
        env.sim.qpos[0, qa:qa + 7] = torch.tensor(np.concatenate([g["cur_pos"][t_grouped, i], quat[i]]).astype(np.float32), device=env.device)
    env.goal[0] = torch.tensor(np.concatenate([g["goal_pos"][t_grouped, :2], gq], -1).astype(np.float32), device=env.device)
    env.goal_rot[0] = torch.tensor(g["goal_rot"][t_grouped, :2].astype(np.float32), device=env.device)
    env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
    out = _launch(env, g["groups"][[t_grouped], :2])
    assert float(env.observe(out["packed"])["is_goal_achieved"][0, 0]) == 1.0 and float(out["reward"][0, 1]) == 2.0 and bool(out["sub_goal_ok"][0])
    assert float(out["goal_dist"][0, 0]) == 0.0
    out = _launch(env, None)
    assert float(env.observe(out["packed"])["is_goal_achieved"][0, 0]) == 0.0 and float(out["reward"][0, 1]) == 0.0 and not bool(out["sub_goal_ok"][0])


# ------------------------------------------------------------------------------------------------ matching
def test_golden_holds_the_cases_the_matching_is_pinned_by(golden):
    g = golden
    kinds = list(g["kind"])
    assert kinds.count("swapped") == 2 and kinds.count("tie") == 4 and sorted(set(g["n"].tolist())) == [2, 5, 8]
    layouts = {tuple(np.bincount(g["groups"][t, :g["n"][t]]).tolist()) for t in range(len(kinds))}
    assert {(2,), (1, 1), (5,), (2, 1, 2), (1, 4), (1,) * 5, (8,), (3, 3, 2), (1,) * 8} <= layouts
    # the lowest-flat-index rule decides three of the ties: taking the LAST of the equal minima would give another matching
    t0, t1, t2, _ = np.nonzero(g["kind"] == "tie")[0]
    assert list(g["match"][t0, :2]) == [0, 1] and int(g["match"][t1, 1]) == 0 and int(g["match"][t2, 3]) == 3


def test_swapped_pair_is_achieved_only_with_groups_emul(golden, emul_lib):
    _swapped_pair(golden, emul_lib, "cpu")


def test_matching_against_the_reference_code_emul(golden, emul_lib):
    _matching_against_golden(golden, emul_lib, "cpu")


@pytest.mark.gpu
def test_swapped_pair_is_achieved_only_with_groups_gpu(golden):
    _swapped_pair(golden, None, "cuda:0")


@pytest.mark.gpu
def test_matching_against_the_reference_code_gpu(golden):
    _matching_against_golden(golden, None, "cuda:0")


# ------------------------------------------------------------------------------------------------ group sampling
def test_host_group_sampling_replays_the_reference_draw_for_draw(golden):
    for seed in range(256):
        rs = np.random.RandomState(seed)
        counts = sample_group_counts(rs, 5, 1.0, 8.0)
        want = golden["sample_counts"][seed]
        assert counts == want[want > 0].tolist() and rs.uniform() == golden["sample_next_draw"][seed], seed
    assert group_ids([2, 1, 2]).tolist() == [0, 0, 1, 2, 2]


def _exact_group_probabilities(N, lo, hi):
    """P(first count = 1) and P(all distinct) of sample_group_counts, from its formula: a round with `rem` objects left picks 1 with probability
    E_lam[exp(-lam) / sum_{k = 1..rem} exp(-k lam)], lam ~ U(lo, hi) drawn anew every round (Simpson's rule, fp64)."""
    lam = np.linspace(lo, hi, 20001)
    w = np.ones_like(lam); w[1:-1:2] = 4.0; w[2:-1:2] = 2.0
    w *= (lam[1] - lam[0]) / 3.0 / (hi - lo)
    p1 = [float((w * np.exp(-lam) / sum(np.exp(-k * lam) for k in range(1, rem + 1))).sum()) for rem in range(1, N + 1)]      # p1[rem - 1]
    return p1[N - 1], float(np.prod(p1))


def _device_group_sampling(lib, device, B):
    N = 5
    env = _env(lib, device, B, N, object_groups="sample", pipelined_reset=True, device_reset=True, starting_seed=7)
    assert env.obj_group.tolist() == [list(range(N))] * B and env.recipe.group_mode == 1
    env.stage.zero_(); env.done.fill_(True); env.goal_reset.fill_(False)
    r = env.recipe
    r.step = 1
    _native.check(env._L, env._L.ra_env_recipe_step(env.sim._bh, env.solver_sim._bh, ctypes.byref(r), env._stream()), "ra_env_recipe_step")
    env.sync()
    rows = env.obj_group.cpu().numpy()
    assert bool(env.ended.all()) and int(env.placement_failed.max()) == 0
    d = np.diff(rows, axis=1)
    assert (rows[:, 0] == 0).all() and ((d == 0) | (d == 1)).all()              # contiguous groups, ids 0, 1, ... in order: every row's counts sum to N
    first_is_one = rows[:, 1] == 1
    distinct = rows[:, -1] == N - 1
    p_first, p_distinct = _exact_group_probabilities(N, *env.sample_lam)
    for name, hits, p in (("first count = 1", first_is_one, p_first), ("all distinct", distinct, p_distinct)):
        sd = np.sqrt(p * (1 - p) / B)
        print("%s: %.4f of %d rows, exact %.4f (binomial sd %.4f)" % (name, hits.mean(), B, p, sd))
        assert abs(hits.mean() - p) < 5 * sd, (name, hits.mean(), p, sd)
    assert len({tuple(r_) for r_ in rows}) > 8                                   # (of the 16 compositions of 5)


def test_exact_group_probabilities_against_the_host_sampler():
    """the integration itself, against 4000 host samples"""
    rs = np.random.RandomState(3)
    draws = [sample_group_counts(rs, 5, 1.0, 8.0) for _ in range(4000)]
    p_first, p_distinct = _exact_group_probabilities(5, 1.0, 8.0)
    for hits, p in ((np.mean([c[0] == 1 for c in draws]), p_first), (np.mean([len(c) == 5 for c in draws]), p_distinct)):
        assert abs(hits - p) < 5 * np.sqrt(p * (1 - p) / 4000)


def test_device_group_sampling_emul(emul_lib):
    _device_group_sampling(emul_lib, "cpu", 512)


@pytest.mark.gpu
def test_device_group_sampling_gpu():
    _device_group_sampling(None, "cuda:0", 4096)


def test_host_recipe_samples_groups_at_reset_emul(emul_lib):
    env = _env(emul_lib, "cpu", 6, 5, object_groups="sample", sample_lam=(0.1, 1.0), starting_seed=4)      # (slow decay: many duplicates)
    env.reset()
    rows = env.obj_group.numpy().copy()
    d = np.diff(rows, axis=1)
    assert (rows[:, 0] == 0).all() and ((d == 0) | (d == 1)).all() and len({tuple(r) for r in rows}) > 1
    mask = torch.tensor([True, False, True, False, False, False])
    env.reset(mask)
    assert np.array_equal(env.obj_group.numpy()[~mask.numpy()], rows[~mask.numpy()])          # the other envs keep their groups
    rs = np.random.RandomState(4)                                                                # the first draws of the env's generator are the first env's counts
    assert group_ids(sample_group_counts(rs, 5, *env.sample_lam)).tolist() == rows[0].tolist()


# ------------------------------------------------------------------------------------------------ public surface
def test_group_keywords_and_what_is_refused_emul(emul_lib):
    kw = dict(batch_size=2, device="cpu", lib=emul_lib, **FAST)
    env = blocks.make_env(**kw)
    assert env.obj_group is None and env.group_mode == "distinct" and not env.post.obj_group             # the default allocates nothing
    assert blocks.make_env(parameters={"simulation_params": {"object_groups": "single"}}, **kw).obj_group.tolist() == [[0] * 5] * 2
    assert blocks.make_env(parameters={"simulation_params": {"object_groups": [2, 1, 2]}}, **kw).obj_group.tolist() == [[0, 0, 1, 2, 2]] * 2
    assert blocks.make_env(parameters={"simulation_params": {"object_groups": [{"count": 1}, {"count": 4}]}}, **kw).obj_group.tolist() == [[0, 1, 1, 1, 1]] * 2
    env = blocks.make_env(parameters={"simulation_params": {"object_groups": "sample"}}, constants={"sample_lam_low": 0.1, "sample_lam_high": 5.0}, **kw)
    assert env.group_mode == "sample" and env.sample_lam == (0.1, 5.0)
    assert blocks.make_env(parameters={"simulation_params": {"object_groups": "sample"}}, **kw).sample_lam == (1.0, 8.0)
    with pytest.raises(ValueError, match="sum to num_objects"):
        blocks.make_env(parameters={"simulation_params": {"object_groups": [2, 2]}}, **kw)
    with pytest.raises(NotImplementedError, match="material_args"):
        blocks.make_env(parameters={"simulation_params": {"object_groups": [{"count": 5, "material_args": {"type": "rubber"}}]}}, **kw)
    with pytest.raises(NotImplementedError, match="color"):
        blocks.make_env(parameters={"simulation_params": {"object_groups": [{"count": 5, "color": [1, 0, 0, 1]}]}}, **kw)
    with pytest.raises(ValueError, match="reach"):
        BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, num_objects=1, goal_kind="reach", object_groups="single", **FAST)
    with pytest.raises(ValueError):
        BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, object_groups="pairs", **FAST)
    # the C ABI refuses groups for the reach kinds too
    env = BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, num_objects=1, goal_kind="reach", **FAST)
    row = torch.zeros(1, 1, dtype=torch.int32)
    env.post.obj_group = row.data_ptr()
    with pytest.raises(_native.NativeError, match="obj_group"):
        env._post()
    from robogym_amd.envs.rearrange import ycb
    assert ycb.make_env(parameters={"simulation_params": {"object_groups": [4, 4]}}, **kw).obj_group.tolist() == [[0] * 4 + [1] * 4] * 2


def test_blocks_duplicate_surface_and_keys_emul(emul_lib):
    kw = dict(batch_size=1, device="cpu", lib=emul_lib, **FAST)
    env = blocks_duplicate.make_env(**kw)
    assert env.N == 2 and env.wrapped and env.goal_kind == 0 and env.obj_group.tolist() == [[0, 0]]
    env5 = blocks_duplicate.make_simple_env(parameters={"simulation_params": {"num_objects": 5}}, **kw)
    assert env5.N == 5 and env5.wrapped is False and env5.obj_group.tolist() == [[0] * 5]
    with pytest.raises(NotImplementedError, match="1, 2, 5"):
        blocks_duplicate.make_env(parameters={"simulation_params": {"num_objects": 3}}, **kw)
    with pytest.raises(ValueError, match="one group"):
        blocks_duplicate.make_env(parameters={"simulation_params": {"object_groups": "sample"}}, **kw)
    # observation and info keys are those of blocks (tests/golden/rearrange_obs_keys.json: `RearrangeEnv._observe_simple`'s own)
    ref = json.load(open(os.path.join(GOLDEN, "rearrange_obs_keys.json")))
    plain = blocks.make_simple_env(parameters={"simulation_params": {"num_objects": 5}}, **kw)
    obs = env5.reset()
    assert list(obs) == [k for k, _ in ref] == [k for k, _ in OBS_KEYS] == list(plain.reset())
    assert list(env5.info()) == list(plain.info())
    assert {k: tuple(v.shape) for k, v in obs.items()} == {k: tuple(v.shape) for k, v in plain.observe().items()}


# ------------------------------------------------------------------------------------------------ the env over pipelined resets
def _duplicate_sequence(lib, device, B, N, nsteps, **kw):
    """blocks_duplicate over goal time-outs and a 1 + 1 + 1 step recipe, the device recipe and its host twin side by side: no status bit, constant group rows, and
    agreement on everything the two random streams have no part in -- the whole row until an env's first restart, the episode bookkeeping throughout (a time-out
    does not depend on where the blocks were put)."""
    args = dict(lib=lib, n_substeps=1) if lib is not None else {}
    mk = lambda device_reset: blocks_duplicate.make_simple_env(
        batch_size=B, device=device, parameters={"simulation_params": {"num_objects": N}}, constants={"max_timesteps_per_goal_per_obj": 1}, stabilize_steps=1,
        n_random_initial_steps=1, settle_steps=1, pipelined_reset=True, device_reset=device_reset, starting_seed=9, **args, **kw)
    dev_env, host_env = mk(True), mk(False)
    for env in (dev_env, host_env):
        env.reset()
    assert torch.equal(dev_env.packed, host_env.packed)
    fresh = torch.ones(B, dtype=torch.bool, device=dev_env.device)
    ends = starts = 0
    for k in range(nsteps):
        act = torch.zeros((B, dev_env.action_dim), device=dev_env.device)
        out = [env.step(act) for env in (dev_env, host_env)]
        for env in (dev_env, host_env):
            env.sync()
            assert int(env.sim.status.max()) == 0 and int(env.solver_sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
            assert env.obj_group.tolist() == [[0] * N] * B
        (obs, rew, done, info), (obs_h, rew_h, done_h, info_h) = out
        assert torch.equal(obs["obj_pos"][fresh], obs_h["obj_pos"][fresh]) and torch.equal(rew[fresh], rew_h[fresh]) and torch.equal(dev_env.packed[fresh], host_env.packed[fresh])
        off = info["objects_off_table"] | info_h["objects_off_table"]
        if not bool(off.any()):
            assert torch.equal(done, done_h) and torch.equal(info["resetting"], info_h["resetting"]) and torch.equal(info["episode_started"], info_h["episode_started"])
            assert torch.equal(dev_env.steps, host_env.steps)
        fresh &= ~done
        ends += int(done.sum()); starts += int(info["episode_started"].sum())
        st = info["episode_started"]
        if bool(st.any()):          # the first observation of a new episode is measured through the match: rel = matched goal - object
            o, gl = obs["obj_pos"][st].cpu().numpy().astype(np.float64), dev_env.goal[st][..., :3].cpu().numpy().astype(np.float64)
            rel = obs["rel_goal_obj_pos"][st].cpu().numpy()
            for b in range(len(o)):
                m = greedy_group_match(o[b], gl[b], np.zeros(N, dtype=int))
                assert np.abs(rel[b] - (gl[b][m] - o[b])).max() < 1e-5
    assert ends >= B and starts >= B and int(dev_env.placement_failed.max()) == 0


@pytest.mark.parametrize("N", [2, 5])
def test_blocks_duplicate_pipelined_device_resets_emul(emul_lib, N):
    _duplicate_sequence(emul_lib, "cpu", 2, N, nsteps=12)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [2, 5])
def test_blocks_duplicate_pipelined_device_resets_gpu(N):
    _duplicate_sequence(None, "cuda:0", 64, N, nsteps=30)


# ------------------------------------------------------------------------------------------------ the train goal (goal kind 5, envs/rearrange/blocks_train.py)
def test_host_train_goal_replays_the_reference_code(golden):
    """ratio in {1, 0.5, 0} x (pickup, stack) in {(0, 0), (1, 0), (0, 1)}, four seeds each: positions to 1e-6, the generator consumed draw for draw; the tower's members
    come from the global np.random in the reference, so for the stack only the tower's shape is compared."""
    from robogym_amd.envs.rearrange.blocks import move_one_object_to_the_air_with_restrictions, place_targets_with_goal_distance_ratio

    g = golden
    assert len(g["train_seed"]) == 36
    for t in range(36):
        rs = np.random.RandomState(int(g["train_seed"][t]))
        ratio, pp, sp = float(g["train_ratio"][t]), float(g["train_pickup"][t]), float(g["train_stack"][t])
        before, ok = place_targets_with_goal_distance_ratio(rs, g["train_centre"][t], g["train_half"][t], g["train_table_pos"], g["train_table_size"], g["train_area_offset"],
                                                            g["train_area_size"], g["train_obj"][t], ratio, 0.06)
        assert ok and np.abs(before - g["train_before"][t]).max() < 1e-6, t
        after = move_one_object_to_the_air_with_restrictions(rs, before.copy(), (0.05, 0.25), 0.0254, pp, sp, ratio)
        if sp == 0.0:
            assert np.abs(after - g["train_after"][t]).max() < 1e-6 and rs.uniform() == g["train_next_draw"][t], t
            if pp == 1.0:
                assert ((after - before)[:, 2] != 0).sum() == (1 if ratio > 0 else 0)
        else:
            dz, dz_ref = np.sort((after - before)[:, 2]), np.sort((g["train_after"][t] - g["train_before"][t])[:, 2])
            assert np.abs(dz - dz_ref).max() < 1e-6 and 1 <= (dz > 0).sum() <= 4, (t, dz, dz_ref)
            top = np.nonzero((after - before)[:, 2] > 0)[0]
            base = [i for i in range(5) if i not in top and np.abs(after[top[0], :2] - after[i, :2]).max() < 1e-12]
            assert len(base) == 1 and np.abs(after[top, :2] - after[base[0], :2]).max() < 1e-12


def _train_goal_properties(env, goal, qpos, ratios, pp, sp):
    """[R, N, 3] goals of the envs whose qpos rows are `qpos`: inside the area, apart from one another, within ratio x the area's diagonal of their objects and
    goal_distance_min away from them unless the proposal itself was closer; a pickup raises one goal by U(height_range) x ratio, a stack makes a tower."""
    N, R = env.N, len(goal)
    yaw = env.goal_rot[..., 2].cpu().numpy().astype(np.float64)[:R] if goal.shape[0] == env.B else None
    (off_x, off_y, _), (width, height, _) = env.placement_area()
    lo = np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2]
    z0 = env.obj_half[:, 2] + env.table_size[2] + env.table_pos[2] - env.obj_center[:, 2]
    dz = goal[..., 2] - z0
    xy = goal[..., :2]
    obj = np.stack([qpos[:, qa:qa + 2] for qa in env.obj_q], 1)
    half = 0.0254 * np.sqrt(2.0)                                 # (any yaw: the yawed box is no larger; the blocks' centres are their body origins)
    assert np.abs(env.obj_center).max() < 1e-9
    raised = dz > 1e-6
    assert (np.abs(dz[~raised]) < 1e-6).all()
    if sp == 0.0:
        flat = np.ones(R, dtype=bool)
    else:
        flat = ~raised.any(1)
    # inside the area (the box of the smallest yawed block: half 0.0254)
    assert (xy >= lo + 0.0254 - 1e-5).all() and (xy <= lo + [width, height] - 0.0254 + 1e-5).all()
    # apart: the centres of two non-overlapping yawed boxes differ by at least 2 x 0.0254 on one axis
    for i in range(N):
        for j in range(i):
            d = np.abs(xy[flat, i] - xy[flat, j]).max(-1)
            assert (d >= 2 * 0.0254 - 1e-5).all(), (i, j, d.min())
    dist = np.linalg.norm(xy - obj, axis=-1)
    in_tower = raised if sp > 0 else np.zeros_like(raised)
    diag = np.hypot(width, height)
    r = ratios[:, None].repeat(N, 1)[~in_tower]
    # within ratio x diagonal -- or AT goal_distance_min where the pull stops there (the clip's lower bound: a ratio of 0 leaves every goal 0.06 m from its object)
    assert (dist[~in_tower] <= np.maximum(r * diag, env.goal_distance_min) + 1e-5).all()
    assert ((dist[~in_tower] >= env.goal_distance_min - 1e-5) | (dist[~in_tower] <= r * env.goal_distance_min + 1e-5)).all()
    if pp == 1.0:
        assert (raised.sum(1) == (ratios > 0)).all()
        h = dz[raised] / ratios[:, None].repeat(N, 1)[raised]
        assert (h >= env.height_range[0] - 1e-5).all() and (h <= env.height_range[1] + 1e-5).all() and h.std() > 0.01
    elif sp == 1.0:
        k = raised.sum(1)
        assert (k >= 1).all() and (k <= N - 1).all() and (N == 2 or len(set(k.tolist())) > 1)
        for b in range(R):
            steps = np.sort(dz[b][raised[b]]) / (2 * env.object_size)
            assert np.abs(steps - np.arange(1, k[b] + 1)).max() < 1e-4
            top = np.nonzero(raised[b])[0]
            base = [i for i in range(N) if not raised[b, i] and np.abs(xy[b, i] - xy[b, top[0]]).max() < 1e-6]
            assert len(base) == 1 and np.abs(xy[b, top] - xy[b, base[0]]).max() < 1e-6
    else:
        assert not raised.any()


def _device_train_goals(lib, device, B, N, pp, sp):
    env = _env(lib, device, B, N, goal_kind="train", pickup_proba=pp, stacking_proba=sp, goal_distance_ratio=np.tile([1.0, 0.5, 0.0, 0.25], B // 4), stabilize_steps=0,
               n_random_initial_steps=0, settle_steps=0, pipelined_reset=True, device_reset=True, starting_seed=5)
    r = env.recipe
    env.stage.zero_(); env.done.fill_(True); env.goal_reset.fill_(False)
    for step, done in ((1, True), (2, False)):       # every env is told its episode ended, then (zero-length recipe stages) that it starts: the first goal of each env
        env.done.fill_(done)
        r.step = step
        _native.check(env._L, env._L.ra_env_recipe_step(env.sim._bh, env.solver_sim._bh, ctypes.byref(r), env._stream()), "ra_env_recipe_step")
    env.sync()
    assert bool(env.episode_started.all()) and int(env.placement_failed.max()) == 0
    goal, qpos = env.goal[..., :3].cpu().numpy().astype(np.float64), env.sim.qpos.cpu().numpy().astype(np.float64)
    _train_goal_properties(env, goal, qpos, env.goal_distance_ratio.cpu().numpy().astype(np.float64), pp, sp)
    assert np.abs(env.qpos_goal.cpu().numpy()[:, env.obj_q[0]:env.obj_q[0] + 3] - goal[:, 0]).max() < 1e-6


TRAIN_CASES = [(2, 0.0, 0.0), (5, 0.0, 0.0), (5, 1.0, 0.0), (5, 0.0, 1.0), (2, 0.0, 1.0)]


@pytest.mark.parametrize("N,pp,sp", TRAIN_CASES)
def test_device_train_goal_properties_emul(emul_lib, N, pp, sp):
    _device_train_goals(emul_lib, "cpu", 64, N, pp, sp)


@pytest.mark.gpu
@pytest.mark.parametrize("N,pp,sp", TRAIN_CASES)
def test_device_train_goal_properties_gpu(N, pp, sp):
    _device_train_goals(None, "cuda:0", 1024, N, pp, sp)


@pytest.mark.parametrize("pp,sp", [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0)])
def test_host_train_goal_properties_emul(emul_lib, pp, sp):
    """the host recipe's goals over 64 envs, the same properties; the restated reference routine never runs out of restarts on the 5-block world"""
    B = 64
    env = _env(emul_lib, "cpu", B, 5, goal_kind="train", pickup_proba=pp, stacking_proba=sp, goal_distance_ratio=np.tile([1.0, 0.5, 0.0, 0.25], B // 4), starting_seed=6)
    rows = np.arange(B)
    yaw = env._begin_episode_state(rows, torch.arange(B))
    goal = env._goal_positions(rows, yaw)
    assert env.host_placement_failed == 0
    _train_goal_properties(env, goal, env.sim.qpos.numpy().astype(np.float64), env.goal_distance_ratio.numpy().astype(np.float64), pp, sp)


def test_blocks_train_surface_emul(emul_lib):
    from robogym_amd.envs.rearrange import blocks_train

    kw = dict(batch_size=2, device="cpu", lib=emul_lib, **FAST)
    env = blocks_train.make_env(**kw)
    assert env.N == 5 and env.goal_kind == 5 and env.post.goal_kind == 0 and env.group_mode == "sample" and env.wrapped and not env.reach
    assert env.goal_distance_ratio.tolist() == [1.0, 1.0] and abs(env.goal_distance_min - 0.06) < 1e-12 and env.pickup_proba == env.stacking_proba == 0.0
    assert env.height_range == (0.05, 0.25) and env.object_size == 0.0254
    env = blocks_train.make_simple_env(parameters={"simulation_params": {"goal_distance_ratio": [0.5, 0.1], "goal_distance_min": 0.05, "object_groups": "distinct"}},
                                       constants={"goal_args": {"pickup_proba": 0.3, "stacking_proba": 0.2, "height_range": (0.1, 0.2)}, "use_cuboid": True}, **kw)
    assert np.allclose(env.goal_distance_ratio.numpy(), [0.5, 0.1]) and env.pickup_proba == 0.3 and env.stacking_proba == 0.2 and env.height_range == (0.1, 0.2) and env.obj_group is None
    assert blocks_train.make_env(parameters={"object_scale_low": 0.0, "object_scale_high": 0.0}, constants={"use_cuboid": True}, **kw).N == 5      # the reference's no-op
    with pytest.raises(NotImplementedError, match="use_cuboid"):
        blocks_train.make_env(parameters={"object_scale_high": 0.3}, constants={"use_cuboid": True}, **kw)
    with pytest.raises(NotImplementedError, match="object_scale"):
        blocks_train.make_env(parameters={"object_scale_low": 0.3}, **kw)
    with pytest.raises(NotImplementedError, match="rot_dist_type"):
        blocks_train.make_env(constants={"goal_args": {"rot_dist_type": "icp"}}, **kw)
    with pytest.raises(ValueError):
        blocks_train.make_env(constants={"goal_args": {"pickup_proba": 0.8, "stacking_proba": 0.5}}, **kw)
    ref = json.load(open(os.path.join(GOLDEN, "rearrange_obs_keys.json")))
    plain = blocks.make_simple_env(**kw)
    assert list(env.reset()) == [k for k, _ in ref] == list(plain.reset()) and list(env.info()) == list(plain.info())


def _train_sequence(lib, device, B, nsteps):
    """blocks_train with pipelined device resets over goal time-outs and a 1 + 1 + 1 step recipe: no status bit, finite rows, episodes that end and restart with
    freshly sampled groups and goals that keep the train goal's properties."""
    from robogym_amd.envs.rearrange import blocks_train

    args = dict(lib=lib, n_substeps=1) if lib is not None else {}
    env = blocks_train.make_simple_env(batch_size=B, device=device, constants={"max_timesteps_per_goal_per_obj": 1, "goal_args": {"pickup_proba": 0.3, "stacking_proba": 0.3}},
                                       parameters={"simulation_params": {"goal_distance_ratio": 0.5}}, stabilize_steps=1, n_random_initial_steps=1, settle_steps=1,
                                       pipelined_reset=True, device_reset=True, starting_seed=3, **args)
    env.reset()
    ends = starts = 0
    for _ in range(nsteps):
        obs, rew, done, info = env.step(torch.zeros((B, env.action_dim), device=env.device))
        env.sync()
        assert int(env.sim.status.max()) == 0 and int(env.solver_sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
        rows = env.obj_group.cpu().numpy(); d = np.diff(rows, axis=1)
        assert (rows[:, 0] == 0).all() and ((d == 0) | (d == 1)).all()
        ends += int(done.sum()); st = info["episode_started"]; starts += int(st.sum())
        if bool(st.any()):
            assert torch.allclose(obs["goal_obj_pos"][st], env.goal[st][:, :, :3])
    assert ends >= B and starts >= B and int(env.placement_failed.max()) == 0


def test_blocks_train_pipelined_device_resets_emul(emul_lib):
    _train_sequence(emul_lib, "cpu", 2, nsteps=12)


@pytest.mark.gpu
def test_blocks_train_pipelined_device_resets_gpu():
    _train_sequence(None, "cuda:0", 64, nsteps=30)
