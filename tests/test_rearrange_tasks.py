"""The rearrange block tasks -- pick-and-place, stack, reach (state / det-state) on the blocks world, pick-and-place on the ycb world: the goal generators on the host
(numpy) and in ra_recipe_kernel / ra_post_step_kernel, against tests/golden/rearrange_tasks.npz (the reference's own goal code, tools/gen_golden_rearrange_tasks.py)
and by their properties over many envs.  CPU: host path and the kernel source on the emulation harness; `-m gpu`: the MI355X."""
import json
import os

import numpy as np
import pytest
import torch

from robogym_amd.envs.rearrange import blocks_pickandplace, blocks_reach, blocks_stack, ycb_pickandplace
from robogym_amd.envs.rearrange.blocks import DET_REACH_POINTS, OBS_KEYS, BatchedBlockRearrangeEnv

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FAST = dict(n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)


def _golden():
    return np.load(os.path.join(GOLDEN, "rearrange_tasks.npz"))


class ReplayRng:
    """Stands in for the env's RandomState: hands out recorded draws, in order, per method."""

    def __init__(self, **queues):
        self.q = {k: list(v) for k, v in queues.items()}

    def uniform(self, low=0.0, high=1.0, size=None):
        return np.array([self.q["uniform"].pop(0) for _ in range(int(np.prod(size or 1)))]).reshape(size or ())

    def randint(self, n, size=None):
        return np.array([self.q["randint"].pop(0) for _ in range(int(np.prod(size or 1)))]).reshape(size or ())

    def permutation(self, n):
        return np.array(self.q["permutation"].pop(0))


def _env(lib, device, B, **kw):
    args = dict(FAST) if lib is not None else dict(stabilize_steps=20, n_random_initial_steps=1, settle_steps=10)
    args.update(kw)
    return BatchedBlockRearrangeEnv(B, device=device, **(dict(lib=lib) if lib is not None else {}), **args)


# ------------------------------------------------------------------------------------------------ public surface
def test_task_modules_build_with_the_reference_defaults_emul(emul_lib):
    kw = dict(batch_size=1, device="cpu", lib=emul_lib, **FAST)
    for mod, name, N, kind in ((blocks_pickandplace, "blocks_pickandplace", 1, 1), (blocks_stack, "blocks_stack", 2, 2), (blocks_reach, "blocks_reach", 1, 3)):
        env = mod.make_env(**kw)
        assert env.N == N and env.goal_kind == kind and env.wrapped and mod.make_simple_env(**kw).wrapped is False
    assert blocks_stack.make_env(**kw).fixed_order is False and blocks_stack.make_env(constants={"fixed_order": True}, **kw).fixed_order is True
    assert blocks_reach.make_env(constants={"goal_generation": "det-state"}, **kw).goal_kind == 4
    assert blocks_reach.make_env(parameters={"simulation_params": {"target_height": 0.05}}, **kw).target_height == 0.05
    assert blocks_pickandplace.make_env(parameters={"simulation_params": {"num_objects": 5}}, **kw).N == 5
    env = ycb_pickandplace.make_simple_env(**kw)
    assert env.N == 8 and env.goal_kind == 1


def test_task_modules_reject_what_they_do_not_build_emul(emul_lib):
    kw = dict(batch_size=1, device="cpu", lib=emul_lib, **FAST)
    with pytest.raises(NotImplementedError, match="1, 2, 5"):
        blocks_pickandplace.make_env(parameters={"simulation_params": {"num_objects": 3}}, **kw)
    with pytest.raises(NotImplementedError, match="1, 2, 5"):
        blocks_stack.make_env(parameters={"simulation_params": {"num_objects": 4}}, **kw)
    with pytest.raises(NotImplementedError):
        blocks_reach.make_env(parameters={"simulation_params": {"num_objects": 2}}, **kw)
    with pytest.raises(ValueError):
        blocks_reach.make_env(constants={"goal_generation": "image"}, **kw)
    with pytest.raises(NotImplementedError):
        blocks_stack.make_env(constants={"goal_generation": "state"}, **kw)      # (a reach constant: not the stack env's)
    with pytest.raises(NotImplementedError):
        blocks_pickandplace.make_env(constants={"fixed_order": True}, **kw)
    with pytest.raises(ValueError):
        BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, goal_kind="dominos", **FAST)


def test_observation_and_info_keys_match_the_golden_emul(emul_lib):
    keys = json.load(open(os.path.join(GOLDEN, "rearrange_task_keys.json")))
    kw = dict(batch_size=1, device="cpu", lib=emul_lib, **FAST)
    for name, mod in (("blocks_pickandplace", blocks_pickandplace), ("blocks_stack", blocks_stack), ("blocks_reach", blocks_reach)):
        env = mod.make_simple_env(**kw)
        obs = env.reset()
        assert list(obs) == keys[name]["obs"] == [k for k, _ in OBS_KEYS]
        assert sorted(k[len("goal_dist_"):] for k in env.info() if k.startswith("goal_dist_")) == keys[name]["goal_dist"]
    assert keys["ycb_pickandplace"]["goal_dist"] == ["obj_pos", "obj_rot"] and keys["ycb_pickandplace"]["obs"] == keys["blocks_stack"]["obs"]
    # the stack's relative goal gains gripper_pos, which the observation does not carry (RearrangeEnv._observe_simple reads rel_goal_obj_pos / rel_goal_obj_rot only)
    assert keys["blocks_stack"]["relative_goal"] == ["gripper_pos", "obj_pos", "obj_rot"] and "rel_goal_gripper_pos" not in keys["blocks_stack"]["obs"]


# ------------------------------------------------------------------------------------------------ golden replay, host path
def test_host_goal_kinds_replay_the_reference_goal_code_emul(emul_lib):
    """`_goal_positions` with the placement and the task's draws taken from the golden: the goals the reference's code made from the same inputs."""
    g = _golden()
    for N in (1, 5):
        env = _env(emul_lib, "cpu", 1, num_objects=N, goal_kind="pickandplace")
        for t in range(len(g["pnp%d_goal" % N])):
            env._grid_placement = lambda yaw, rows, n=None, t=t: g["pnp%d_placement" % N][t][None].copy()
            env._rng = ReplayRng(uniform=[g["pnp%d_height" % N][t]], randint=[g["pnp%d_index" % N][t]])
            assert np.abs(env._goal_positions(np.arange(1), np.zeros((1, N)))[0] - g["pnp%d_goal" % N][t]).max() < 1e-12
    for N, fixed in ((2, False), (5, False), (5, True)):
        tag = "stack%d%s" % (N, "_fixed" if fixed else "")
        env = _env(emul_lib, "cpu", 1, num_objects=N, goal_kind="stack", fixed_order=fixed)
        for t in range(len(g[tag + "_goal"])):
            env._free_placement_of_object0 = lambda yaw0, n=None, t=t: g[tag + "_bottom"][t].copy()
            env._rng = ReplayRng(permutation=[] if fixed else [g[tag + "_order"][t]])
            assert np.abs(env._goal_positions(np.arange(1), np.zeros((1, N)))[0] - g[tag + "_goal"][t]).max() < 1e-12
    env = _env(emul_lib, "cpu", 1, num_objects=1, goal_kind="reach")
    qa = env.obj_q[0]
    for t in range(8):
        env._free_placement_of_object0 = lambda yaw0, n=None, t=t: g["reach_placement"][t].copy()
        before = env.sim.qpos[0].clone()
        got = env._goal_positions(np.arange(1), np.zeros((1, 1)))[0]
        assert np.abs(got - g["reach_goal"][t]).max() < 1e-12
        q = env.sim.qpos[0]
        assert np.abs(q[qa:qa + 3].numpy() - g["reach_moved"][t][0]).max() < 1e-6                     # set_object_pos: the position ...
        assert torch.equal(q[qa + 3:], before[qa + 3:]) and torch.equal(q[:qa], before[:qa])             # ... and nothing else
    env = _env(emul_lib, "cpu", 2, num_objects=1, goal_kind="det-reach")
    for t in range(5):
        got = env._goal_positions(np.arange(2), np.zeros((2, 1)))
        assert np.abs(got - g["det_goal"][t][None]).max() < 1e-12
        assert np.abs(env.sim.qpos[:, qa:qa + 3].numpy() - g["det_moved"][t]).max() < 1e-6


def test_goal_distance_restatements_match_the_reference_code():
    """What the post kernel computes for stack and reach, restated in numpy, against the reference's goal_distance / current_state / reach reward."""
    g = _golden()
    rel = g["stackd_goal_pos"] - g["stackd_cur_pos"]
    assert np.abs(np.linalg.norm(rel, axis=-1) - g["stackd_obj_pos"]).max() < 1e-12
    gp = g["stackd_cur_pos"] - g["stackd_grip"]
    assert np.abs(gp - g["stackd_rel_gripper_pos"]).max() < 1e-12 and np.abs(np.linalg.norm(gp, axis=-1) - g["stackd_gripper_pos"]).max() < 1e-12
    assert np.array_equal(g["stackd_contact"].sum(-1), g["stackd_grasped"])
    cs = g["reach_current_state"][:, 0]
    assert np.array_equal(cs[:, :3], g["reach_site"]) and np.all(cs[:, 3:] == 0)
    assert np.abs((g["reach_prev_dist"] - g["reach_cur_dist"]).sum(-1) - g["reach_reward"]).max() < 1e-12
    assert np.abs(g["det_moved"][:2, 0] - DET_REACH_POINTS[[1, 0]]).max() == 0


# ------------------------------------------------------------------------------------------------ properties over many envs
def _check_goal_properties(env, goal, yaw, qpos=None):
    """goal [B, N, 3] of `env`'s task, drawn for objects of yaw [B, N]."""
    B, N = goal.shape[:2]
    top = env.table_height + env.obj_half[:, 2] - env.obj_center[:, 2]           # body origin of an object resting on the table
    (off_x, off_y, _), (width, height, _) = env.placement_area()
    lo = np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2]
    if env.goal_kind == 1:
        lift = goal[..., 2] - top
        up = lift > 1e-4
        assert np.all(up.sum(1) == 1) and lift[up].min() >= 0.05 - 1e-5 and lift[up].max() <= 0.25 + 1e-5 and np.all(np.abs(lift[~up]) < 1e-5)
        if N > 1:
            assert len(set(np.nonzero(up)[1])) == N                               # every object gets lifted by some env
    elif env.goal_kind == 2:
        assert np.abs(goal[..., :2] - goal[:, :1, :2]).max() < 1e-6
        level = (goal[..., 2] - top[0]) / (2 * env.object_size)
        assert np.abs(level - np.round(level)).max() < 1e-3
        order = np.round(level).astype(int)
        assert np.all(np.sort(order, 1) == np.arange(N))                          # a permutation of the levels
        if env.fixed_order:
            assert np.all(order == np.arange(N))
        elif N > 1 and B >= 32:
            assert len({tuple(o) for o in order}) > 1
        half = env._aabb_half(yaw)[:, 0, :2]
        assert np.all(goal[:, 0, :2] - half >= lo - 1e-5) and np.all(goal[:, 0, :2] + half <= lo + [width, height] + 1e-5)
    else:
        q = qpos[:, env.obj_q[0]:env.obj_q[0] + 3]
        assert np.abs(goal[:, 0, :2] - q[:, :2]).max() < 1e-6 and np.abs(goal[:, 0, 2] - q[:, 2] - env.target_height).max() < 1e-5
        if env.goal_kind == 3:
            assert np.abs(q[:, 2] - top[0]).max() < 1e-5
            half = env._aabb_half(yaw)[:, 0, :2]
            assert np.all(q[:, :2] - half >= lo - 1e-5) and np.all(q[:, :2] + half <= lo + [width, height] + 1e-5)


KINDS = [("pickandplace", 1, {}), ("pickandplace", 5, {}), ("stack", 2, {}), ("stack", 5, {}), ("stack", 5, {"fixed_order": True}), ("reach", 1, {}), ("det-reach", 1, {})]


@pytest.mark.parametrize("kind,N,extra", KINDS)
def test_host_goal_properties_over_many_envs_emul(emul_lib, kind, N, extra):
    env = _env(emul_lib, "cpu", 256, num_objects=N, goal_kind=kind, **extra)
    rows = np.arange(env.B)
    yaw = env._rng.uniform(0, 2 * np.pi, (env.B, N))
    goal = env._goal_positions(rows, yaw)
    _check_goal_properties(env, goal, yaw, env.sim.qpos.numpy().astype(np.float64))
    if kind == "det-reach":
        assert np.abs(goal[:, 0] - DET_REACH_POINTS[1] - [0, 0, 0.1]).max() < 1e-12


def _device_goals(lib, device, B, kind, N, **extra):
    """Every env is told its episode ended, then (zero-length recipe stages) that it starts: the kernel's first goal of each env."""
    env = _env(lib, device, B, num_objects=N, goal_kind=kind, stabilize_steps=0, n_random_initial_steps=0, settle_steps=0, pipelined_reset=True, device_reset=True, starting_seed=5, **extra)
    env.stage.zero_(); env.done.fill_(True); env.goal_reset.fill_(False)
    env._advance_recipes_device()
    env.done.fill_(False)
    env._advance_recipes_device()
    env.sync()
    assert bool(env.episode_started.all()) and int(env.placement_failed.max()) == 0
    goal = env.goal[..., :3].cpu().numpy().astype(np.float64)
    yaw = env.goal_rot[..., 2].cpu().numpy().astype(np.float64)
    qpos = env.sim.qpos.cpu().numpy().astype(np.float64)
    _check_goal_properties(env, goal, yaw, qpos)
    g7 = env.goal.cpu().numpy()
    qg = env.qpos_goal.cpu().numpy()
    for i, qa in enumerate(env.obj_q):       # qpos_goal: the current qpos with the objects at their goals (object_state.py:381-389)
        assert np.abs(qg[:, qa:qa + 7] - g7[:, i]).max() < 1e-6
    others = np.setdiff1d(np.arange(env.nq), np.concatenate([np.arange(qa, qa + 7) for qa in env.obj_q]))
    assert np.array_equal(qg[:, others], qpos[:, others])
    return env, goal


@pytest.mark.parametrize("kind,N,extra", KINDS)
def test_device_goal_properties_over_many_envs_emul(emul_lib, kind, N, extra):
    env, goal = _device_goals(emul_lib, "cpu", 64, kind, N, **extra)
    if kind == "det-reach":       # per env: 1 -> 0 -> 1 on the goals that follow
        assert np.array_equal(env.goal_index.numpy(), np.ones(64)) and np.abs(goal[:, 0] - DET_REACH_POINTS[1] - [0, 0, 0.1]).max() < 1e-6
        for want in (0, 1):
            env.goal_reset.fill_(True)
            env._advance_recipes_device()
            assert np.abs(env.goal[:, 0, :3].numpy() - DET_REACH_POINTS[want] - [0, 0, 0.1]).max() < 1e-6
            assert np.abs(env.sim.qpos[:, env.obj_q[0]:env.obj_q[0] + 3].numpy() - DET_REACH_POINTS[want]).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the post kernel's stack / reach terms
def _post_kernel_terms(lib, device, B, nsteps):
    """Stack: info's goal_dist_gripper_pos = sum |obj_pos - grip site|, goal_dist_grasped = the summed finger-contact flags of the observation.  Reach: goal_dist_obj_pos =
    |grip site - goal|, rel_goal_obj_pos = goal - grip site, rel_goal_obj_rot = the goal's rotation (the achieved one is zero), reward[1] = the decrease of the distance."""
    rng = np.random.RandomState(1)
    for kind, N in (("stack", 2), ("reach", 1)):
        env = _env(lib, device, B, num_objects=N, goal_kind=kind)
        obs = env.reset()
        s = env._grip_site
        prev = env.goal_dist[:, 0].cpu().numpy().astype(np.float64).copy()
        assert int(env.prev_valid.min()) == 1 and np.abs(env.prev_nsucc.cpu().numpy() - prev).max() < (1e-6 if kind == "reach" else 1e9)
        for _ in range(nsteps):
            a = rng.uniform(-1, 1, (B, 6)).astype(np.float32); a[:, 2] = -np.abs(a[:, 2])
            obs, rew, done, info = env.step(torch.tensor(a, device=env.device))
            env.sync()
            site = env.sim.scratch("site_xpos")[:, 3 * s:3 * s + 3].cpu().numpy().astype(np.float64)
            op = obs["obj_pos"].cpu().numpy().astype(np.float64)
            goal = env.goal[..., :3].cpu().numpy().astype(np.float64)
            if kind == "stack":
                dg = np.linalg.norm(op - site[:, None], axis=-1).sum(1)
                assert np.abs(info["goal_dist_gripper_pos"].cpu().numpy() - dg).max() < 1e-5
                assert np.array_equal(info["goal_dist_grasped"].cpu().numpy(), obs["obj_gripper_contact"].cpu().numpy().sum((1, 2)))
                assert np.abs(info["goal_dist_obj_pos"].cpu().numpy() - np.linalg.norm(goal - op, axis=-1).sum(1)).max() < 1e-5
            else:
                d = np.linalg.norm(goal[:, 0] - site, axis=-1)
                assert np.abs(info["goal_dist_obj_pos"].cpu().numpy() - d).max() < 1e-5
                assert np.abs(obs["rel_goal_obj_pos"][:, 0].cpu().numpy() - (goal[:, 0] - site)).max() < 1e-5
                assert np.abs(obs["rel_goal_obj_rot"][:, 0].cpu().numpy() - env.goal_rot[:, 0].cpu().numpy()).max() < 1e-5
                cur = info["goal_dist_obj_pos"].cpu().numpy().astype(np.float64)
                live = ~done.cpu().numpy()
                assert np.all(np.abs(rew[:, 1].cpu().numpy() - (prev - cur))[live] < 2e-6)
                prev = cur.copy()
            assert int(env.sim.status.max()) == 0
    return env


def test_post_kernel_stack_and_reach_terms_emul(emul_lib):
    _post_kernel_terms(emul_lib, "cpu", B=2, nsteps=1)


# ------------------------------------------------------------------------------------------------ pipelined resets through the task envs
def _task_sequence(lib, device, B, n_substeps, kind, N, device_reset, nsteps=12, **extra):
    """Goal time-out after 2 steps, a 1 + 1 + 1 step recipe: episodes end, restart inside the step calls with a fresh goal of the task's kind that the returned
    observation carries, and (reach) the block moved where the goal says."""
    kw = dict(lib=lib) if lib is not None else {}
    env = BatchedBlockRearrangeEnv(B, device=device, n_substeps=n_substeps, num_objects=N, goal_kind=kind, stabilize_steps=1, n_random_initial_steps=1, settle_steps=1,
                                   max_timesteps_per_goal_per_obj=2 if N == 1 else 1, pipelined_reset=True, device_reset=device_reset, starting_seed=11, **kw, **extra)
    env.reset()
    ends = starts = 0
    for k in range(nsteps):
        obs, rew, done, info = env.step(torch.zeros((B, env.action_dim), device=env.device))
        env.sync()
        assert int(env.sim.status.max()) == 0 and int(env.solver_sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
        ends += int(done.sum()); st = info["episode_started"]; starts += int(st.sum())
        if bool(st.any()):
            assert torch.allclose(obs["goal_obj_pos"][st], env.goal[st][:, :, :3])
            if env.reach:      # the forward after the move: the observation sees the block under its goal
                assert torch.allclose(obs["obj_pos"][st][:, 0, :2], env.goal[st][:, 0, :2], atol=1e-5)
            _check_goal_properties(env, env.goal[st][..., :3].cpu().numpy().astype(np.float64), env.goal_rot[st][..., 2].cpu().numpy().astype(np.float64),
                                   env.sim.qpos[st].cpu().numpy().astype(np.float64))
    assert ends >= B and starts >= B
    if device_reset:
        assert int(env.placement_failed.max()) == 0
    return env


@pytest.mark.parametrize("device_reset", [False, True])
def test_task_pipelined_reset_sequence_emul(emul_lib, device_reset):
    for kind, N in (("pickandplace", 1), ("stack", 2), ("reach", 1), ("det-reach", 1)):
        _task_sequence(emul_lib, "cpu", 2, 1, kind, N, device_reset, nsteps=8)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("device_reset", [False, True])
def test_task_pipelined_reset_sequence_gpu(device_reset):
    """device-reset and host-recipe twins of every task through the same protocol (the standard of test_rearrange_env.py's device-reset tests)"""
    for kind, N, extra in KINDS:
        _task_sequence(None, "cuda:0", 64, 40, kind, N, device_reset, nsteps=14, **extra)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,N,extra", KINDS)
def test_device_goal_properties_over_many_envs_gpu(kind, N, extra):
    _device_goals(None, "cuda:0", 4096, kind, N, **extra)


@pytest.mark.gpu
def test_post_kernel_stack_and_reach_terms_gpu():
    _post_kernel_terms(None, "cuda:0", B=64, nsteps=6)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2])
def test_one_and_two_block_worlds_step_matches_oracle_gpu(N):
    """The shipped 1- and 2-object worlds on rb_step_kernel against the unchanged OracleRearrangeEnv, under test_rearrange_env.py's re-synchronised protocol and tolerances."""
    from tests.test_rearrange_env import _check_steps

    mk = lambda: BatchedBlockRearrangeEnv(16, device="cuda:0", num_objects=N, n_substeps=40, stabilize_steps=20, n_random_initial_steps=1, settle_steps=10, starting_seed=3)
    env = _check_steps(None, "cuda:0", B=16, n_substeps=40, nsteps=6, make=mk, min_same_fraction=0.5)
    assert env.N == N


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["blocks_pickandplace", "blocks_stack", "blocks_reach", "ycb_pickandplace"])
def test_task_env_long_pipelined_device_reset_run_gpu(name):
    """B = 4096, `make_env` with the wrapper stack, pipelined device resets, 320 steps of random bin actions: no status bit, finite rows, episodes that end and restart."""
    mod = {"blocks_pickandplace": blocks_pickandplace, "blocks_stack": blocks_stack, "blocks_reach": blocks_reach, "ycb_pickandplace": ycb_pickandplace}[name]
    env = mod.make_env(batch_size=4096, device="cuda:0", constants={"max_timesteps_per_goal_per_obj": 5}, pipelined_reset=True, device_reset=True, starting_seed=2)
    env.reset()
    g = torch.Generator(device="cuda:0"); g.manual_seed(0)
    ends = torch.zeros((), dtype=torch.int64, device="cuda:0"); starts = torch.zeros_like(ends)
    for _ in range(320):
        idx = torch.randint(0, 11, env.action_shape, device="cuda:0", generator=g, dtype=torch.int32)
        obs, rew, done, info = env.step(idx)
        ends += done.sum(); starts += info["episode_started"].sum()
    env.sync()
    assert int(env.sim.status.max()) == 0 and int(env.solver_sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
    assert int(env.placement_failed.max()) == 0 and int(ends) >= 4096 and int(starts) >= 4096, (int(ends), int(starts))


# ------------------------------------------------------------------------------------------------ the 1- and 2-block worlds
@pytest.mark.parametrize("N", [1, 2])
def test_smaller_blocks_worlds_equal_the_mjcf_build(N):
    """`load_blocks_model(N)` cuts the world out of the shipped 5-block one: every array as compile_mjcf builds the MJCF with N blocks (the same bytes; the constants
    set_constants computes through a matrix inverse to 1e-12), the same name tables (tests/golden/rearrange_blocks_worlds.json, tools/gen_golden_blocks_worlds.py)."""
    import hashlib

    from robogym_amd.envs.rearrange.xml import load_blocks_model

    want = json.load(open(os.path.join(GOLDEN, "rearrange_blocks_worlds.json")))[str(N)]
    m = load_blocks_model(N)
    assert m.names == want["names"]
    assert set(m.arrays) == set(want["arrays"]) | set(want["computed"])
    for k, w in want["arrays"].items():
        a = np.ascontiguousarray(m.arrays[k])
        assert [list(a.shape), a.dtype.str, hashlib.sha256(a.tobytes()).hexdigest()] == [w["shape"], w["dtype"], w["sha256"]], k
    for k, v in want["computed"].items():
        a, v = np.asarray(m.arrays[k], dtype=np.float64).ravel(), np.asarray(v)
        assert a.shape == v.shape and np.all(np.abs(a - v) <= 1e-12 * np.maximum(1.0, np.abs(v))), k
    assert m.arrays["dims"][0] == 7 * N + 8 and m.names["body"][-1] == "target:object%d" % (N - 1)
