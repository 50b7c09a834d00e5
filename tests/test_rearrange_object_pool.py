"""Per-env object subsets of the rearrange envs (`object_pool`): an env uses n of its world's M objects, observation / goal slot i being world
object `object_perm[e, i]`, the others parked.  The identity permutation against the plain env (bit for bit), a relabelling of the same world at n = M, a two-of-five
subset against the 2-block world, the rows of a three-of-eight ycb subset against the objects they name, the sampler of ra_recipe_kernel, the grouped ycb env, the
surface and its refusals.  Every check runs twice: on the emulation harness (CPU, the same kernel source) and, `-m gpu`, on the MI355X."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import blocks, ycb, ycb_pickandplace
from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv, yawed_half
from robogym_amd.envs.rearrange.xml import load_blocks_model, load_ycb_model, object_bounding_boxes
from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv

PER_OBJECT_KEYS = ("obj_pos", "obj_rel_pos", "obj_vel_pos", "obj_rot", "obj_vel_rot", "goal_obj_pos", "goal_obj_rot", "rel_goal_obj_pos", "rel_goal_obj_rot", "obj_gripper_contact",
                   "obj_bbox_size", "obj_colors")
#: a yawed half extent or a rest height restated in float64 from float32 inputs: a handful of fp32 roundings (cosf, sinf, two products, three sums) of lengths below
#: 0.6 m (the table top's height), 6e-8 each -- 2e-6 leaves room for thirty of them and is a hundredth of the smallest difference between two of a set's objects
GEOMETRY_TOL = 2e-6
_models = {}


def _ycb_world(set_index):
    if set_index not in _models:
        _models[set_index] = load_ycb_model(8, set_index=set_index)
    return _models[set_index]


def _kw(lib, **more):
    """the recipe stages the neighbouring tests use: the shortest on the emulator (about one mj_step per env and second), a short real recipe on the GPU"""
    if lib is not None:
        kw = dict(device="cpu", lib=lib, n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
    else:
        kw = dict(device="cuda:0", n_substeps=40, stabilize_steps=10, n_random_initial_steps=1, settle_steps=5)
    kw.update(more)
    return kw


def _ok(*envs):
    for env in envs:
        env.sync()
        assert int(env.sim.status.max()) == 0
        if env.solver_sim is not None:
            assert int(env.solver_sim.status.max()) == 0


def _actions(env, rng, zero=False):
    a = np.zeros(env.action_shape, dtype=np.float32) if zero else rng.uniform(-1, 1, env.action_shape).astype(np.float32)
    a[:, 2] = -np.abs(a[:, 2])      # (downwards: towards the objects)
    return a


def _assert_padded_zero(env):
    """the packed row keeps the world's width: behind the n slots in use every per-object key is zero"""
    o, n = 0, env.num_objects_initial
    for k, w in env.obs_keys:
        width = env.nq if w == "nq" else (env.N * int(w[1]) if isinstance(w, str) else w)
        if isinstance(w, str) and w != "nq":
            assert not env.packed[:, o:o + width].view(env.B, env.N, int(w[1]))[:, n:].any(), k
        o += width
    assert o == env.obs_dim


def _forward_and_observe(env):
    env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
    env._observe_only()


# ------------------------------------------------------------------------------------------------ 1. off is untouched; the identity is bit-identical
def _identity_is_the_plain_env(lib):
    """5-block world, B = 2: the pool env with n = 5 and the identity pinned against the plain env of the same seed, over a device reset, three steps that each reach
    the goal (thresholds of 10: a new goal per step, the regoal branch), the episode end that the third success brings, the recipe and the next episode's first steps"""
    kw = _kw(lib, starting_seed=3, pipelined_reset=True, device_reset=True, successes_needed=3, success_threshold={"obj_pos": 10.0, "obj_rot": 10.0})
    plain, pool = BatchedBlockRearrangeEnv(2, num_objects=5, **kw), BatchedBlockRearrangeEnv(2, num_objects=5, object_pool=True, **kw)
    assert plain.object_perm is None and not plain.post.obj_perm and not plain.recipe.obj_perm and not plain.param_rows.obj_perm and not plain.recipe.obj_perm_next
    pool.set_object_perm_next(np.arange(5))
    plain.reset(on_device=True); pool.reset()
    rng = np.random.RandomState(1)
    ends = starts = 0

    def same(where):
        for name in ("packed", "goal", "reward", "done"):
            assert torch.equal(getattr(plain, name), getattr(pool, name)), (where, name)
        assert torch.equal(plain.sim.qpos, pool.sim.qpos), (where, "qpos")

    same("reset")
    steps = 4 + (1 if lib is not None else 16)      # (the GPU's recipe: 10 + 1 + 5 steps)
    for k in range(steps):
        a = torch.tensor(_actions(plain, rng), device=plain.device)
        o1, o2 = plain.step(a), pool.step(a)
        same(k)
        ends += int(o2[2].sum()); starts += int(o2[3]["episode_started"].sum())
        assert o2[0]["obj_pos"].shape == (2, 5, 3) and torch.equal(o1[0]["obj_pos"], o2[0]["obj_pos"])
    _ok(plain, pool)
    assert ends == 2 and starts == 2 and pool.object_set().tolist() == [[0, 1, 2, 3, 4]] * 2


def test_identity_is_the_plain_env_emul(emul_lib):
    _identity_is_the_plain_env(emul_lib)


@pytest.mark.gpu
def test_identity_is_the_plain_env_gpu():
    _identity_is_the_plain_env(None)


# ------------------------------------------------------------------------------------------------ 2. relabelling at n = M
def _relabelled_world(lib, rot_dist_type, nsteps):
    """ycb set 4, B = 2: the plain env E0 and the pool env E1 with n = 8 and a pinned permutation P, given the same world state and E0's goal rows slot-permuted.  The
    worlds are the same world, so qpos agrees bit for bit; slot i of E1 is slot P[i] of E0, bit for bit in every per-object key (one lane per object, the same inputs);
    flags, counters and reward are equal; goal_dist, a sum of at most 8 non-negative fp32 terms in another order, within 8 x 2^-23 relative."""
    P = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    kw = _kw(lib, starting_seed=2, device_reset=True, rot_dist_type=rot_dist_type, main_model=_ycb_world(4))
    e0, e1 = BatchedYcbRearrangeEnv(2, **kw), BatchedYcbRearrangeEnv(2, object_pool=True, **kw)
    e1.set_object_perm_next(P)
    e0.reset(); e1.reset()
    assert e1.object_set().tolist() == [P.tolist()] * 2 and e1.N == 8 and e1.num_active.tolist() == [8, 8]
    for s0, s1 in ((e0.sim, e1.sim), (e0.solver_sim, e1.solver_sim)):
        for f in ("qpos", "qvel", "ctrl", "pid", "qacc_warmstart", "mocap", "eq_data"):
            getattr(s1, f).copy_(getattr(s0, f))
    idx = torch.as_tensor(P, device=e0.device)
    for f in ("goal", "goal_rot", "static_obs"):
        getattr(e1, f).copy_(getattr(e0, f)[:, idx])
    assert e0.goal_in_area is None and e1.goal_in_area is None      # (the row exists with the placement-area masks only)
    e1.qpos_goal.copy_(e0.qpos_goal)
    for env in (e0, e1):
        _forward_and_observe(env)
    rng = np.random.RandomState(4)
    for step in range(nsteps):
        a = _actions(e0, rng)
        (o0, r0, d0, i0), (o1, r1, d1, i1) = (env.step(torch.tensor(a, device=env.device)) for env in (e0, e1))
        assert torch.equal(e0.sim.qpos, e1.sim.qpos) and torch.equal(o0["qpos"], o1["qpos"]), step
        for k in PER_OBJECT_KEYS:
            assert torch.equal(o1[k], o0[k][:, idx]), (step, k)
        if rot_dist_type == "icp":
            assert torch.equal(e1.icp_rel, e0.icp_rel[:, idx]), step
        assert torch.equal(d0, d1) and torch.equal(r0, r1) and torch.equal(o0["is_goal_achieved"], o1["is_goal_achieved"])
        for f in ("t", "steps", "ssl", "successes", "consecutive", "goal_reset", "trial_success", "objects_off_table", "env_crash"):
            assert torch.equal(getattr(e0, f), getattr(e1, f)), (step, f)
        g0, g1 = e0.goal_dist.cpu().numpy().astype(np.float64), e1.goal_dist.cpu().numpy().astype(np.float64)
        print("relabelled world (%s) step %d: goal_dist %s vs %s" % (rot_dist_type, step, g0.tolist(), g1.tolist()))
        assert np.all(np.abs(g0 - g1) <= 8 * 2.0 ** -23 * np.abs(g0))
    _ok(e0, e1)


@pytest.mark.parametrize("rot_dist_type", ["full", "icp"])
def test_relabelled_world_emul(emul_lib, rot_dist_type):
    _relabelled_world(emul_lib, rot_dist_type, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("rot_dist_type", ["full", "icp"])
def test_relabelled_world_gpu(rot_dist_type):
    _relabelled_world(None, rot_dist_type, 4)


# ------------------------------------------------------------------------------------------------ 3. a subset against the small world
def _subset_twin(lib, B, nsteps):
    """tests/test_rearrange_num_objects.py `_twin_worlds` with a permutation: the 5-block world whose envs use blocks P[0], P[1] = 3, 1 against the 2-block world, the
    small world's block i sitting in world block P[i]; that test's tolerances (per env.step SAME_HISTORY_TAIL x STEP_TOL, `nsteps` times that over the run; reward and
    done exactly).  No contact names a geom of a parked block; the parked blocks end within 1e-5 of their OWN parking poses."""
    from tests.test_rearrange_env import SAME_HISTORY_TAIL, STEP_TOL

    P = np.array([3, 1, 4, 0, 2])
    kw = _kw(lib, starting_seed=3, device_reset=True)
    big = BatchedBlockRearrangeEnv(B, num_objects=2, model=load_blocks_model(5), object_pool=True, **kw)
    small = BatchedBlockRearrangeEnv(B, num_objects=2, **kw)
    big.set_object_perm_next(P)
    big.reset(); small.reset()
    assert big.N == 5 and small.N == 2 and big.num_active.tolist() == [2] * B and big.object_set().tolist() == [[3, 1]] * B and small.sim.nq + 21 == big.sim.nq
    nq0, nv0 = small.obj_q[0], small.obj_v[0]      # (the rows in front of the blocks: the robot's, the same in both worlds)
    assert big.obj_q[0] == nq0 and big.obj_v[0] == nv0
    # the parked blocks sit at their own cells after the reset, the two in use on the table
    q = big.sim.qpos.cpu().numpy()
    for j in (2, 3, 4):
        assert np.abs(q[:, big.obj_q[P[j]]:big.obj_q[P[j]] + 7] - big.park_pose[P[j]]).max() < 1e-6, j
    for j in (0, 1):
        assert np.all(q[:, big.obj_q[P[j]] + 2] < big.table_height + 0.1), j
    for f, adr_b, adr_s, w, n0 in (("qpos", big.obj_q, small.obj_q, 7, nq0), ("qvel", big.obj_v, small.obj_v, 6, nv0), ("qacc_warmstart", big.obj_v, small.obj_v, 6, nv0)):
        dst, src = getattr(big.sim, f), getattr(small.sim, f)
        dst[:, :n0] = src[:, :n0]
        for i in range(2):
            dst[:, adr_b[P[i]]:adr_b[P[i]] + w] = src[:, adr_s[i]:adr_s[i] + w]
    for f in ("ctrl", "pid", "qpos", "qvel", "qacc_warmstart", "mocap", "eq_data"):
        getattr(big.solver_sim, f).copy_(getattr(small.solver_sim, f))
    big.sim.ctrl.copy_(small.sim.ctrl); big.sim.pid.copy_(small.sim.pid)
    big.goal[:, :2] = small.goal; big.goal_rot[:, :2] = small.goal_rot; big.static_obs[:, :2] = small.static_obs
    big.qpos_goal[:, :nq0] = small.qpos_goal[:, :nq0]
    for i in range(2):
        big.qpos_goal[:, big.obj_q[P[i]]:big.obj_q[P[i]] + 7] = small.qpos_goal[:, small.obj_q[i]:small.obj_q[i] + 7]
    for env in (big, small):
        _forward_and_observe(env)
    parked_bodies = {int(big.post.obj_body[int(p)]) for p in P[2:]}
    parked_geoms = {gi for gi, b in enumerate(big.model.arrays["geom_bodyid"]) if int(b) in parked_bodies}
    gather = list(range(nq0)) + [big.obj_q[P[i]] + k for i in range(2) for k in range(7)]      # the small world's qpos out of the big one's
    rng = np.random.RandomState(5)
    worst = {k: 0.0 for k in STEP_TOL}
    for step in range(nsteps):
        a = _actions(big, rng)
        outs = []
        for env in (big, small):
            obs, rew, done, info = env.step(torch.tensor(a, device=env.device))
            env.sync()
            outs.append((obs, rew.cpu().numpy().copy(), done.cpu().numpy().copy(), env.goal_dist.cpu().numpy().copy()))
        (ob, rb, db, gb), (os_, rs, ds, gs) = outs
        for k in STEP_TOL:
            x, y = ob[k].cpu().numpy().astype(np.float64), os_[k].cpu().numpy().astype(np.float64)
            x = x[:, gather] if k == "qpos" else x
            assert x.shape == y.shape, (k, x.shape, y.shape)      # (the pool env returns n slots per object key)
            worst[k] = max(worst[k], float(np.abs(x - y).max()))
        assert np.array_equal(rb, rs) and np.array_equal(db, ds), (step, rb, rs, db, ds)
        assert np.abs(gb[:, 0] - gs[:, 0]).max() < nsteps * max(1e-4, 2 * STEP_TOL["obj_pos"]) and np.abs(gb[:, 1] - gs[:, 1]).max() < nsteps * max(2e-3, 2 * STEP_TOL["obj_rot"])
        assert np.array_equal(ob["is_goal_achieved"].cpu().numpy(), os_["is_goal_achieved"].cpu().numpy())
        _assert_padded_zero(big)
        ncon = big.sim.scratch("dbg")[:, 3].cpu().numpy().astype(int)
        con = big.sim.scratch("contact").cpu().numpy().reshape(B, -1, 32)
        for r in range(B):
            geoms = {int(x) for c in con[r, :ncon[r]] if int(c[31]) != 2 for x in (c[27], c[28])}      # (kind 2: the finger coupling's equality record)
            assert not (geoms & parked_geoms), (step, r, sorted(geoms & parked_geoms))
        _ok(big, small)
    q = big.sim.qpos.cpu().numpy().astype(np.float64)
    for j in (2, 3, 4):
        d = np.abs(q[:, big.obj_q[P[j]]:big.obj_q[P[j]] + 7] - big.park_pose[P[j]]).max()
        print("parked world block %d: |pose - its parking pose| = %.2e" % (P[j], d))
        assert d < 1e-5, (P[j], d)
    print("subset twin (%d steps): worst error / (SAME_HISTORY_TAIL x STEP_TOL) per key: %s" % (nsteps, {k: round(worst[k] / max(SAME_HISTORY_TAIL * tl, 1e-12), 3) for k, tl in STEP_TOL.items()}))
    for k, tl in STEP_TOL.items():
        assert worst[k] <= nsteps * max(SAME_HISTORY_TAIL * tl, 1e-6), (k, worst[k])


def test_subset_twin_emul(emul_lib):
    _subset_twin(emul_lib, 2, 2)


@pytest.mark.gpu
def test_subset_twin_gpu():
    _subset_twin(None, 4, 6)


# ------------------------------------------------------------------------------------------------ 4. the rows say which object they are
def _boxes_apart_and_inside(env, xy_centre, half, n):
    """the yawed boxes [B, n] (centres and half extents in x, y) overlap nowhere and lie inside the placement area of n objects"""
    (off_x, off_y, _), (width, height, _) = env.placement_area(n)
    lo = np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2]
    assert np.all(xy_centre - half >= lo - 1e-5) and np.all(xy_centre + half <= lo + [width, height] + 1e-5)
    for i in range(n):
        for j in range(i):
            gap = np.abs(xy_centre[:, i] - xy_centre[:, j]) - (half[:, i] + half[:, j])
            assert np.all(gap.max(-1) >= -1e-5), (i, j, gap)


def _rows_name_their_objects(lib):
    """ycb set 5 (eight distinct objects), B = 4, n = 3, a different pinned permutation per env, pipelined device resets, goal time-out after 3 steps"""
    B, n = 4, 3
    model = _ycb_world(5)
    names = list(model.names["object_mesh"])
    assert len(set(names)) == 8
    rng = np.random.RandomState(11)
    P = np.stack([rng.permutation(8) for _ in range(B)])
    P2 = np.stack([np.roll(p, 3) for p in P])
    assert len({tuple(p[:n]) for p in P}) == B and not np.any(P[:, :n] == P2[:, :n])
    env = BatchedYcbRearrangeEnv(B, num_objects=n, main_model=model, object_pool=True, **_kw(lib, starting_seed=6, pipelined_reset=True, device_reset=True, max_timesteps_per_goal_per_obj=1))
    env.set_object_perm_next(P)
    obs = env.reset()
    bb = object_bounding_boxes(model, 8)
    centre, half = bb[:, :3], bb[:, 3:]
    bodies = np.array([model.name2id("body", "object%d" % i) for i in range(8)])
    rest_z = half[:, 2] - centre[:, 2] + env.table_height
    assert len(np.unique(np.round(rest_z, 4))) == 8      # (the eight differ: a wrong index shows)

    def check(obs, perm, where, rows=range(B)):
        """the envs `rows`, whose running episode has the permutations `perm` [B, 8]"""
        rows = list(rows)
        used = perm[rows, :n]
        assert env.object_set()[rows].tolist() == used.tolist(), where
        for k in PER_OBJECT_KEYS:
            assert obs[k].shape[:2] == (B, n), (where, k)
        assert obs["qpos"].shape == (B, env.nq) and obs["qpos_goal"].shape == (B, env.nq)
        xpos = env.sim.scratch("xpos").reshape(B, -1, 3)
        want = torch.stack([xpos[e, torch.as_tensor(bodies[perm[e, :n]], device=env.device)] for e in rows])
        assert torch.equal(obs["obj_pos"][rows], want), where
        yaw = env.yaw.cpu().numpy().astype(np.float64)[rows, :n]
        want_half = np.stack([yawed_half(half[u], y) for u, y in zip(used, yaw)])
        got_half = obs["obj_bbox_size"].cpu().numpy().astype(np.float64)[rows]
        assert np.abs(got_half - want_half).max() < GEOMETRY_TOL, (where, np.abs(got_half - want_half).max())
        goal = env.goal.cpu().numpy().astype(np.float64)[rows]
        assert np.abs(goal[:, :n, 2] - rest_z[used]).max() < GEOMETRY_TOL, (where, goal[:, :n, 2], rest_z[used])
        assert not goal[:, n:, :3].any() and not env.static_obs[rows][:, n:].any()
        _assert_padded_zero(env)
        assert env.placement_failed.tolist() == [0] * B, where
        # the goals' boxes: centre = origin + the yawed centre of the box
        gyaw = env.goal_rot.cpu().numpy().astype(np.float64)[rows, :n, 2]
        ghalf = np.stack([yawed_half(half[u], y) for u, y in zip(used, gyaw)])[..., :2]
        gc = np.stack([blocks.yawed_centre(centre[u], y) for u, y in zip(used, gyaw)])[..., :2]
        _boxes_apart_and_inside(env, goal[:, :n, :2] + gc, ghalf, n)
        # the parked five sit at their own cells
        q = env.sim.qpos.cpu().numpy().astype(np.float64)
        for e in rows:
            for p in perm[e, n:]:
                assert np.abs(q[e, env.obj_q[p]:env.obj_q[p] + 7] - env.park_pose[p]).max() < 1e-4, (where, e, p)

    # the placement of the reset: the objects' boxes, from the qpos the recipe wrote, before anything moved them far (one stabilising step on the emulator)
    check(obs, P, "reset")
    assert env.info()["object_names"] == [[names[p] for p in row[:n]] for row in P]
    act = torch.zeros(env.action_shape, device=env.device)
    obs, rew, done, info = env.step(act)
    check(obs, P, "step 1")
    q = env.sim.qpos.cpu().numpy().astype(np.float64)
    yaw = env.yaw.cpu().numpy().astype(np.float64)[:, :n]
    if lib is not None:      # (after one mj_step the objects are where the recipe put them, to a millimetre; the GPU's recipe lets them settle and move)
        oc = np.stack([blocks.yawed_centre(centre[P[e, :n]], yaw[e]) for e in range(B)])[..., :2]
        oh = np.stack([yawed_half(half[P[e, :n]], yaw[e]) for e in range(B)])[..., :2]
        xy = np.stack([[q[e, env.obj_q[p]:env.obj_q[p] + 2] for p in P[e, :n]] for e in range(B)])
        (off_x, off_y, _), (width, height, _) = env.placement_area(n)
        lo = np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2]
        assert np.all(xy + oc - oh >= lo - 2e-3) and np.all(xy + oc + oh <= lo + [width, height] + 2e-3)
    # a row written mid-episode waits for the next episode
    env.set_object_perm_next(P2)
    assert not bool(done.any())
    ended, started = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)      # per env: its first episode ended / its second one started
    want_names = lambda perm, e: [names[p] for p in perm[e, :n]]
    for k in range(2, 60):
        obs, rew, done, info = env.step(act)
        d, s_ = done.cpu().numpy().astype(bool), info["episode_started"].cpu().numpy().astype(bool)
        print("step %d: done %s goal_reset %s episode_started %s steps_since_last_goal %s" % (k, d.tolist(), info["goal_reset"].tolist(), s_.tolist(), info["steps_since_last_goal"].tolist()))
        got_names = list(info["object_names"])
        live = ~ended
        for e in np.nonzero(live)[0]:      # the old permutation holds until the episode's end, the terminal step's names among it
            assert got_names[e] == want_names(P, e), (k, e)
        if (live & ~d).any():
            check(obs, P, "step %d" % k, np.nonzero(live & ~d)[0])
        now = live & d
        ended |= now
        if now.any():      # latched where the episode ended: the recipe runs with the new objects
            assert env.object_set()[now].tolist() == P2[now, :n].tolist()
        first = ~live & ~started & s_
        if first.any():    # ... and the new one from the next episode's first observation
            check(obs, P2, "next episode (step %d)" % k, np.nonzero(first)[0])
            for e in np.nonzero(first)[0]:
                assert got_names[e] == want_names(P2, e), (k, e)
        started |= first
        if started.all():
            break
    assert ended.all() and started.all()
    _ok(env)


def test_rows_name_their_objects_emul(emul_lib):
    _rows_name_their_objects(emul_lib)


@pytest.mark.gpu
def test_rows_name_their_objects_gpu():
    _rows_name_their_objects(None)


def _initial_placement(lib):
    """The placement `ra_begin_recipe` makes under a non-identity permutation, read from `sim.qpos` straight after the recipe launch that ends the episodes -- no
    physics launch in between, so the rows hold what the kernel wrote, on the emulator and on the GPU alike.  ycb set 5, B = 4, n = 3, a permutation per env.  For slot
    i of env e, p = P[e][i]: the pose sits at world object p's qpos address, its quaternion is the z rotation by `yaw[e, i]`, its z is object p's rest height and the
    static observation's box object p's yawed half extents (GEOMETRY_TOL); the three yawed boxes -- object p's centre and half extents -- overlap nowhere and lie inside
    the placement area of three objects (1e-5, `_boxes_apart_and_inside`); the other five objects sit at their own parking poses.  The eight boxes and rest heights
    differ, so the identity or a stale row in place of the latched one fails every one of these."""
    B, n = 4, 3
    model = _ycb_world(5)
    P = np.array([[4, 6, 1, 0, 7, 2, 5, 3], [7, 2, 5, 3, 1, 0, 6, 4], [3, 0, 6, 5, 2, 7, 4, 1], [5, 7, 3, 6, 0, 4, 1, 2]])
    assert np.array_equal(np.sort(P, axis=1), np.tile(np.arange(8), (B, 1))) and not np.any(P[:, :n] == np.arange(n))      # (no slot in use holds the object of its own index)
    bb = object_bounding_boxes(model, 8)
    centre, half = bb[:, :3], bb[:, 3:]
    for goal_kind in ("object_state", "pickandplace"):
        env = BatchedYcbRearrangeEnv(B, num_objects=n, main_model=model, object_pool=True, goal_kind=goal_kind,
                                    **_kw(lib, starting_seed=9, device_reset=True, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0))      # (one stage of one step: the second launch starts the episode)
        rest_z = half[:, 2] - centre[:, 2] + env.table_height
        for rnd, perm in enumerate((P, np.stack([np.roll(p, 4) for p in P]))):      # (the second round: the row of the first must not linger)
            env.set_object_perm_next(perm)
            _recipe_launch_alone(env, True)
            used = perm[:, :n]
            assert env.object_perm.cpu().numpy().tolist() == perm.tolist() and env.placement_failed.tolist() == [0] * B
            q = env.sim.qpos.cpu().numpy().astype(np.float64)
            yaw = env.yaw.cpu().numpy().astype(np.float64)
            assert not yaw[:, n:].any() and np.all(yaw[:, :n] != 0)
            pose = np.stack([[q[e, env.obj_q[p]:env.obj_q[p] + 7] for p in perm[e]] for e in range(B)])      # [B, 8 slots, 7]
            want_quat = np.stack([np.cos(yaw[:, :n] / 2), 0 * yaw[:, :n], 0 * yaw[:, :n], np.sin(yaw[:, :n] / 2)], -1)
            assert np.abs(pose[:, :n, 3:] - want_quat).max() < 1e-6, (goal_kind, rnd)
            assert np.abs(pose[:, :n, 2] - rest_z[used]).max() < GEOMETRY_TOL, (goal_kind, rnd, pose[:, :n, 2], rest_z[used])
            oc = np.stack([blocks.yawed_centre(centre[used[e]], yaw[e, :n]) for e in range(B)])[..., :2]
            oh = np.stack([yawed_half(half[used[e]], yaw[e, :n]) for e in range(B)])
            _boxes_apart_and_inside(env, pose[:, :n, :2] + oc, oh[..., :2], n)
            so = env.static_obs.cpu().numpy().astype(np.float64)
            assert np.abs(so[:, :n, :3] - oh).max() < GEOMETRY_TOL and not so[:, n:].any(), (goal_kind, rnd)
            for e in range(B):
                assert np.abs(pose[e, n:] - env.park_pose[perm[e, n:]]).max() < 1e-6, (goal_kind, rnd, e)
            # the episode's first goal: the stage machine's next launch starts the episode (one stabilising step counted, no physics needed for the goal rows)
            _recipe_launch_alone(env, False)
            assert bool(env.episode_started.all())
            goal = env.goal.cpu().numpy().astype(np.float64)
            gyaw = env.goal_rot.cpu().numpy().astype(np.float64)[:, :n, 2]
            raised = goal[:, :n, 2] - rest_z[used]
            if goal_kind == "pickandplace":      # one SLOT in use raised by U(height_range), the others at their objects' rest heights
                assert np.all((np.abs(raised) < GEOMETRY_TOL).sum(1) == n - 1) and np.all((raised.max(1) >= 0.05 - 1e-6) & (raised.max(1) <= 0.25 + 1e-6)), raised
            else:
                assert np.abs(raised).max() < GEOMETRY_TOL, raised
            gc = np.stack([blocks.yawed_centre(centre[used[e]], gyaw[e]) for e in range(B)])[..., :2]
            gh = np.stack([yawed_half(half[used[e]], gyaw[e]) for e in range(B)])[..., :2]
            _boxes_apart_and_inside(env, goal[:, :n, :2] + gc, gh, n)
            qg = env.qpos_goal.cpu().numpy().astype(np.float64)
            for e in range(B):      # qpos_goal: slot i's goal at world object p's address, the parked objects at their own poses
                for i, p in enumerate(perm[e]):
                    want = goal[e, i, :3] if i < n else env.park_pose[p, :3]
                    assert np.abs(qg[e, env.obj_q[p]:env.obj_q[p] + 3] - want).max() < 1e-6, (goal_kind, rnd, e, i)
        _ok(env)


def test_initial_placement_by_world_object_emul(emul_lib):
    _initial_placement(emul_lib)


@pytest.mark.gpu
def test_initial_placement_by_world_object_gpu():
    _initial_placement(None)


# ------------------------------------------------------------------------------------------------ 5. the sampler
def _recipe_launch_alone(env, forced):
    """one launch of ra_recipe_kernel for every env, no physics: a forced episode end (the synchronous reset's first launch), or the stage machine's next step"""
    r = env.recipe
    env.active_row.fill_(1)
    r.active, r.sync_mode = ctypes.c_void_p(env.active_row.data_ptr()), _native.RA_SYNC_FORCED_END if forced else _native.RA_SYNC_PIPELINED
    try:
        env._recipe_launch()
    finally:
        r.active, r.sync_mode = None, _native.RA_SYNC_PIPELINED
    env.sync()


def _sampler(lib, B, rounds):
    n, M = 4, 8
    model = _ycb_world(0)
    make = lambda seed, **more: BatchedYcbRearrangeEnv(B, num_objects=more.pop("num_objects", n), main_model=model, **_kw(lib, starting_seed=seed, device_reset=True, **more))
    env, twin, other = make(5, object_pool=True), make(5, object_pool=True), make(6, object_pool=True)
    rows = []
    for k in range(rounds):
        for e in (env, twin, other):
            _recipe_launch_alone(e, True)
        rows.append(env.object_perm.cpu().numpy().copy())
        assert torch.equal(env.object_perm, twin.object_perm), k                     # the same seed: the same rows
        assert not torch.equal(env.object_perm, other.object_perm), k                # another seed: other rows
        assert env.num_active.tolist() == [n] * B
    rows = np.concatenate(rows)
    S = len(rows)
    assert S == 4096 and np.array_equal(np.sort(rows, axis=1), np.tile(np.arange(M), (S, 1)))      # every row a permutation
    assert len({tuple(r) for r in rows}) > S // 2                                                   # (8! orders: hardly a repeat; the rounds differ)
    p_use, p_first = n / M, 1.0 / M
    f_use = np.array([(rows[:, :n] == o).any(1).mean() for o in range(M)])
    f_first = np.array([(rows[:, 0] == o).mean() for o in range(M)])
    print("sampler, S = %d: in use %s (n / M = %.3f, bound %.4f); in slot 0 %s (1 / M = %.3f, bound %.4f)" % (
        S, np.round(f_use, 4).tolist(), p_use, 5 * np.sqrt(p_use * (1 - p_use) / S), np.round(f_first, 4).tolist(), p_first, 5 * np.sqrt(p_first * (1 - p_first) / S)))
    assert np.all(np.abs(f_use - p_use) < 5 * np.sqrt(p_use * (1 - p_use) / S))
    assert np.all(np.abs(f_first - p_first) < 5 * np.sqrt(p_first * (1 - p_first) / S))
    # a row that is no permutation, written straight to the device: a sampled one takes its place; the host setter refuses the same row
    bad = [0, 1, 2, 3, 4, 5, 6, 6]
    env.object_perm_next[0] = torch.tensor(bad, dtype=torch.int32, device=env.device)
    env.object_perm_next[1] = torch.tensor([0, 1, 2, 3, 4, 5, 6, 99], dtype=torch.int32, device=env.device)
    env.object_perm_next[2] = torch.tensor([7, 6, 5, 4, 3, 2, 1, 0], dtype=torch.int32, device=env.device)
    _recipe_launch_alone(env, True)
    got = env.object_perm.cpu().numpy()
    assert np.array_equal(np.sort(got, axis=1), np.tile(np.arange(M), (B, 1))) and got[2].tolist() == [7, 6, 5, 4, 3, 2, 1, 0]
    with pytest.raises(ValueError, match="object_pool"):
        env.set_object_perm_next(bad, rows=[0])
    for wrong in ([0, 1, 2], [[0, 1, 2, 3, 4, 5, 6, 8]], 3, [0.5] * 8, [-1, 0, 1, 2, 3, 4, 5, 6]):
        with pytest.raises(ValueError, match="object_pool"):
            env.set_object_perm_next(wrong)
    env.set_object_perm_next(None); assert bool((env.object_perm_next == -1).all())
    env.set_object_perm_next([1, 0, 2, 3, 4, 5, 6, 7], rows=[1]); env.set_object_perm_next(-1, rows=[0])
    assert env.object_perm_next[1].tolist() == [1, 0, 2, 3, 4, 5, 6, 7] and env.object_perm_next[0].tolist() == [-1] * 8
    _ok(env, twin, other)
    # the new stream took no existing draw: placement (yaw) and goal draws of the identity-pinned pool env with n = M are the plain env's, byte for byte
    stages = dict(stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
    small = min(B, 64)
    kw = _kw(lib, starting_seed=5, device_reset=True, main_model=model, **stages)
    plain, pinned = BatchedYcbRearrangeEnv(small, **kw), BatchedYcbRearrangeEnv(small, object_pool=True, **kw)
    pinned.set_object_perm_next(np.arange(M))
    for e in (plain, pinned):
        _recipe_launch_alone(e, True)       # the episode ends: yaws and placement drawn
        _recipe_launch_alone(e, False)      # the one stabilising step is counted: the episode starts, the first goal drawn
    assert bool(plain.episode_started.all()) and bool(plain.yaw.any()) and bool(plain.goal[:, :, :3].any())
    assert torch.equal(plain.yaw, pinned.yaw) and torch.equal(plain.goal, pinned.goal) and torch.equal(plain.sim.qpos, pinned.sim.qpos) and torch.equal(plain.static_obs, pinned.static_obs)


def test_sampler_emul(emul_lib):
    _sampler(emul_lib, 512, 8)


@pytest.mark.gpu
def test_sampler_gpu():
    _sampler(None, 1024, 4)


# ------------------------------------------------------------------------------------------------ 6. the grouped env
@contextlib.contextmanager
def _readback_is_an_error(device):
    """on the GPU the check of tests/test_rearrange_sync_reset.py (torch's sync debug mode, or its patched methods); on the emulator the patched methods"""
    if device.type == "cuda":
        from tests.test_rearrange_sync_reset import _sync_is_an_error

        with _sync_is_an_error() as how:
            yield how
        return

    def refuse(*a, **k):
        raise RuntimeError("a synchronising call inside step()")
    saved = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "nonzero")}
    try:
        for name in saved:
            setattr(torch.Tensor, name, refuse)
        yield "patched Tensor.cpu / item / tolist / nonzero"
    finally:
        for name, f in saved.items():
            setattr(torch.Tensor, name, f)


def _grouped(lib):
    B, n = 4, 3
    env = ycb.make_env(batch_size=B, parameters={"simulation_params": {"num_objects": n}}, object_sets=(0, 1), object_pool=True, starting_seed=4,
                       **_kw(lib, pipelined_reset=True, device_reset=True, max_timesteps_per_goal_per_obj=1))
    assert isinstance(env, ycb.GroupedYcbRearrangeEnv) and env.object_pool and env._device_trade and env.N == 8
    obs = env.reset()
    assert obs["obj_pos"].shape == (B, n, 3) and obs["qpos"].shape == (B, env.groups[0].nq)

    def names_fit(names, sets):
        assert len(names) == B
        for e in range(B):
            pool = env.object_names[int(sets[e])]
            assert len(names[e]) == n and len(set(names[e])) == n and set(names[e]) <= set(pool), (e, names[e], pool)

    gen = torch.Generator().manual_seed(2)
    ends = 0
    kept = []
    for k in range(8 if lib is not None else 30):
        a = torch.randint(0, 11, (B, 6), generator=gen).to(env.device)
        with _readback_is_an_error(env.device) as how:
            obs, rew, done, info = env.step(a)
        kept.append((info["object_names"], env._slot_of_step_dev))
        ends += int(done.sum())
        for key in ("obj_pos", "goal_obj_pos", "obj_bbox_size", "qpos"):
            assert bool(torch.isfinite(obs[key]).all()), (k, key)
        assert obs["obj_pos"].shape == (B, n, 3)
    print("grouped env: no readback inside step() by", how, "-", ends, "episode ends")
    for names, slots in kept:
        names_fit(names, slots.cpu().numpy() // env.b)
    names_fit(env._pool_names(env._slot_dev), env.object_set_of_env())
    assert ends >= 1 and env.object_set().shape == (B, n)
    # a batch-wide row goes through the env <-> slot tables: env e's slot gets env e's row
    P = np.stack([np.roll(np.arange(8), e + 1) for e in range(B)])
    env.set_object_perm_next(P)
    slots = env._slot
    full = torch.cat([g.object_perm_next for g in env.groups]).cpu().numpy()
    assert np.array_equal(full[slots], P)
    with pytest.raises(ValueError, match="object_pool"):
        env.set_object_perm_next([0] * 8)
    env.sync()
    assert int(env.status().max()) == 0


def test_grouped_env_emul(emul_lib):
    _grouped(emul_lib)


@pytest.mark.gpu
def test_grouped_env_gpu():
    _grouped(None)


# ------------------------------------------------------------------------------------------------ 7. surface and refusals
def _refusals(lib):
    kw = _kw(lib)
    base = dict(num_objects=2, object_pool=True, device_reset=True)
    five = load_blocks_model(5)
    cases = [dict(device_reset=False), dict(per_env_parameters=False), dict(goal_kind="stack"), dict(goal_kind="train"), dict(goal_kind="reach", num_objects=1),
             dict(goal_kind="fixed", relative_placements=[[0.2, 0.2], [0.6, 0.6]]), dict(object_groups="single"), dict(object_groups="sample"), dict(object_groups=[1, 1]),
             dict(initial_states={"obj_pos": np.zeros((2, 3)), "obj_quat": np.tile([1.0, 0, 0, 0], (2, 1))}), dict(goal_states=[{"obj_pos": np.zeros((2, 3)), "obj_quat": np.tile([1.0, 0, 0, 0], (2, 1))}]),
             dict(max_num_objects=5), dict(tcp_solver_mode="mocap")]
    for case in cases:
        args = dict(base, **case)
        with pytest.raises(NotImplementedError, match="object_pool"):
            BatchedBlockRearrangeEnv(2, **args, **kw)
    with pytest.raises(ValueError, match="object_pool"):
        BatchedBlockRearrangeEnv(2, num_objects=6, model=five, object_pool=True, device_reset=True, **kw)
    with pytest.raises(NotImplementedError, match="object_pool"):
        ycb.make_env(batch_size=2, parameters={"simulation_params": {"num_objects": 3, "max_num_objects": 8}}, object_pool=True, device_reset=True, **kw)
    env = BatchedBlockRearrangeEnv(2, model=five, **base, **kw)
    assert env.N == 5 and env.num_objects_initial == 2 and env.object_perm.shape == (2, 5) and bool((env.object_perm_next == -1).all())
    assert env.packed.shape == (2, 36 * 5 + 23 + 2 * env.nq + 4)      # (the packed row keeps the world's width)
    for call in (lambda: env.reset(on_device=False), lambda: env.reset_goals(on_device=False), lambda: env.set_num_objects_next(1)):
        with pytest.raises(NotImplementedError, match="object_pool"):
            call()
    plain = BatchedBlockRearrangeEnv(2, num_objects=2, device_reset=True, **kw)
    for call in (lambda: plain.set_object_perm_next(None), plain.object_set):
        with pytest.raises(ValueError, match="object_pool"):
            call()
    # the launches: obj_perm without num_active is an error code, as is the recipe's obj_perm without its obj_perm_next
    L = env._L
    env.param_rows.stages = _native.RA_ROWS_RESTORE | _native.RA_ROWS_PARK
    for args, fn, handles in ((env.post, L.ra_env_post_step, (env.sim._bh, env.solver_sim._bh)), (env.param_rows, L.ra_env_param_rows, (env.sim._bh,)),
                              (env.recipe, L.ra_env_recipe_step, (env.sim._bh, env.solver_sim._bh))):
        had, args.num_active = args.num_active, None
        try:
            assert fn(*handles, ctypes.byref(args), None) != 0 and b"obj_perm" in L.rg_last_error()
        finally:
            args.num_active = had
    had, env.recipe.obj_perm_next = env.recipe.obj_perm_next, None
    try:
        assert L.ra_env_recipe_step(env.sim._bh, env.solver_sim._bh, ctypes.byref(env.recipe), None) != 0 and b"obj_perm" in L.rg_last_error()
    finally:
        env.recipe.obj_perm_next = had
    _ok(env, plain)
    # ycb: the shipped 8-object world whatever the count, through both surfaces; without the option every refusal stays
    for mod in (ycb, ycb_pickandplace):
        e = mod.make_env(batch_size=2, parameters={"simulation_params": {"num_objects": 3}}, object_pool=True, device_reset=True, **kw)
        assert e.N == 8 and e.num_objects_initial == 3 and len(e.object_names) == 8 and e.observe()["obj_pos"].shape == (2, 3, 3)
        assert e.goal_kind_name == ("pickandplace" if mod is ycb_pickandplace else "object_state")
        _ok(e)
    with pytest.raises(NotImplementedError, match="a prefix of a set is no set of its own"):
        ycb.make_env(batch_size=2, parameters={"simulation_params": {"max_num_objects": 8}}, **kw)


def test_refusals_name_object_pool_emul(emul_lib):
    _refusals(emul_lib)


@pytest.mark.gpu
def test_refusals_name_object_pool_gpu():
    _refusals(None)


def _abi(L):
    """tests/test_rearrange_icp.py's check, for the four structs that grew: the library's sizes are the binding's, and the three headers declare the functions they
    declared (a new entry point would live in a header of its own)"""
    for name, struct in (("ra_post_args", _native.RaPostArgs), ("ra_recipe_args", _native.RaRecipeArgs), ("ra_icp_args", _native.RaIcpArgs), ("ra_param_rows_args", _native.RaParamRowsArgs)):
        assert getattr(L, name + "_size")() == ctypes.sizeof(struct), name
        fields = [f[0] for f in struct._fields_]
        assert "obj_perm" in fields and fields[-1] == ("obj_perm_next" if name == "ra_recipe_args" else "obj_perm"), (name, fields[-3:])      # appended
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = lambda h: sorted(set(re.findall(r"\b(ra_[a-z_0-9]+)\s*\(", open(os.path.join(root, "include", h)).read())))
    assert declared("rgstep.h") == ["ra_env_post_step", "ra_env_recipe_step", "ra_post_args_size", "ra_recipe_args_size"]
    assert declared("rgstep_icp.h") == ["ra_env_icp", "ra_icp_args_size"] and declared("rgstep_sync_reset.h") == ["ra_env_param_rows", "ra_param_rows_args_size"]
    assert set(_native.EXPORTS_ICP) == {"ra_env_icp", "ra_icp_args_size"} and set(_native.EXPORTS_SYNC_RESET) == {"ra_env_param_rows", "ra_param_rows_args_size"}


def test_abi_sizes_and_function_lists_emul(emul_lib):
    _abi(emul_lib)


def test_abi_sizes_and_function_lists_gfx950_build():
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robogym_amd", "csrc", "librgstep.so")
    assert os.path.exists(path), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    _abi(ctypes.CDLL(path))
