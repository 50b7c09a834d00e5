"""Recorded scenes of the rearrange family (robogym_amd/envs/rearrange/holdout.py; `initial_states` / `goal_states` / `advance_goals` of BatchedBlockRearrangeEnv;
ra_recipe_args' scene tables and ra_post_args' rel_dist, include/rgstep.h): an episode that starts from a recorded object state, goals that are recorded states,
and the relative distance of the reference's HoldoutObjectStateGoal.

Two tiers with the same protocols and shapes: the kernel source on the emulation harness and the gfx950 library through the C ABI; B = 4 or 8, N = 2 and 4,
S = 2 scenes, at most 3 goals per scene, n_substeps = 1 (the physics test alone runs the full 40 substeps).  The reference side is
tests/golden/rearrange_holdout.npz (tools/gen_golden_rearrange_holdout.py: the reference's own goal code on stubs), float64 numpy, or -- host route against device
route -- the other route, bit for bit."""
import os

import numpy as np
import pytest
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import blocks, holdout
from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STACKED4 = os.path.join(GOLDEN, "rearrange_holdout_initial_state_4_blocks_stacked.npz")
SAMPLE_GOAL = os.path.join(GOLDEN, "rearrange_holdout_goal_state_20200422_232013.npz")
FAST = dict(stabilize_steps=2, n_random_initial_steps=1, settle_steps=2)
NO_RECIPE = dict(stabilize_steps=0, n_random_initial_steps=0, settle_steps=0)      # no stabilisation, no random steps: the episode starts AT the recorded state
EMUL = dict(device="cpu", n_substeps=1)
GPU = dict(device="cuda:0", n_substeps=1)
ROT_TOL = 5e-5      # tests/test_rearrange_dominos.py's tolerance for the reference's rotation-distance code: angles and distances
_cache = {}


def _golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(GOLDEN, "rearrange_holdout.npz")))
    return _cache["g"]


def _kw(tier, lib, **kw):
    args = dict(tier, **FAST)
    if lib is not None:
        args["lib"] = lib
    args.update(kw)
    return args


def _shifted(state, shift=(0.0, 0.0, 0.0), tilt=None):
    """the state moved by `shift`, its first object turned by the quaternion `tilt` on top of what it has"""
    s = blocks.load_state(state, len(np.load(state)["obj_pos"]) if isinstance(state, str) else len(state["obj_pos"]))
    pos, quat = s[:, :3] + np.asarray(shift), s[:, 3:].copy()
    if tilt is not None:
        w1, v1, w2, v2 = tilt[0], np.asarray(tilt[1:]), quat[0, 0], quat[0, 1:]
        quat[0] = np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + np.cross(v1, v2)])
    return {"obj_pos": pos, "obj_quat": quat}


def _f32_state(state, n):
    """what the tables hold of a state: the first n rows, quaternions normalised in float64, cast to float32"""
    return blocks.load_state(state, n).astype(np.float32)


def _objects(env):
    return np.stack([env.sim.qpos[:, qa:qa + 7].cpu().numpy() for qa in env.obj_q], 1)


def _zero_action(env):
    return torch.zeros((env.B, env.action_dim), dtype=torch.float32, device=env.device)


def _angle_between(e_a, e_b):
    """the angle of the rotation between two orientations given as Euler angles (float64)"""
    qa, qb = blocks.euler2quat(np.asarray(e_a, dtype=np.float64)), blocks.euler2quat(np.asarray(e_b, dtype=np.float64))
    dot = np.clip(np.abs((qa * qb).sum(-1)), 0.0, 1.0)
    return 2.0 * np.arctan2(np.sqrt(np.maximum(1.0 - dot * dot, 0.0)), dot)


def _quat_angle_between(qa, qb):
    dot = np.clip(np.abs((np.asarray(qa, dtype=np.float64) * np.asarray(qb, dtype=np.float64)).sum(-1)), 0.0, 1.0)
    return 2.0 * np.arctan2(np.sqrt(np.maximum(1.0 - dot * dot, 0.0)), dot)


# ------------------------------------------------------------------------------------------------ 1. the goal layer against the reference's code
def _golden_layer(tier, lib):
    """The reference's `ObjectStateGoal.next_goal`, `relative_goal`, `goal_distance`, `HoldoutObjectStateGoal.goal_distance`, `rotate_bounding_box` and
    `_calculate_num_success` (the golden) against the env: the recorded sample goal state and three further orientations, as S = 2 scenes of two goals each.
    Positions and recorded quaternions as cast to float32: exact.  Angles and distances: 5e-5 (ROT_TOL).  Success bits: exact (the golden keeps 1e-3 from every
    threshold).  Gimbal orientations are left out of the golden (cos(pitch) >= 0.1 for every goal and current state): the float32 mat2euler of the env kernel
    branches at another cos(pitch) than the float64 reference, and near the lock the Euler angles are ill-conditioned; the relative rotation, which may come near
    its own lock, is compared as a rotation everywhere and per angle away from it."""
    g = _golden()
    N, T, B = g["goal_state_pos"].shape[1], g["cur_pos"].shape[1], 8
    thr = {k: float(g["threshold_" + k]) for k in ("obj_pos", "obj_rot", "rel_dist")}
    worst = dict(goal_rot=0.0, qpos_goal=0.0, bbox=0.0, rel_pos=0.0, rel_rot=0.0, rel_euler=0.0, dist=0.0, rel_dist=0.0)
    seen = set()
    all_states = [{"obj_pos": g["goal_state_pos"][c], "obj_quat": g["goal_state_quat"][c]} for c in range(4)]
    env = holdout.make_simple_env(B, parameters=dict(simulation_params=dict(num_objects=N), n_random_initial_steps=0),
                                  constants=dict(initial_state=all_states[:2], advance_goals=True, success_threshold=thr,
                                                 goal_args=dict(goal_states=[[all_states[0], all_states[2]], [all_states[1], all_states[3]]], rot_dist_type="mod90")),
                                  **_kw(tier, lib, **NO_RECIPE))
    for h in (0, 1):      # the episode's first goals: states 0 and 1 (whose boxes the recorded start shows); the next goals: states 2 and 3 (boxes: _episode_start)
        cs = [2 * h, 2 * h + 1]
        states = [all_states[c] for c in cs]
        if h == 0:
            obs = env.reset()
        else:
            env.post.rot_dist_type = blocks.ROT_DIST_TYPES["mod90"]
            env.goal_reset.fill_(True)
            env.reset_goals()
            obs = env.observe()
        env.sync()
        scene = np.arange(B) % 2
        c_of = np.array(cs)[scene]
        assert env.scene.tolist() == scene.tolist()
        table = np.stack([_f32_state(s, N) for s in states])[scene]
        assert np.array_equal(env.goal.cpu().numpy(), table) and np.array_equal(obs["goal_obj_pos"].cpu().numpy(), table[..., :3])
        assert np.array_equal(obs["goal_obj_pos"].cpu().numpy(), g["goal_obj_pos"][c_of].astype(np.float32))
        worst["goal_rot"] = max(worst["goal_rot"], np.abs(blocks.euler2quat(obs["goal_obj_rot"].cpu().numpy()) - blocks.euler2quat(g["goal_obj_rot"][c_of])).max(),
                                np.abs(obs["goal_obj_rot"].cpu().numpy() - g["goal_obj_rot"][c_of]).max())
        qg = np.stack([env.qpos_goal[:, qa:qa + 7].cpu().numpy() for qa in env.obj_q], 1)
        assert np.array_equal(qg[..., :3], g["qpos_goal_obj"][c_of][..., :3].astype(np.float32))
        worst["qpos_goal"] = max(worst["qpos_goal"], np.abs(qg[..., 3:] - g["qpos_goal_obj"][c_of][..., 3:]).max())
        if h == 0:
            worst["bbox"] = max(worst["bbox"], np.abs(obs["obj_bbox_size"].cpu().numpy() - g["bbox"][c_of]).max())
        for t0 in range(0, T, B // 2):
            t_of = t0 + np.arange(B) // 2
            pose = np.concatenate([g["cur_pos"][c_of, t_of], g["cur_quat"][c_of, t_of]], -1).astype(np.float32)
            for i, qa in enumerate(env.obj_q):
                env.sim.qpos[:, qa:qa + 7] = torch.tensor(pose[:, i], device=env.device)
            env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
            for mode in ("full", "mod90", "mod180"):
                env.post.rot_dist_type = blocks.ROT_DIST_TYPES[mode]      # (the tables of parallel quaternions are the env's: it was built with mod90)
                env._observe_only()
                env._reobserve(np.zeros(0, dtype=np.int64), np.arange(B))      # (under "a new goal": is_goal_achieved)
                env.sync()
                o = env.observe()
                want = {k: g["%s_%s" % (mode, k)][c_of, t_of] for k in ("rel_pos", "rel_rot", "dist_pos", "dist_rot", "rel_dist", "success")}
                rp, rr = o["rel_goal_obj_pos"].cpu().numpy().astype(np.float64), o["rel_goal_obj_rot"].cpu().numpy().astype(np.float64)
                rd, gd = env.rel_dist.cpu().numpy().astype(np.float64), env.goal_dist.cpu().numpy().astype(np.float64)
                lock = np.abs(np.abs(want["rel_rot"][..., 1]) - np.pi / 2) < 0.05
                e_eul = np.abs(np.mod(rr - want["rel_rot"] + np.pi, 2 * np.pi) - np.pi).max(-1)
                d_rot = _angle_between(rr, np.zeros_like(rr))
                worst["rel_pos"] = max(worst["rel_pos"], np.abs(rp - want["rel_pos"]).max())
                worst["rel_rot"] = max(worst["rel_rot"], _angle_between(rr, want["rel_rot"]).max())
                worst["rel_euler"] = max(worst["rel_euler"], e_eul[~lock].max() if (~lock).any() else 0.0)
                worst["dist"] = max(worst["dist"], np.abs(gd[:, 0] - want["dist_pos"].sum(-1)).max(), np.abs(gd[:, 1] - want["dist_rot"].sum(-1)).max(),
                                    np.abs(d_rot - want["dist_rot"]).max(), np.abs(np.linalg.norm(rp, axis=-1) - want["dist_pos"]).max())
                worst["rel_dist"] = max(worst["rel_dist"], np.abs(rd - want["rel_dist"]).max())
                # per object from the kernel's own per-object numbers; the kernel's count and flag from its own bits
                bits = (np.linalg.norm(rp, axis=-1) < thr["obj_pos"]) & (d_rot < thr["obj_rot"]) & (rd < thr["rel_dist"])
                assert np.array_equal(bits, want["success"].astype(bool)), (mode, t0)
                assert np.array_equal(env.prev_nsucc.cpu().numpy(), want["success"].sum(-1).astype(np.float32)), (mode, t0, env.prev_nsucc, want["success"])
                assert np.array_equal(o["is_goal_achieved"][:, 0].cpu().numpy().astype(bool), want["success"].astype(bool).all(-1)), (mode, t0)
                seen |= set(want["success"].astype(bool).all(-1).tolist())
    print("recorded goals vs the reference's code:", ", ".join("%s %.1e" % kv for kv in worst.items()))
    assert seen == {True, False}
    assert worst["rel_pos"] < 2e-6 and max(worst.values()) < ROT_TOL, worst


def test_recorded_goals_match_reference_code_emul(emul_lib):
    _golden_layer(EMUL, emul_lib)


@pytest.mark.gpu
def test_recorded_goals_match_reference_code_gpu():
    _golden_layer(GPU, None)


# ------------------------------------------------------------------------------------------------ 2. rel_dist
def _rel_dist(tier, lib):
    """A rigid shift of all objects gives 0 (the reference's test_relative_distance); one non-anchor object moved by d gives d for it and 0 for the rest.  Against
    float64 numpy on the float32 positions the kernel read: 2e-6, eight float32 ulps at 2 m.  With groups of duplicates there is no rel_dist."""
    B, N = 4, 4
    goal = _shifted(STACKED4, (-0.35, 0.2, 0.0))
    env = BatchedBlockRearrangeEnv(B, num_objects=N, initial_states=STACKED4, goal_states=[goal], success_threshold={"obj_pos": 0.04, "obj_rot": 0.2, "rel_dist": 0.03},
                                   **_kw(tier, lib, **NO_RECIPE))
    env.reset()
    gpos = env.goal[:, :, :3].cpu().numpy().astype(np.float64)
    anchor = int(np.argmin(gpos[0, :, 2]))
    assert anchor == 3 and env.post.rel_threshold == pytest.approx(0.03) and "rel_dist" in env.info()["goal_dist"]
    shifts = np.array([[0.0, 0.0, 0.0], [0.11, -0.07, 0.0], [-0.3, 0.25, 0.0], [0.05, 0.05, 0.0]])
    moved, d = [0, 1, 2, 0], np.array([[0.0, 0.0, 0.0], [0.02, 0.0, 0.0], [0.0, -0.05, 0.0], [0.03, 0.04, 0.0]])
    for with_move in (False, True):
        pos = gpos + shifts[:, None, :]
        if with_move:
            pos[np.arange(B), moved] += d
        for i, qa in enumerate(env.obj_q):
            env.sim.qpos[:, qa:qa + 3] = torch.tensor(pos[:, i].astype(np.float32), device=env.device)
        env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
        env._observe_only()
        env.sync()
        p = env.observe()["obj_pos"].cpu().numpy().astype(np.float64)
        want = np.linalg.norm(p - (gpos - gpos[:, anchor:anchor + 1] + p[:, anchor:anchor + 1]), axis=-1)
        got = env.rel_dist.cpu().numpy().astype(np.float64)
        assert np.abs(got - want).max() < 2e-6, (got, want)
        expect = np.zeros((B, N))
        if with_move:
            expect[np.arange(B), moved] = np.linalg.norm(d, axis=-1)
        assert np.abs(got - expect).max() < 2e-6, (got, expect)
    # duplicates: the reference computes rel_dist for distinct objects only
    dup = BatchedBlockRearrangeEnv(B, num_objects=N, initial_states=STACKED4, goal_states=[goal], object_groups="single", **_kw(tier, lib, **NO_RECIPE))
    dup.reset()
    assert dup.rel_dist is None and not dup.post.rel_dist and "goal_dist" not in dup.info()


def test_rel_dist_emul(emul_lib):
    _rel_dist(EMUL, emul_lib)


@pytest.mark.gpu
def test_rel_dist_gpu():
    _rel_dist(GPU, None)


# ------------------------------------------------------------------------------------------------ 3. episode start
def _episode_start(tier, lib, on_device):
    g = _golden()
    B, N = 4, 2
    states = [{"obj_pos": g["goal_state_pos"][c], "obj_quat": g["goal_state_quat"][c]} for c in (2, 3)]
    env = BatchedBlockRearrangeEnv(B, num_objects=N, initial_states=states, device_reset=on_device, **_kw(tier, lib, **NO_RECIPE))
    table = np.stack([_f32_state(s, N) for s in states])
    arm = blocks.TABLETOP_EXPERIMENT_INITIAL_POS.astype(np.float32)

    def check(scene):
        env.sync()
        assert env.scene.tolist() == list(scene)
        assert np.array_equal(_objects(env), table[list(scene)])                                   # the recorded state as cast to float32, exactly
        assert np.array_equal(env.sim.qpos[:, env.arm_q].cpu().numpy(), np.tile(arm, (B, 1)))       # the arm at its start pose
        assert not bool(env.sim.qvel.any())
        bbox = env.observe()["obj_bbox_size"].cpu().numpy()
        assert np.abs(bbox - g["bbox"][2:][list(scene)]).max() < ROT_TOL

    env.reset(on_device=on_device)
    check([0, 1, 0, 1])                                 # two scenes in one batch, on the envs scene_next named
    env.set_scene_next([1, 1, 0, 0])
    env.step(_zero_action(env))
    env.sync()
    assert env.scene.tolist() == [0, 1, 0, 1] and env.scene_next.tolist() == [1, 1, 0, 0]      # not before the next episode start
    mask = torch.tensor([True, False, True, True], device=env.device)
    env.reset(mask, on_device=on_device)
    env.sync()
    assert env.scene.tolist() == [1, 1, 0, 0]
    rows = [0, 2, 3]
    assert np.array_equal(_objects(env)[rows], table[[1, 0, 0]])
    env.reset(on_device=on_device)
    check([1, 1, 0, 0])


@pytest.mark.parametrize("on_device", [False, True])
def test_episode_starts_from_the_recorded_state_emul(emul_lib, on_device):
    _episode_start(EMUL, emul_lib, on_device)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_episode_starts_from_the_recorded_state_gpu(on_device):
    _episode_start(GPU, None, on_device)


# ------------------------------------------------------------------------------------------------ 4. the goal cursor
def _cursor(tier, lib, advance, route):
    """Scene 0 has three goals, scene 1 two.  advance_goals False: every goal is state 0 across three re-goals (what the reference's code does).  True: 0, 1, 2, 0
    (scene 1: 0, 1, 0, 1) and 0 again after an episode end.  `route`: reset_goals() / reset() on the host or the device, or the pipelined recipe's own step."""
    B, N = 4, 2
    pipelined, on_device = route.startswith("pipe"), route.endswith("device")
    base = SAMPLE_GOAL
    goals = [[_shifted(base, (0.01 * k, 0.0, 0.0)) for k in range(3)], [_shifted(base, (0.0, -0.01 * (k + 1), 0.0)) for k in range(2)]]
    env = BatchedBlockRearrangeEnv(B, num_objects=N, initial_states=[base, _shifted(base, (0.05, 0.0, 0.0))], goal_states=goals, advance_goals=advance,
                                   pipelined_reset=pipelined, device_reset=on_device, **_kw(tier, lib, **NO_RECIPE))
    tables = [np.stack([_f32_state(s, N) for s in gs]) for gs in goals]

    def which():
        env.sync()
        goal = env.goal.cpu().numpy()
        out = []
        for e in range(B):
            hit = [k for k, row in enumerate(tables[e % 2]) if np.array_equal(goal[e], row)]
            assert len(hit) == 1, (e, goal[e])
            out.append(hit[0])
        return out

    def advance_recipe():
        env._advance_recipes_device() if on_device else env._advance_recipes()

    def regoal():
        env.goal_reset.fill_(True); env.done.fill_(False)
        if pipelined:
            advance_recipe()
        else:
            env.reset_goals(on_device=on_device)
        return which()

    def new_episode():
        if not pipelined:
            env.reset(on_device=on_device)
            return which()
        env.goal_reset.fill_(False); env.done.fill_(True)
        advance_recipe()
        env.done.fill_(False)
        for _ in range(3):
            advance_recipe()
            env.sync()
            if bool(env.episode_started.all()):
                return which()
        raise AssertionError("the episodes did not start")

    env.reset(on_device=False if pipelined else on_device)
    seq = [which()] + [regoal() for _ in range(3)]
    want = [[0, 0, 0, 0], [1, 1, 1, 1], [2, 0, 2, 0], [0, 1, 0, 1]] if advance else [[0] * B] * 4
    assert seq == want, seq
    assert new_episode() == [0] * B
    assert regoal() == ([1] * B if advance else [0] * B)
    assert env.goal_cursor.tolist() == ([2, 0, 2, 0] if advance else [0] * B)


@pytest.mark.parametrize("route", ["sync_host", "sync_device", "pipe_host", "pipe_device"])
@pytest.mark.parametrize("advance", [False, True])
def test_goal_cursor_emul(emul_lib, advance, route):
    _cursor(EMUL, emul_lib, advance, route)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["sync_host", "sync_device", "pipe_host", "pipe_device"])
@pytest.mark.parametrize("advance", [False, True])
def test_goal_cursor_gpu(advance, route):
    _cursor(GPU, None, advance, route)


# ------------------------------------------------------------------------------------------------ 5. host recipe against device recipe
TWIN_ROWS = ("qpos", "qvel", "ctrl", "pid", "warmstart", "time", "status", "goal", "goal_rot", "qpos_goal", "static_obs", "t", "steps", "ssl", "successes", "consecutive",
             "prev_valid", "prev_nsucc", "packed", "reward", "done", "goal_reset", "goal_dist", "rel_dist", "info_ssl", "trial_success", "hold", "hold_ctrl", "frozen",
             "solver_active", "nticks", "scripted", "resetting", "episode_started", "scene", "goal_cursor", "params", "solver_qpos", "solver_qvel", "solver_ctrl", "solver_pid",
             "solver_warmstart", "solver_time", "solver_mocap", "solver_eq_data")


def _rows(env):
    s = dict(qpos=env.sim.qpos, qvel=env.sim.qvel, ctrl=env.sim.ctrl, pid=env.sim.pid, warmstart=env.sim.qacc_warmstart, time=env.sim.time, status=env.sim.status,
             goal=env.goal, goal_rot=env.goal_rot, qpos_goal=env.qpos_goal, static_obs=env.static_obs, t=env.t, steps=env.steps, ssl=env.ssl, successes=env.successes,
             consecutive=env.consecutive, prev_valid=env.prev_valid, prev_nsucc=env.prev_nsucc, packed=env.packed, reward=env.reward, done=env.done, goal_reset=env.goal_reset,
             goal_dist=env.goal_dist, rel_dist=env.rel_dist, info_ssl=env.info_ssl, trial_success=env.trial_success, hold=env.hold, hold_ctrl=env.hold_ctrl, frozen=env.frozen,
             solver_active=env.solver_active, nticks=env.nticks, scripted=env.scripted, resetting=env.resetting, episode_started=env.episode_started, scene=env.scene,
             goal_cursor=env.goal_cursor, params=env.sim.params.block)
    v = env.solver_sim
    s.update(solver_qpos=v.qpos, solver_qvel=v.qvel, solver_ctrl=v.ctrl, solver_pid=v.pid, solver_warmstart=v.qacc_warmstart, solver_time=v.time, solver_mocap=v.mocap,
             solver_eq_data=v.eq_data)
    assert set(s) == set(TWIN_ROWS)
    return {k: v.clone() for k, v in s.items()}


def _twin(tier, lib):
    """Host recipe against device recipe (pipelined resets) on a recorded scene, two scenes in the batch, six steps of the zero action.  Thresholds no state can miss
    force a re-goal at every step and, with successes_needed = 3, an episode end at the third; the recipe (two steps of stabilisation, no random action) restarts the
    episode at the fifth.  A recorded scene involves no draw: every env row is equal bit for bit."""
    B, N = 4, 4
    scenes = [STACKED4, _shifted(STACKED4, (-0.3, 0.2, 0.0), tilt=(np.cos(0.2), np.sin(0.2), 0.0, 0.0))]
    goals = [[_shifted(STACKED4, (-0.2, 0.1, 0.0)), STACKED4], [_shifted(STACKED4, (-0.1, 0.3, 0.0))]]
    kw = dict(num_objects=N, initial_states=scenes, goal_states=goals, advance_goals=True, pipelined_reset=True, successes_needed=3, starting_seed=3,
              success_threshold={"obj_pos": 10.0, "obj_rot": 10.0, "rel_dist": 10.0})
    H = BatchedBlockRearrangeEnv(B, device_reset=False, **_kw(tier, lib, n_random_initial_steps=0, **kw))
    D = BatchedBlockRearrangeEnv(B, device_reset=True, **_kw(tier, lib, n_random_initial_steps=0, **kw))
    H.reset(); D.reset()
    seen = dict(regoal=0, ended=0, started=0)
    for k in range(7):
        if k:
            oh, rh, dh, ih = H.step(_zero_action(H))
            od, rd, dd, idv = D.step(_zero_action(D))
            seen["regoal"] += int((ih["goal_reset"] & ~dh).sum()); seen["ended"] += int(dh.sum()); seen["started"] += int(ih["episode_started"].sum())
        H.sync(); D.sync()
        h, d = _rows(H), _rows(D)
        bad = ["%s (max |diff| %.3e)" % (q, float((h[q].double() - d[q].double()).abs().max())) for q in TWIN_ROWS if not torch.equal(h[q], d[q])]
        assert not bad, "after %s: host and device recipes differ in %s" % ("reset()" if k == 0 else "step %d" % k, ", ".join(bad))
    assert seen["regoal"] >= 2 * B and seen["ended"] == B and seen["started"] == B, seen
    assert int(H.sim.status.max()) == 0 and bool(torch.isfinite(H.packed).all())


def test_host_and_device_recipes_agree_bit_for_bit_emul(emul_lib):
    _twin(EMUL, emul_lib)


@pytest.mark.gpu
def test_host_and_device_recipes_agree_bit_for_bit_gpu():
    _twin(GPU, None)


# ------------------------------------------------------------------------------------------------ 6. the default path
def _unchanged_default(tier, lib):
    """An env built without tables has NULL table pointers and no rel_dist, and its packed rows over five steps are those of a BatchedBlockRearrangeEnv built the old
    way -- through the holdout surface with the blocks env's own goal orientation, pipelined device resets with an episode end inside the five steps."""
    B = 4
    kw = _kw(tier, lib, pipelined_reset=True, device_reset=True, max_timesteps_per_goal_per_obj=1, starting_seed=7)
    new = holdout.make_simple_env(B, parameters=dict(simulation_params=dict(num_objects=2), n_random_initial_steps=1),
                                  constants=dict(goal_args=dict(randomize_goal_rot=False), max_timesteps_per_goal_per_obj=1),
                                  **{k: v for k, v in kw.items() if k not in ("max_timesteps_per_goal_per_obj", "n_random_initial_steps")})
    old = BatchedBlockRearrangeEnv(B, num_objects=2, **kw)
    r, p = new.recipe, new.post
    assert not any((r.scene_init, r.scene_init_half, r.scene_goal, r.scene_goal_rot, r.scene_num_goals, r.scene_next, r.scene, r.goal_cursor, r.num_scenes, r.max_scene_goals,
                    r.advance_goals, p.rel_dist)) and p.rel_threshold == 0.0
    assert new.rel_dist is None and new.scene is None and new.scene_next is None and new.num_scenes == 0 and "goal_dist" not in new.info()
    new.reset(); old.reset()
    assert torch.equal(new.packed, old.packed)
    ended = 0
    for k in range(5):
        new.step(_zero_action(new)); old.step(_zero_action(old))
        new.sync(); old.sync()
        assert torch.equal(new.packed, old.packed) and torch.equal(new.sim.qpos, old.sim.qpos) and torch.equal(new.goal, old.goal), k
        ended += int(new.done.sum())
    assert ended >= B


def test_default_path_is_unchanged_emul(emul_lib):
    _unchanged_default(EMUL, emul_lib)


@pytest.mark.gpu
def test_default_path_is_unchanged_gpu():
    _unchanged_default(GPU, None)


# ------------------------------------------------------------------------------------------------ 7. a sampled goal after a recorded start
def _sampled_goal(tier, lib, on_device):
    """No goal states: the goals are sampled.  The reference's holdout reset sets the objects, not the targets, so the first goal starts from the target's model
    orientation: its yaw is the draw alone, whatever the recorded objects' orientation.  Host route: the draws replayed from the seed.  Device route: the goal rows
    of a twin env whose recorded start has the same positions and identity orientations are the same bits.  Every goal lies flat inside the placement area."""
    B, N, seed = 4, 2, 5
    st = blocks.load_state(SAMPLE_GOAL, N)
    flat = {"obj_pos": st[:, :3], "obj_quat": np.tile([1.0, 0.0, 0.0, 0.0], (N, 1))}
    assert np.abs(st[:, 4:6]).max() > 0.1 and np.abs(2 * np.arctan2(st[1, 6], st[1, 3])) > 0.5      # (a tilted block and a yawed one)
    make = lambda s, rnd: BatchedBlockRearrangeEnv(B, num_objects=N, initial_states=s, randomize_goal_rot=rnd, device_reset=on_device, starting_seed=seed, **_kw(tier, lib, **NO_RECIPE))
    for rnd in (False, True):
        env = make(SAMPLE_GOAL, rnd)
        env.reset(on_device=on_device)
        env.sync()
        rot, goal = env.goal_rot.cpu().numpy().astype(np.float64), env.goal.cpu().numpy().astype(np.float64)
        assert not rot[..., :2].any() and not goal[..., 4:6].any()
        if not rnd:
            assert not rot.any()                                              # base 0 and no draw: yaw 0 exactly
        elif not on_device:
            rs = np.random.RandomState(seed)
            want = np.stack([rs.uniform(0.0, 2.0 * np.pi, N) for _ in range(B)])
            assert np.abs(np.mod(rot[..., 2] - want + np.pi, 2 * np.pi) - np.pi).max() < 1e-6
        else:
            twin = make(flat, rnd)
            twin.reset(on_device=on_device)
            twin.sync()
            assert torch.equal(env.goal, twin.goal) and torch.equal(env.goal_rot, twin.goal_rot) and len(np.unique(rot[..., 2])) == B * N
        lo, hi = env.placement_area_boundary()
        half = blocks.yawed_half(env.obj_half, rot[..., 2])
        assert (goal[..., :2] - half[..., :2] >= lo[:2] - 1e-6).all() and (goal[..., :2] + half[..., :2] <= hi[:2] + 1e-6).all()
        assert np.abs(goal[..., 2] - (env.table_height + env.obj_half[:, 2] - env.obj_center[:, 2])).max() < 1e-6


@pytest.mark.parametrize("on_device", [False, True])
def test_sampled_goal_after_a_recorded_start_emul(emul_lib, on_device):
    _sampled_goal(EMUL, emul_lib, on_device)


@pytest.mark.gpu
@pytest.mark.parametrize("on_device", [False, True])
def test_sampled_goal_after_a_recorded_start_gpu(on_device):
    _sampled_goal(GPU, None, on_device)


# ------------------------------------------------------------------------------------------------ 8. refusals and the surface
def test_refusals_name_their_key(emul_lib):
    kw = _kw(EMUL, emul_lib, **NO_RECIPE)
    sp = lambda **k: dict(simulation_params=dict(num_objects=2, **k))
    const = dict(initial_state_path=SAMPLE_GOAL)
    for key in ("task_object_configs", "scene_object_configs", "material_names", "mesh_names"):
        with pytest.raises(NotImplementedError, match=key):
            holdout.make_simple_env(4, parameters=sp(**{key: []}), constants=const, **kw)
    with pytest.raises(NotImplementedError, match="shared_settings"):
        holdout.make_simple_env(4, parameters=sp(), constants=dict(const, shared_settings={}), **kw)
    with pytest.raises(NotImplementedError, match="max_num_objects"):
        holdout.make_simple_env(4, parameters=sp(max_num_objects=5), constants=const, **kw)
    with pytest.raises(NotImplementedError, match="max_num_objects"):
        BatchedBlockRearrangeEnv(4, num_objects=2, max_num_objects=5, initial_states=SAMPLE_GOAL, **kw)
    with pytest.raises(NotImplementedError, match="num_objects"):
        holdout.make_simple_env(4, parameters=dict(simulation_params=dict(num_objects=9)), constants=const, **kw)
    from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv
    with pytest.raises(NotImplementedError, match="ycb"):
        BatchedYcbRearrangeEnv(4, initial_states=SAMPLE_GOAL, **kw)
    with pytest.raises(NotImplementedError, match="ycb"):
        holdout.make_simple_env(4, parameters=sp(), constants=const, model=object(), **kw)
    with pytest.raises(NotImplementedError, match="goal_state_file"):
        holdout.make_simple_env(4, parameters=sp(), constants=dict(const, goal_args=dict(goal_state_file="x")), **kw)
    with pytest.raises(ValueError, match="rel_dist"):
        holdout.make_simple_env(4, parameters=sp(object_groups=[2]), constants=dict(const, success_threshold={"obj_pos": 0.04, "obj_rot": 0.2, "rel_dist": 0.02}), **kw)
    with pytest.raises(ValueError, match=r"initial_states\[0\] has 3 rows, fewer than num_objects=4"):
        holdout.make_simple_env(4, parameters=dict(simulation_params=dict(num_objects=4)), constants=const, **kw)
    with pytest.raises(ValueError, match=r"goal_states\[0\]\[1\] has 3 rows"):
        holdout.make_simple_env(4, parameters=dict(simulation_params=dict(num_objects=4)), constants=dict(goal_args=dict(goal_state_paths=[STACKED4, SAMPLE_GOAL])), **kw)
    env = holdout.make_simple_env(4, parameters=sp(), constants=dict(initial_state=[SAMPLE_GOAL, STACKED4]), device_reset=True, **kw)
    for bad in (2, -1, [0, 1, 2, 0]):
        with pytest.raises(ValueError, match="scene"):
            env.set_scene_next(bad)
    with pytest.raises(ValueError, match="scene_next"):
        BatchedBlockRearrangeEnv(4, num_objects=2, **kw).set_scene_next(0)
    # the C ABI checks the table pointers and counts, with a message as the other kinds have
    r = env.recipe
    for field, value, text in (("num_scenes", 0, "num_scenes"), ("scene_init_half", None, "scene_init_half"), ("scene_next", None, "scene_next"), ("goal_kind", 1, "goal_kind 0"),
                               ("advance_goals", 1, "advance_goals")):
        keep = getattr(r, field)
        setattr(r, field, value)
        with pytest.raises(_native.NativeError, match=text):
            env._recipe_launch()
        setattr(r, field, keep)
    g = holdout.make_simple_env(4, parameters=sp(), constants=dict(goal_args=dict(goal_state_paths=[SAMPLE_GOAL])), device_reset=True, **kw)
    for field, value, text in (("scene_goal_rot", None, "scene_goal_rot"), ("goal_cursor", None, "goal_cursor"), ("max_scene_goals", 0, "max_scene_goals")):
        keep = getattr(g.recipe, field)
        setattr(g.recipe, field, value)
        with pytest.raises(_native.NativeError, match=text):
            g._recipe_launch()
        setattr(g.recipe, field, keep)
    p = g.post
    p.rel_threshold, keep = 0.5, p.rel_dist
    p.rel_dist = None
    with pytest.raises(_native.NativeError, match="rel_threshold needs rel_dist"):
        g._post()
    p.rel_dist, p.rel_threshold = keep, 0.0


def test_surface_defaults_and_record_state_round_trip(emul_lib):
    kw = _kw(EMUL, emul_lib, **NO_RECIPE)
    sp = dict(simulation_params=dict(num_objects=2), n_random_initial_steps=0)
    env = holdout.make_env(4, parameters=sp, device_reset=True, **kw)      # HoldoutGoalArgs.randomize_goal_rot = True; the default threshold has no rel_dist; the wrapper stack as in the reference
    assert env.randomize_goal_rot is True and env.recipe.randomize_goal_rot == 1 and env.wrapped and env.rel_dist is None and env.post.rel_threshold == 0.0
    simple = holdout.make_simple_env(4, parameters=sp, constants=dict(goal_args=dict(randomize_goal_rot=False)), starting_seed=2, **kw)
    assert simple.randomize_goal_rot is False and not simple.wrapped
    simple.reset()
    state = simple.record_state(1)                        # the reference's create_holdout use: the live objects as a state
    assert state["obj_pos"].shape == (2, 3) and state["obj_quat"].shape == (2, 4) and simple.record_state()["obj_pos"].shape == (4, 2, 3)
    path = os.path.join(_tmp(), "state.npz")
    np.savez(path, **state)
    assert np.array_equal(blocks.load_state(path, 2), blocks.load_state(state, 2))
    again = holdout.make_simple_env(4, parameters=sp, constants=dict(initial_state_path=path, goal_args=dict(goal_state_paths=[path])), device_reset=True, **kw)
    assert again.advance_goals is False and again.recipe.advance_goals == 0 and again.rel_dist is not None and again.post.rel_threshold == 0.0      # rel_dist reported, not part of success
    again.reset()
    back = again.record_state()
    assert np.array_equal(back["obj_pos"], np.tile(state["obj_pos"], (4, 1, 1))) and np.abs(back["obj_quat"] - state["obj_quat"]).max() < 2e-7
    view = blocks.SingleEnvView(holdout.make_simple_env(1, parameters=sp, constants=dict(initial_state=state, goal_args=dict(goal_states=[state])), **kw))
    view.reset()
    info = view.step(np.zeros(6))[3]                      # the reference's types: goal_dist is a dict of per-object arrays
    assert info["goal_dist"]["rel_dist"].shape == (2,) and float(info["goal_dist"]["rel_dist"].max()) < 1e-3


def _tmp():
    if "tmp" not in _cache:
        import tempfile
        _cache["tmp"] = tempfile.mkdtemp(prefix="rearrange_holdout_")
    return _cache["tmp"]


# ------------------------------------------------------------------------------------------------ 9. physics: the tower of block_stacking4
#: the reference's test_stacking caps (envs/rearrange/holdouts/tests/test_stability.py:215-221), which the CPU oracle keeps on this scene (profiles/rearrange_holdout.txt)
MAX_SPEED, MAX_ANGULAR_SPEED = 0.3, 3.0


@pytest.mark.gpu
def test_stacked_tower_stays_standing_gpu():
    """The four stacked blocks of the reference's block_stacking4, no stabilisation, no random steps, the full 40 substeps, 50 steps of the zero action: the tower stays
    standing (z order kept, each block within half a block width of its start in x and y) and the objects' speeds after every step stay below the reference's
    test_stacking caps, 0.3 m/s and 3.0 rad/s (measured as that test measures them: the norms of the free joint's qvel[:3] and qvel[3:])."""
    B, N = 4, 4
    env = BatchedBlockRearrangeEnv(B, device="cuda:0", num_objects=N, initial_states=STACKED4, n_substeps=40, **NO_RECIPE)
    env.reset()
    start = _objects(env)[..., :3].astype(np.float64)
    vmax = wmax = 0.0
    dofs = torch.tensor(env.obj_v, device=env.device)
    for k in range(50):
        env.step(_zero_action(env))
        v = torch.stack([env.sim.qvel[:, d:d + 3].norm(dim=1) for d in env.obj_v], 1); w = torch.stack([env.sim.qvel[:, d + 3:d + 6].norm(dim=1) for d in env.obj_v], 1)
        vmax, wmax = max(vmax, float(v.max())), max(wmax, float(w.max()))
    env.sync()
    end = _objects(env)[..., :3].astype(np.float64)
    print("stacked tower on the GPU: max speed %.4f m/s, max angular speed %.4f rad/s, max |dx, dy| %.4f m" % (vmax, wmax, np.abs(end[..., :2] - start[..., :2]).max()))
    assert int(env.sim.status.max()) == 0 and not bool(env.done.any())
    assert np.array_equal(np.argsort(end[..., 2], -1), np.argsort(start[..., 2], -1))
    assert np.abs(end[..., :2] - start[..., :2]).max() < 0.0254
    assert vmax <= MAX_SPEED and wmax <= MAX_ANGULAR_SPEED
