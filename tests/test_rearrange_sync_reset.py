"""The synchronous episode API of the rearrange envs on the device: `reset(mask, on_device=...)` and `reset_goals(on_device=...)` of BatchedBlockRearrangeEnv
(robogym_amd/envs/rearrange/blocks.py `_reset_device`), ra_recipe_kernel's `active` row and `sync_mode` (forced end, regoal only; include/rgstep.h) and
ra_param_rows_kernel (include/rgstep_sync_reset.h).  The reference of every check is the pipelined device recipe itself -- the same kernel with the same draw
streams -- or a clone of the tensors taken before the call, compared bit for bit.

Two tiers with the same protocols: the kernel source on the emulation harness (B = 4, n_substeps = 1) and the gfx950 library through the C ABI (B = 64,
n_substeps = 2).  Recipe stages of 2 + 1 + 2 steps.  Masks always include env 0 and env B - 1."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv

FAST = dict(stabilize_steps=2, n_random_initial_steps=1, settle_steps=2)
EMUL = dict(device="cpu", B=4, n_substeps=1)
GPU = dict(device="cuda:0", B=64, n_substeps=2)


def _make(tier, lib, cls=BatchedBlockRearrangeEnv, **kw):
    args = dict(device=tier["device"], n_substeps=tier["n_substeps"], **FAST)
    if lib is not None:
        args["lib"] = lib
    args.update(kw)
    return cls(tier["B"], **args)


def _state(env):
    """Clones of everything a reset may touch: both worlds, goal rows, tracker counters, the recipe's rows, the parameter block, the packed observation row and the
    outputs of the last step"""
    s = dict(qpos=env.sim.qpos, qvel=env.sim.qvel, ctrl=env.sim.ctrl, pid=env.sim.pid, warmstart=env.sim.qacc_warmstart, time=env.sim.time, status=env.sim.status,
             goal=env.goal, goal_rot=env.goal_rot, qpos_goal=env.qpos_goal, static_obs=env.static_obs, t=env.t, steps=env.steps, ssl=env.ssl, successes=env.successes,
             consecutive=env.consecutive, prev_valid=env.prev_valid, prev_nsucc=env.prev_nsucc, packed=env.packed, reward=env.reward, done=env.done, goal_reset=env.goal_reset,
             goal_dist=env.goal_dist, info_ssl=env.info_ssl, trial_success=env.trial_success, hold=env.hold, hold_ctrl=env.hold_ctrl, frozen=env.frozen,
             solver_active=env.solver_active, nticks=env.nticks, scripted=env.scripted, resetting=env.resetting, episode_started=env.episode_started,
             ema_value=env.ema_value, ema_t=env.ema_t, action_ema=env.action_ema)
    if env.device_reset:
        s.update(yaw=env.yaw, stage=env.stage, left=env.left, placement_failed=env.placement_failed)
    if env.per_env_parameters:
        s["params"] = env.sim.params.block
    if env.obj_group is not None:
        s["obj_group"] = env.obj_group
    if env.num_active is not None:
        s["num_active"] = env.num_active
    if env.solver_sim is not None:
        v = env.solver_sim
        s.update(solver_qpos=v.qpos, solver_qvel=v.qvel, solver_ctrl=v.ctrl, solver_pid=v.pid, solver_warmstart=v.qacc_warmstart, solver_time=v.time, solver_mocap=v.mocap,
                 solver_eq_data=v.eq_data)
    return {k: v.clone() for k, v in s.items()}


# rows of the recipe that a pipelined env writes on every step and a synchronous one only inside reset(): equal after a reset, not compared between the two while stepping
TWIN_KEYS = ("qpos", "qvel", "ctrl", "pid", "warmstart", "time", "status", "goal", "goal_rot", "qpos_goal", "static_obs", "yaw", "t", "steps", "ssl", "successes", "consecutive",
             "prev_valid", "prev_nsucc", "packed", "placement_failed", "params", "solver_qpos", "solver_qvel", "solver_ctrl", "solver_pid", "solver_warmstart", "solver_time",
             "solver_mocap", "solver_eq_data", "reward", "done", "goal_reset", "goal_dist", "info_ssl", "hold", "hold_ctrl", "frozen", "solver_active", "nticks", "scripted",
             "resetting", "stage", "left", "ema_value", "ema_t", "action_ema", "obj_group", "num_active")


def _assert_rows_equal(a, b, rows=None, keys=None, what=""):
    bad = []
    for k in (keys if keys is not None else a.keys()):
        if k not in a or k not in b:
            continue
        x, y = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        if not torch.equal(x, y):
            bad.append("%s (max |diff| %.3e)" % (k, float((x.double() - y.double()).abs().max())))
    assert not bad, "%s: not bit-identical: %s" % (what, ", ".join(bad))


def _zero_action(env):
    if env.wrapped:
        return torch.full((env.B, env.action_dim), env.n_action_bins // 2, dtype=torch.int64, device=env.device)
    return torch.zeros((env.B, env.action_dim), dtype=torch.float32, device=env.device)


def _mask(env, rows):
    m = torch.zeros(env.B, dtype=torch.bool, device=env.device)
    m[torch.as_tensor(rows, device=env.device)] = True
    return m


def _sync(env):
    env.sync()
    assert int(env.sim.status.max()) == 0 and (env.solver_sim is None or int(env.solver_sim.status.max()) == 0), "status words"
    assert bool(torch.isfinite(env.packed).all()) and bool(torch.isfinite(env.sim.qpos).all())


def _step_both_equal(P, S, k):
    op, rp, dp, _ = P.step(_zero_action(P))
    os_, rs, ds, _ = S.step(_zero_action(S))
    assert torch.equal(rp, rs) and torch.equal(dp, ds) and all(torch.equal(op[q], os_[q]) for q in op), "step %d: the synchronous env's outputs differ from the pipelined env's" % k
    return dp


# ------------------------------------------------------------------------------------------------ 1. twin of the pipelined device recipe
def _twin_of_pipelined(tier, lib, **extra):
    """P: pipelined device recipe.  S: the same env without pipelined_reset.  Equal host resets, five equal steps into the time-out, then P's recipe inside its next
    five steps against S.reset(mask=done) with the recipe launch counter P's step 5 carried: every env bit-identical.  Then the new episodes, equal again for five
    steps into the next time-out, and a reset of {0, middle, B - 1}: those rows as P's, every other row of S as it was."""
    kw = dict(device_reset=True, max_timesteps_per_goal_per_obj=1, starting_seed=11, **extra)
    P, S = _make(tier, lib, pipelined_reset=True, **kw), _make(tier, lib, pipelined_reset=False, **kw)
    B = P.B
    P.reset(on_device=False); S.reset(on_device=False)
    _assert_rows_equal(_state(P), _state(S), what="after the host resets")
    for rnd, rows in ((0, None), (1, [0, B // 2, B - 1])):
        for k in range(1, 6):
            done = _step_both_equal(P, S, 10 * rnd + k)
        assert bool(done.all()) and bool(S.done.all())
        counter = int(P.recipe.step)                      # what P's launch of the time-out step carried
        for k in range(5):
            info = P.step(_zero_action(P))[3]
        assert bool(info["episode_started"].all()) and not bool(info["resetting"].any())
        S.recipe.step = counter - 1
        before = _state(S)
        mask = S.done.clone() if rows is None else _mask(S, rows)
        obs = S.reset(mask=mask)
        _sync(P); _sync(S)
        p, s = _state(P), _state(S)
        assert int(p["placement_failed"].max()) == 0 and int(s["placement_failed"].max()) == 0
        _assert_rows_equal(p, s, rows=rows, keys=TWIN_KEYS, what="after reset(mask) of %s" % ("every env" if rows is None else rows))
        sel = slice(None) if rows is None else rows
        assert all(torch.equal(obs[q][sel], P.observe()[q][sel]) for q in obs)
        if rows is not None:
            others = [e for e in range(B) if e not in rows]
            _assert_rows_equal(before, s, rows=others, what="rows outside the mask")
            assert bool(S.done[others].all()) and not bool(S.done[rows].any())      # finished envs stay done until they are reset


def test_sync_reset_is_the_pipelined_recipe_emul(emul_lib):
    _twin_of_pipelined(EMUL, emul_lib)


@pytest.mark.gpu
def test_sync_reset_is_the_pipelined_recipe_gpu():
    _twin_of_pipelined(GPU, None)


@pytest.mark.gpu
@pytest.mark.parametrize("control_mode", ["joint", "tcp+wrist"])
def test_sync_reset_is_the_pipelined_recipe_control_modes_gpu(control_mode):
    _twin_of_pipelined(GPU, None, control_mode=control_mode)


# ------------------------------------------------------------------------------------------------ 2. mask edge cases
def _mask_edge_cases(tier, lib):
    kw = dict(device_reset=True, starting_seed=3)
    A, C = _make(tier, lib, **kw), _make(tier, lib, **kw)
    B = A.B
    # an all-true mask is mask=None (here: the first reset of both envs)
    A.reset(mask=torch.ones(B, dtype=torch.bool, device=A.device)); C.reset()
    _sync(A); _sync(C)
    a = _state(A)
    _assert_rows_equal(a, _state(C), what="all-true mask against mask=None")
    assert int(a["placement_failed"].max()) == 0 and not bool(a["episode_started"].any()) and not bool(a["resetting"].any()) and int(a["stage"].max()) == 0
    # an empty mask: nothing changes and the observation is observe(); a mask that lives on the host is seen to be empty, no launch is issued
    counter = int(A.recipe.step)
    obs = A.reset(mask=torch.zeros(B, dtype=torch.bool))
    assert int(A.recipe.step) == counter
    _assert_rows_equal(a, _state(A), what="empty mask (host)")
    assert all(torch.equal(obs[q], A.observe()[q]) for q in obs)
    obs = A.reset(mask=torch.zeros(B, dtype=torch.bool, device=A.device))      # (a device mask is not read back: its launches skip every env)
    A.recipe.step = counter
    _sync(A)
    _assert_rows_equal(a, _state(A), what="empty mask (device)")
    assert all(torch.equal(obs[q], A.observe()[q]) for q in obs)
    # an S-type env whose rows say "inside the recipe" (as a reset cut short would leave them): the forced end restarts it -- the same result as for the untouched twin
    rows, others = [0, B - 1], list(range(1, B - 1))
    A.stage[rows] = 2; A.left[rows] = 1; A.hold[rows] = 1; A.frozen[rows] = 4; A.resetting[rows] = True; A.solver_active[rows] = 0; A.nticks[rows] = 1
    A.scripted[rows] = 0.5
    before = _state(C)
    A.reset(mask=_mask(A, rows), on_device=True); C.reset(mask=_mask(C, rows), on_device=True)
    _sync(A); _sync(C)
    a, c = _state(A), _state(C)
    _assert_rows_equal(a, c, what="restart of an env inside its recipe (synchronous env)")
    _assert_rows_equal(before, c, rows=others, what="rows outside the mask")
    assert not torch.equal(before["qpos"][rows], c["qpos"][rows]) and int(c["stage"].max()) == 0
    # a pipelined env two steps into the recipe of every env: reset(mask, on_device=True) restarts the masked envs' episodes now, the others go on where they were
    P = _make(tier, lib, pipelined_reset=True, max_timesteps_per_goal_per_obj=1, **kw)
    P.reset()
    for k in range(7):
        info = P.step(_zero_action(P))[3]
    assert bool(info["resetting"].all()) and int(P.stage.min()) >= 1
    before = _state(P)
    P.reset(mask=_mask(P, rows), on_device=True)
    _sync(P)
    p = _state(P)
    _assert_rows_equal(before, p, rows=others, what="pipelined env, rows outside the mask")
    for k in ("stage", "left", "hold", "hold_ctrl", "frozen", "steps", "t", "ssl", "successes"):
        assert int(p[k][rows].abs().max()) == 0, k
    assert not bool(p["resetting"][rows].any()) and not bool(p["done"][rows].any()) and not bool(p["episode_started"][rows].any()) and int(p["placement_failed"].max()) == 0
    assert bool((p["solver_active"][rows] == 1).all()) and bool((p["nticks"][rows] == 2).all())
    assert not torch.equal(before["goal"][rows], p["goal"][rows])
    _rests_on_table(P, rows)
    for k in range(3):      # the others finish their recipe on step 10, the restarted envs are live
        info = P.step(_zero_action(P))[3]
    _sync(P)
    assert bool(info["episode_started"][others].all()) and not bool(info["episode_started"][rows].any()) and not bool(info["resetting"].any())
    assert bool((P.steps[rows] == 3).all()) and bool((P.steps[others] == 0).all())


def test_sync_reset_mask_edge_cases_emul(emul_lib):
    _mask_edge_cases(EMUL, emul_lib)


@pytest.mark.gpu
def test_sync_reset_mask_edge_cases_gpu():
    _mask_edge_cases(GPU, None)


# ------------------------------------------------------------------------------------------------ 3. reset_goals() on the device
def _reset_goals_twin(tier, lib, goal_kind):
    """Two synchronous envs and a pipelined one, equal after their host resets; a success threshold every env meets on the first step.  The pipelined env's step
    already made the next goals (its regoal branch, launch counter 1); reset_goals() on the device makes the same draw."""
    kw = dict(device_reset=True, starting_seed=5, goal_kind=goal_kind, success_threshold={"obj_pos": 10.0, "obj_rot": 10.0})
    if goal_kind == "reach":
        kw["num_objects"] = 1
    A, C, P = _make(tier, lib, **kw), _make(tier, lib, **kw), _make(tier, lib, pipelined_reset=True, **kw)
    B = A.B
    for env in (A, C, P):
        env.reset(on_device=False)
    goal0, qpos0 = A.goal.clone(), A.sim.qpos.clone()
    for env in (A, C, P):
        env.step(_zero_action(env))
    assert bool(A.goal_reset.all()) and bool(C.goal_reset.all()) and not bool(A.done.any()) and int(A.recipe.step) == 0 and int(P.recipe.step) == 1
    assert torch.equal(A.goal, goal0) and not torch.equal(P.goal, goal0)
    keys = ("goal", "goal_rot", "qpos_goal", "packed", "prev_valid", "prev_nsucc", "qpos", "goal_reset", "reward", "done")
    A.reset_goals()
    _sync(A); _sync(P)
    _assert_rows_equal(_state(P), _state(A), keys=keys, what="reset_goals() against the pipelined step's regoal")
    assert int(A.placement_failed.max()) == 0 and torch.equal(A.observe()["goal_obj_pos"], A.goal[:, :, :3])
    if goal_kind == "reach":      # the object moved to the new placement, the goal target_height above it
        q = A.obj_q[0]
        assert not torch.equal(A.sim.qpos[:, q:q + 2], qpos0[:, q:q + 2])
        assert torch.equal(A.sim.qpos[:, q:q + 2], A.goal[:, 0, :2]) and torch.allclose(A.sim.qpos[:, q + 2] + A.target_height, A.goal[:, 0, 2], atol=1e-6)
        assert torch.allclose(A.observe()["obj_pos"][:, 0, :2], A.goal[:, 0, :2], atol=1e-6)
    # some envs flagged: those get P's goals (no draw depends on the other envs), the others keep every row
    rows, others = [0, B - 1], list(range(1, B - 1))
    C.goal_reset[others] = False
    before = _state(C)
    C.reset_goals()
    _sync(C)
    c = _state(C)
    _assert_rows_equal(_state(P), c, rows=rows, keys=keys, what="flagged envs")
    _assert_rows_equal(before, c, rows=others, what="unflagged envs")


@pytest.mark.parametrize("goal_kind", ["object_state", "reach"])
def test_reset_goals_on_device_emul(emul_lib, goal_kind):
    _reset_goals_twin(EMUL, emul_lib, goal_kind)


@pytest.mark.gpu
@pytest.mark.parametrize("goal_kind", ["object_state", "reach"])
def test_reset_goals_on_device_gpu(goal_kind):
    _reset_goals_twin(GPU, None, goal_kind)


# ------------------------------------------------------------------------------------------------ 4. what the recipe kernel supports
def _boxes(env, pos, yaw, counts):
    """centres and half extents [B, N, 2] of the objects' yawed bounding boxes at body positions `pos` [B, N, 3]"""
    cen = np.stack([np.cos(yaw) * env.obj_center[:, 0] - np.sin(yaw) * env.obj_center[:, 1], np.sin(yaw) * env.obj_center[:, 0] + np.cos(yaw) * env.obj_center[:, 1]], -1)
    return pos[..., :2] + cen, env._aabb_half(yaw)[..., :2]


def _rests_on_table(env, rows=None):
    rows = list(range(env.B)) if rows is None else rows
    q = env.sim.qpos.cpu().numpy().astype(np.float64)[rows]
    counts = np.full(len(rows), env.N) if env.num_active is None else env.num_active.cpu().numpy()[rows]
    z = np.stack([q[:, qa + 2] for qa in env.obj_q], 1) + env.obj_center[:, 2] - env.obj_half[:, 2] - env.table_height
    used = np.arange(env.N)[None, :] < counts[:, None]
    assert np.abs(z[used]).max() < 5e-3, "objects rest on the table: %.3e" % np.abs(z[used]).max()


def _placement_checks(env, tol_obj=5e-3):
    """After a device reset of every env: the objects (where the recipe's physics left them: `tol_obj`) and the goals' footprints (as placed: 1e-5) inside each env's
    placement area, object boxes pairwise apart, objects resting on the table, status words zero, finite rows, no placement that ran out of restarts."""
    _sync(env)
    assert int(env.placement_failed.max()) == 0 and int(env.stage.max()) == 0 and not bool(env.done.any()) and int(env.steps.max()) == 0
    B, N = env.B, env.N
    counts = np.full(B, N) if env.num_active is None else env.num_active.cpu().numpy()
    q = env.sim.qpos.cpu().numpy().astype(np.float64)
    yaw = env.yaw.cpu().numpy().astype(np.float64)
    pos = np.stack([q[:, qa:qa + 3] for qa in env.obj_q], 1)
    goal, gyaw = env.goal.cpu().numpy().astype(np.float64), env.goal_rot.cpu().numpy().astype(np.float64)[..., 2]
    oc, oh = _boxes(env, pos, yaw, counts)
    gc, gh = _boxes(env, goal[..., :3], gyaw, counts)
    for e in range(B):
        n = int(counts[e])
        (off_x, off_y, _), (width, height, _) = env.placement_area(n)
        lo = np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2]
        hi = lo + [width, height]
        if not env.reach:      # (reach: the goal moved the object itself; its footprint is checked as the goal's)
            assert np.all(oc[e, :n] - oh[e, :n] >= lo - tol_obj) and np.all(oc[e, :n] + oh[e, :n] <= hi + tol_obj), "env %d: an object outside the placement area" % e
            for i in range(n):
                for j in range(i + 1, n):
                    assert (np.abs(oc[e, i] - oc[e, j]) >= oh[e, i] + oh[e, j] - tol_obj).any(), "env %d: objects %d and %d overlap" % (e, i, j)
        m = 1 if env.goal_kind_name == "stack" else n      # (the stack goal places object 0's box; the others stand on it with yaws of their own)
        assert np.all(gc[e, :m] - gh[e, :m] >= lo - 1e-5) and np.all(gc[e, :m] + gh[e, :m] <= hi + 1e-5), "env %d: a goal outside the placement area" % e
        if env.goal_kind_name == "object_state":
            for i in range(n):
                for j in range(i + 1, n):
                    assert (np.abs(gc[e, i] - gc[e, j]) >= gh[e, i] + gh[e, j] - 1e-6).any(), "env %d: goals %d and %d overlap" % (e, i, j)
    _rests_on_table(env)
    obs = env.observe()
    assert torch.equal(obs["goal_obj_pos"], env.goal[:, :, :3]) and all(bool(torch.isfinite(v).all()) for v in obs.values())
    return obs


def _coverage_case(tier, lib, case):
    kw = dict(device_reset=True, starting_seed=7)
    if case == "stack":
        env = _make(tier, lib, goal_kind="stack", num_objects=3, **kw)
    elif case == "reach":
        env = _make(tier, lib, goal_kind="reach", num_objects=1, **kw)
    elif case == "groups":
        env = _make(tier, lib, object_groups="sample", **kw)
    elif case == "joint":
        env = _make(tier, lib, control_mode="joint", **kw)
    elif case == "ycb":
        from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv
        env = _make(tier, lib, cls=BatchedYcbRearrangeEnv, **kw)
    elif case == "wrapped":
        args = dict(lib=lib) if lib is not None else {}
        env = blocks.make_env(batch_size=tier["B"], device=tier["device"], n_substeps=tier["n_substeps"], stabilize_steps=2, settle_steps=2,
                              parameters={"n_random_initial_steps": 1}, device_reset=True, starting_seed=7, **args)
        assert env.wrapped and env.device_reset and not env.pipelined
    else:
        raise AssertionError(case)
    obs = env.reset()
    _placement_checks(env)
    if case == "stack":
        g = env.goal.cpu().numpy()
        assert np.abs(g[:, :, :2] - g[:, :1, :2]).max() == 0 and np.allclose(np.sort(g[:, :, 2] - g[:, :, 2].min(1, keepdims=True), 1), np.arange(3) * 2 * env.object_size, atol=1e-6)
    if case == "groups":
        ids = env.obj_group.cpu().numpy()
        assert (ids[:, 0] == 0).all() and (np.diff(ids, axis=1) >= 0).all() and (np.diff(ids, axis=1) <= 1).all()
    if case == "wrapped":
        assert float(obs["action_ema"].abs().max()) == 0.0
    # the new episodes are live: one step, then a reset of {0, B - 1} that leaves the others alone
    out = env.step(_zero_action(env))
    _sync(env)
    assert int(env.steps.min()) == 1 and bool(torch.isfinite(out[1]).all())
    rows, others = [0, env.B - 1], list(range(1, env.B - 1))
    before = _state(env)
    env.reset(mask=_mask(env, rows))
    _sync(env)
    _assert_rows_equal(before, _state(env), rows=others, what="%s: rows outside the mask" % case)
    assert bool((env.steps[rows] == 0).all()) and bool((env.steps[others] == 1).all()) and int(env.placement_failed.max()) == 0
    if case == "wrapped":
        assert float(env.observe()["action_ema"][rows].abs().max()) == 0.0


@pytest.mark.parametrize("case", ["stack", "reach", "groups", "joint", "wrapped", "ycb"])
def test_sync_reset_coverage_emul(emul_lib, case):
    _coverage_case(EMUL, emul_lib, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["stack", "reach", "groups", "joint", "wrapped", "ycb"])
def test_sync_reset_coverage_gpu(case):
    _coverage_case(GPU, None, case)


def _num_objects_case(tier, lib):
    """max_num_objects = 5: the count written before the reset is latched at the forced end, unused objects sit at their parking poses with their weight cancelled,
    the padded observation entries are zero"""
    env = _make(tier, lib, device_reset=True, starting_seed=9, num_objects=3, max_num_objects=5)
    B = env.B
    env.reset()
    _sync(env)
    assert bool((env.num_active == 3).all())
    _placement_checks(env)
    want = (np.arange(B) % 5 + 1).astype(np.int32); want[0], want[B - 1] = 2, 5
    env.set_num_objects_next(want)
    env.reset()
    obs = _placement_checks(env)
    assert np.array_equal(env.num_active.cpu().numpy(), want)
    q, park = env.sim.qpos.cpu().numpy(), env.park_pose
    P = env.sim.params
    mass, grav, xfrc, damp = (P[k].cpu().numpy() for k in ("body_mass", "gravity", "xfrc_applied", "dof_damping"))
    bodies = env._obj_bodies.cpu().numpy()
    for e in range(B):
        for i in range(env.N):
            b, dofs = bodies[i], np.arange(env.obj_v[i], env.obj_v[i] + 6)
            if i >= want[e]:
                assert np.abs(q[e, env.obj_q[i]:env.obj_q[i] + 7] - park[i]).max() < 1e-4, "env %d: unused object %d left its parking pose" % (e, i)
                assert np.array_equal(xfrc[e, b, :3], -mass[e, b] * grav[e]) and np.all(damp[e, dofs] == np.float32(blocks.PARK_DAMPING))
                for key in ("obj_pos", "obj_rel_pos", "obj_vel_pos", "obj_rot", "obj_vel_rot", "goal_obj_pos", "goal_obj_rot", "rel_goal_obj_pos", "rel_goal_obj_rot",
                            "obj_gripper_contact", "obj_bbox_size", "obj_colors"):
                    assert float(obs[key][e, i].abs().max()) == 0.0, (key, e, i)
            else:
                assert np.all(xfrc[e, b] == 0) and np.array_equal(damp[e, dofs], env._param_defaults["dof_damping"][dofs].cpu().numpy())
    # a masked reset latches the masked envs' counts only
    env.set_num_objects_next(1)
    env.reset(mask=_mask(env, [0, B - 1]))
    _sync(env)
    want[[0, B - 1]] = 1
    assert np.array_equal(env.num_active.cpu().numpy(), want)


def test_sync_reset_num_objects_emul(emul_lib):
    _num_objects_case(EMUL, emul_lib)


@pytest.mark.gpu
def test_sync_reset_num_objects_gpu():
    _num_objects_case(GPU, None)


# ------------------------------------------------------------------------------------------------ 5. no synchronisation
@contextlib.contextmanager
def _sync_is_an_error():
    """torch.cuda.set_sync_debug_mode("error") where this build honours it (a probe readback must raise under it); otherwise Tensor.cpu / item / tolist / nonzero
    patched to raise.  Yields which of the two is in force."""
    probe = torch.ones(1, device="cuda:0")
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            live = False
        except RuntimeError:
            live = True
        if live:
            yield "set_sync_debug_mode"
            return
    finally:
        torch.cuda.set_sync_debug_mode(before)
    def refuse(*a, **k):
        raise RuntimeError("a synchronising call inside the device path")
    saved = {n: getattr(torch.Tensor, n) for n in ("cpu", "item", "tolist", "nonzero")}
    try:
        for n in saved:
            setattr(torch.Tensor, n, refuse)
        yield "patched Tensor.cpu / item / tolist / nonzero"
    finally:
        for n, f in saved.items():
            setattr(torch.Tensor, n, f)


@pytest.mark.gpu
@pytest.mark.parametrize("goal_kind", ["object_state", "reach"])
def test_sync_reset_does_not_synchronise_gpu(goal_kind):
    """reset_goals(), reset(mask) and reset() of a synchronous device env (non-zero gravity randomizer, so the randomizers draw) under the synchronisation check; the
    host recipe trips the same check, which shows it is live.  With the ROCm build of torch the GPU tier runs on, torch.cuda.set_sync_debug_mode("error") is honoured (it is the
    check that ran, and it caught the randomizers' index uploads in a first version of the path); the patched-method fallback is for builds where the probe does not raise."""
    kw = dict(num_objects=1) if goal_kind == "reach" else {}
    env = _make(GPU, None, device_reset=True, starting_seed=2, goal_kind=goal_kind, success_threshold={"obj_pos": 10.0, "obj_rot": 10.0}, randomizer_params={"gravity": 0.1}, **kw)
    env.reset()
    env.step(_zero_action(env))
    _sync(env)
    assert bool(env.goal_reset.all())
    mask, goal0 = _mask(env, [0, env.B // 2, env.B - 1]), env.goal.clone()
    with _sync_is_an_error() as how:
        print("synchronisation check:", how)
        env.reset_goals()
        env.reset(mask=mask)
        env.reset()
        with pytest.raises(RuntimeError):      # the check is live: the host recipe reads the mask back
            env.reset(mask=mask, on_device=False)
        env.goal_reset.fill_(True)
        with pytest.raises(RuntimeError):
            env.reset_goals(on_device=False)
    _sync(env)
    assert not torch.equal(env.goal, goal0) and int(env.steps.max()) == 0


# ------------------------------------------------------------------------------------------------ 6. surface
def _surface(tier, lib):
    S = _make(tier, lib, device_reset=True, pipelined_reset=False, starting_seed=4)
    assert S.device_reset and not S.pipelined and S._on_device(None) and not S._on_device(False)
    H = _make(tier, lib, starting_seed=4)
    assert not H._on_device(None)
    with pytest.raises(ValueError, match="device_reset"):
        H.reset(on_device=True)
    with pytest.raises(ValueError, match="device_reset"):
        H.reset_goals(on_device=True)
    # a synchronous device env steps as the env without device_reset does: equal host resets, then bit-identical outputs
    S.reset(on_device=False); H.reset()
    for k in range(2):
        (os_, rs, ds, is_), (oh, rh, dh, ih) = S.step(_zero_action(S)), H.step(_zero_action(H))
        assert torch.equal(rs, rh) and torch.equal(ds, dh) and all(torch.equal(os_[q], oh[q]) for q in oh) and all(torch.equal(is_[q], ih[q]) for q in ih)
    # a pipelined device env keeps its host reset unless told otherwise
    kw = dict(device_reset=True, pipelined_reset=True, starting_seed=4)
    P1, P2 = _make(tier, lib, **kw), _make(tier, lib, **kw)
    assert not P1._on_device(None)
    P1.reset(); P2.reset(on_device=False)
    _sync(P1); _sync(P2)
    _assert_rows_equal(_state(P1), _state(P2), what="reset() against reset(on_device=False) of a pipelined device env")
    assert int(P1.recipe.step) == 0 and int(P2.recipe.step) == 0      # (no recipe launch: the host recipe ran)


def test_sync_reset_surface_emul(emul_lib):
    _surface(EMUL, emul_lib)
    with pytest.raises(NotImplementedError, match="mocap"):      # the mocap arm keeps its refusal
        BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, tcp_solver_mode="mocap", device_reset=True, **FAST)


@pytest.mark.gpu
def test_sync_reset_surface_gpu():
    _surface(GPU, None)


def _grouped_refusal(tier, lib):
    from robogym_amd.envs.rearrange.ycb import GroupedYcbRearrangeEnv

    args = dict(lib=lib) if lib is not None else {}
    env = GroupedYcbRearrangeEnv(tier["B"], device=tier["device"], object_sets=(0, 1), starting_seed=4, n_substeps=tier["n_substeps"], pipelined_reset=True, device_reset=True,
                                 **FAST, **args)
    with pytest.raises(NotImplementedError, match="on_device"):
        env.reset(on_device=True)
    with pytest.raises(NotImplementedError, match="on_device"):
        env.reset(mask=torch.ones(env.B, dtype=torch.bool, device=env.device), on_device=True)


def test_grouped_ycb_refuses_on_device_emul(emul_lib):
    _grouped_refusal(EMUL, emul_lib)


@pytest.mark.gpu
def test_grouped_ycb_refuses_on_device_gpu():
    _grouped_refusal(GPU, None)


# ------------------------------------------------------------------------------------------------ 7. the parameter rows' launch against the host route's methods
# (ended, stabilised, episode_started) per env; an env of the last pattern has its masks set and `active` = 0
ROW_PATTERNS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 0, 0), (1, 1, 1))


def _param_rows_against_host_route(tier, lib, counted):
    """ra_param_rows_kernel, the device route's only implementation of the per-env parameter rows, against the host route's: the `_param_defaults` restore for
    `ended`, then `_set_object_damping`, then `_apply_parking`, run on the env's own block and swapped out again.  Env e has pattern (e + shift) mod 6 of
    ROW_PATTERNS and, `counted` (max_num_objects = 5), (e + shift) mod 5 + 1 objects; three shifts, so that B = 4 meets every pattern too.  Every word of the block
    is perturbed per env, `body_mass` and `gravity` once more with the env's index.  One launch with both stages: the whole block bit-equal on every env, the
    skipped envs (no mask byte, or outside `active`) as they were to the byte.  52 of the 874 words of a block lie between the named fields (alignment); no
    host method addresses them, the kernel's restore of an ended env returns them to the model's values with the rest, which is what is expected of them here.
    Not `counted`: `num_active` = NULL, nothing is parked."""
    env = _make(tier, lib, device_reset=True, starting_seed=6, **(dict(num_objects=3, max_num_objects=5) if counted else {}))
    B, P, dev = env.B, env.sim.params, env.device
    assert bool(env.param_rows.num_active) == counted
    default = env._param_block_default.clone()
    P.block.zero_()
    for k in P.keys():
        P[k].fill_(1.0)
    between = torch.nonzero(P.block[0] == 0).flatten()
    bits = lambda t: t.contiguous().view(torch.int32)
    e = torch.arange(B, device=dev)
    for shift in (0, 2, 4):
        pattern = torch.tensor(ROW_PATTERNS, device=dev)[(e + shift) % 6].bool()
        active = (e + shift) % 6 != 5
        env.ended.copy_(pattern[:, 0]); env.stabilised.copy_(pattern[:, 1]); env.episode_started.copy_(pattern[:, 2]); env.active_row.copy_(active)
        touched = pattern.any(1) & active
        if counted:
            env.num_active.copy_(((e + shift) % 5 + 1).to(torch.int32))
        noise = torch.rand(P.block.shape, generator=torch.Generator().manual_seed(100 + shift)).to(dev)
        P.block.copy_(default[None, :] * (1.0 + noise) + 0.25 * noise + 0.01)
        P["body_mass"].mul_(1.0 + 0.1 * e[:, None]); P["gravity"].add_(0.01 * e[:, None])
        start = P.block.clone()
        assert bool((bits(start) != bits(default)[None, :]).all()), "a word of the block was left at the model's value"
        # the host route's methods, in its order
        ended = torch.nonzero(env.ended & active).flatten()
        for k, v in env._param_defaults.items():
            P[k][ended] = v
        env._set_object_damping(ended, env.stabilize_object_damping)
        env._set_object_damping(torch.nonzero(env.stabilised & ~env.ended & active).flatten(), None)
        if counted:
            env._apply_parking(touched)
        want = P.block.clone()
        want[ended[:, None], between[None, :]] = default[between]
        P.block.copy_(start)
        env._param_rows_launch(_native.RA_ROWS_RESTORE | _native.RA_ROWS_PARK, env.active_row)
        env.sync()
        got = P.block.clone()
        assert torch.equal(bits(got), bits(want)), "shift %d: envs %s differ from the host route's rows" % (shift, torch.nonzero((bits(got) != bits(want)).any(1)).flatten().tolist())
        assert torch.equal(bits(got[~touched]), bits(start[~touched])) and bool((bits(got[ended]) != bits(start[ended])).any(1).all())
        if counted:      # (the case is live: unused objects exist and hold their parking rows)
            unused = touched[:, None] & (env._slot[None, :] >= env.num_active[:, None])
            assert bool(unused.any()) and bool((P["dof_damping"][:, env.obj_dofs].unflatten(1, (env.N, 6))[unused] == blocks.PARK_DAMPING).all())


@pytest.mark.parametrize("counted", [True, False])
def test_param_rows_launch_is_the_host_route_emul(emul_lib, counted):
    _param_rows_against_host_route(EMUL, emul_lib, counted)


@pytest.mark.gpu
@pytest.mark.parametrize("counted", [True, False])
def test_param_rows_launch_is_the_host_route_gpu(counted):
    _param_rows_against_host_route(GPU, None, counted)


def test_sync_reset_header_matches_the_library_and_the_binding():
    """include/rgstep_sync_reset.h (included by include/rgstep.h) under the rule tests/test_boundary.py applies to rgstep.h itself: the gfx950 build of the library
    exports what it declares, the binding lists the same names, and the argument structs have the library's sizes."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = ctypes.CDLL(os.path.join(root, "robogym_amd", "csrc", "librgstep.so"))
    declared = sorted(set(re.findall(r"\b(r[gba]_[a-z_0-9]+)\s*\(", open(os.path.join(root, "include", "rgstep_sync_reset.h")).read())))
    assert declared == ["ra_env_param_rows", "ra_param_rows_args_size"] and set(_native.EXPORTS_SYNC_RESET) == set(declared)
    assert '#include "rgstep_sync_reset.h"' in open(os.path.join(root, "include", "rgstep.h")).read()
    for name in declared:
        assert hasattr(L, name), name
    assert L.ra_param_rows_args_size() == ctypes.sizeof(_native.RaParamRowsArgs) and L.ra_recipe_args_size() == ctypes.sizeof(_native.RaRecipeArgs)
