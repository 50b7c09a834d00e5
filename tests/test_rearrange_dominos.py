"""rearrange/dominos and the goal-orientation axis of the rearrange family: the rotation distance modes mod90 / mod180 of ra_post_step_kernel, goal yaw randomisation
and the domino arc of ra_recipe_kernel and of the host recipe, the domino world, `envs/rearrange/dominos.py`.  Against tests/golden/rearrange_dominos.npz and
rearrange_dominos_worlds.json (the reference's own code on stubs, tools/gen_golden_rearrange_dominos.py), by the goals' properties over many envs, and against the
unchanged oracle.  CPU: host path and the kernel source on the emulation harness; `-m gpu`: the MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from robogym_amd.envs.rearrange import blocks, blocks_train, dominos
from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv, domino_goal, randomize_yaw_along_z
from robogym_amd.envs.rearrange.xml import load_dominos_model

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FAST = dict(n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
ABOVE_TABLE = np.array([1.45, 0.77, 0.9])      # (the golden's positions are around the origin: somewhere above the table, nothing touches)
_cache = {}


def _golden():
    if "g" not in _cache:
        _cache["g"] = dict(np.load(os.path.join(GOLDEN, "rearrange_dominos.npz")))
    return _cache["g"]


def _lib_args(lib):
    return dict(lib=lib, **FAST) if lib is not None else dict(stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)


# ------------------------------------------------------------------------------------------------ 1. the goal layer against the reference's code
def test_parallel_quat_tables_are_the_reference_tables():
    """utils/rotation.py parallel_quat_table: the reference's PARALLEL_QUATS / PARALLEL_QUATS_180 entry for entry (the order decides ties), up to the quaternion's sign"""
    from robogym_amd.utils.rotation import parallel_quat_table

    g = _golden()
    for mode, key in (("mod90", "parallel_quats"), ("mod180", "parallel_quats_180")):
        ours, ref = parallel_quat_table(mode), g[key]
        assert ours.shape == ref.shape and np.minimum(np.abs(ours - ref).max(1), np.abs(ours + ref).max(1)).max() < 1e-15


def _observe_states(env, cur_pos, cur_rot, goal_pos, goal_rot):
    """`_env_kernel_goal_layer`'s protocol (tests/test_rearrange_env.py): the objects put at (cur_pos, euler2quat(cur_rot)), the goal rows written, one forward, the env
    kernel -- once as the first observation of an episode (distances), once as a re-observation under a new goal (is_goal_achieved)."""
    from oracle import rearrange_oracle as RO

    quat, gq = RO.euler2quat(cur_rot), RO.euler2quat(goal_rot)
    for i, qa in enumerate(env.obj_q):
        env.sim.qpos[:, qa:qa + 7] = torch.tensor(np.concatenate([cur_pos[:, i] + ABOVE_TABLE, quat[:, i]], -1).astype(np.float32), device=env.device)
    env.goal[:] = torch.tensor(np.concatenate([goal_pos + ABOVE_TABLE, gq], -1).astype(np.float32), device=env.device)
    env.goal_rot[:] = torch.tensor(goal_rot.astype(np.float32), device=env.device)
    env.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=32)
    env._observe_only()
    env._reobserve(np.zeros(0, dtype=np.int64), np.arange(env.B))
    env.sync()
    obs = env.observe()
    return (obs["rel_goal_obj_pos"].cpu().numpy(), obs["rel_goal_obj_rot"].cpu().numpy(), env.goal_dist.cpu().numpy().astype(np.float64),
            obs["is_goal_achieved"][:, 0].cpu().numpy())


def _goal_layer(lib, device, B, mode):
    """Tolerances: test_rearrange_env.py `_env_kernel_goal_layer`'s own -- rel pos 2e-6, rel rot 2e-5 away from the gimbal lock, as a quaternion 2e-6, summed
    distances 5e-5; is_goal_achieved exactly (the golden keeps 1e-3 from both thresholds)."""
    from oracle import rearrange_oracle as RO

    g = _golden()
    env = BatchedBlockRearrangeEnv(B, device=device, rot_dist_type=mode, **_lib_args(lib))
    env.reset()
    assert env.post.rot_dist_type == {"full": 0, "mod90": 1, "mod180": 2}[mode]
    worst = np.zeros(4)
    if mode != "full":
        a = {k: g["a_%s_%s" % (mode, k)] for k in ("cur_pos", "cur_rot", "goal_pos", "goal_rot", "rel_pos", "rel_rot", "dist_pos", "dist_rot")}
        T = len(a["cur_pos"]) // B * B if lib is None else 3 * B
        thr_p, thr_r = float(g["pos_threshold"]), float(g["rot_threshold"])
        achieved_seen = set()
        for t0 in range(0, T, B):
            sl = slice(t0, t0 + B)
            rp, rr, gd, ach = _observe_states(env, a["cur_pos"][sl], a["cur_rot"][sl], a["goal_pos"][sl], a["goal_rot"][sl])
            e_rr = np.abs(RO.normalize_angles(rr - a["rel_rot"][sl]))
            q_k, q_g = RO.euler2quat(rr.astype(np.float64)), RO.euler2quat(a["rel_rot"][sl])
            e_q = np.minimum(np.abs(q_k - q_g).max(-1), np.abs(q_k + q_g).max(-1))
            lock = np.abs(np.abs(a["rel_rot"][sl][..., 1]) - np.pi / 2) < 0.05
            worst = np.maximum(worst, [np.abs(rp - a["rel_pos"][sl]).max(), e_rr[~lock].max() if (~lock).any() else 0.0, e_q.max(),
                                       np.abs(gd[:, 0] - a["dist_pos"][sl].sum(-1)).max() + np.abs(gd[:, 1] - a["dist_rot"][sl].sum(-1)).max()])
            want = ((a["dist_pos"][sl] < thr_p) & (a["dist_rot"][sl] < thr_r)).all(-1)
            assert np.array_equal(ach.astype(bool), want), (t0, ach, want)
            achieved_seen |= set(want.tolist())
        assert achieved_seen == {True, False}
        # exact ties between two candidates: either may win in fp32 -- the distance is the same
        tie = {k: g["a_tie_%s_%s" % (mode, k)] for k in ("goal_rot", "cur_rot", "pos", "dist_rot")}
        for t0 in range(0, len(tie["pos"]) // B * B if lib is None else B, B):
            sl = slice(t0, t0 + B)
            gd = _observe_states(env, tie["pos"][sl], tie["cur_rot"][sl], tie["pos"][sl], tie["goal_rot"][sl])[2]
            worst[3] = max(worst[3], np.abs(gd[:, 1] - tie["dist_rot"][sl].sum(-1)).max())
    # the reference's angle -> distance table of this mode (test_object_rotation.py), one object turned about z, the others at their goals
    ang, dist = g["b_%s_angle" % mode], g["b_%s_dist" % mode]
    N = env.N
    for t0 in range(0, len(ang), B):
        n = min(B, len(ang) - t0)
        goal_rot = np.zeros((B, N, 3)); goal_rot[..., 2] = float(g["b_base_yaw"])
        cur_rot = goal_rot.copy(); cur_rot[:n, 0, 2] -= ang[t0:t0 + n]
        pos = np.zeros((B, N, 3)); pos[..., 0] = 0.1 * np.arange(N)
        gd = _observe_states(env, pos, cur_rot, pos, goal_rot)[2]
        worst[3] = max(worst[3], np.abs(gd[:n, 1] - dist[t0:t0 + n]).max())
    print("env kernel goal layer, %s, vs the reference's code: rel pos %.1e, rel rot (Euler, away from gimbal lock) %.1e, as a quaternion %.1e, distances %.1e" % ((mode,) + tuple(worst)))
    assert worst[0] < 2e-6 and worst[1] < 2e-5 and worst[2] < 2e-6 and worst[3] < 5e-5


@pytest.mark.parametrize("mode", ["mod90", "mod180", "full"])
def test_rot_dist_modes_match_reference_code_emul(emul_lib, mode):
    _goal_layer(emul_lib, "cpu", 4, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mod90", "mod180", "full"])
def test_rot_dist_modes_match_reference_code_gpu(mode):
    _goal_layer(None, "cuda:0", 16, mode)


# ------------------------------------------------------------------------------------------------ 2. the world
@pytest.mark.parametrize("N", [1, 2, 5])
@pytest.mark.parametrize("ecc", [1.5, 2.5])
def test_dominos_world_equals_the_mjcf_build(N, ecc):
    """`load_dominos_model(N, e)` derives the world from the shipped 5-block one: every array as compile_mjcf builds the domino MJCF (the same bytes; the constants
    set_constants computes through a matrix inverse to 1e-12), the same name tables -- test_smaller_blocks_worlds_equal_the_mjcf_build's comparison."""
    want = json.load(open(os.path.join(GOLDEN, "rearrange_dominos_worlds.json")))["%d_%g" % (N, ecc)]
    m = load_dominos_model(N, ecc)
    assert m.names == want["names"]
    assert set(m.arrays) == set(want["arrays"]) | set(want["computed"])
    for k, w in want["arrays"].items():
        a = np.ascontiguousarray(m.arrays[k])
        assert [list(a.shape), a.dtype.str, hashlib.sha256(a.tobytes()).hexdigest()] == [w["shape"], w["dtype"], w["sha256"]], k
    for k, v in want["computed"].items():
        a, v = np.asarray(m.arrays[k], dtype=np.float64).ravel(), np.asarray(v)
        assert a.shape == v.shape and np.all(np.abs(a - v) <= 1e-12 * np.maximum(1.0, np.abs(v))), k
    g = int(m.arrays["body_geomadr"][m.name2id("body", "object0")])
    assert np.abs(m.arrays["geom_size"][g] - 0.0254 * np.array([1 / ecc, 1, ecc])).max() <= 5e-7      # (the sizes pass through the MJCF attribute's text: six decimals)


# ------------------------------------------------------------------------------------------------ 3. the host generator replays the reference
class ReplayRandom:
    """Stands in for the env's RandomState: hands out the recorded draws in order"""

    def __init__(self, draws):
        self.q = list(np.asarray(draws).ravel())

    def random_sample(self):
        return self.q.pop(0)

    def uniform(self, low=0.0, high=1.0, size=None):
        return np.array([self.q.pop(0) for _ in range(int(np.prod(size or 1)))]).reshape(size or ())


def test_host_domino_goal_replays_the_reference_code():
    """`domino_goal` on the golden's draw logs: the positions, yaws and goal_valid `DominoStateGoal._sample_next_goal_positions` produced from the same draws, to 1e-12,
    the calls with retries and the one that runs out of them included"""
    g = _golden()
    retried = exhausted = 0
    for si, (N, ecc, mul, portion) in enumerate(g["c_setups"]):
        N = int(N)
        at = np.concatenate([[0], np.cumsum(g["c%d_ndraw" % si])])
        for call in range(len(g["c%d_valid" % si])):
            rs = ReplayRandom(g["c%d_draws" % si][at[call]:at[call + 1]])
            pos, yaw, ok = domino_goal(rs, np.tile(g["c%d_half" % si], (N, 1)), 0.0254 * mul, g["c_table_pos"], g["c_table_size"], g["c%d_area" % si][0], g["c%d_area" % si][1])
            assert not rs.q and ok == bool(g["c%d_valid" % si][call])
            assert np.abs(pos - g["c%d_pos" % si][call]).max() < 1e-12
            assert np.abs(np.angle(np.exp(1j * (yaw - g["c%d_yaw" % si][call])))).max() < 1e-12
            retried += ok and g["c%d_ndraw" % si][call] > 4; exhausted += not ok
    assert retried >= 3 and exhausted == 1


def test_host_goal_yaw_sampler_replays_the_reference_code():
    """`randomize_yaw_along_z` on the golden's draws: the quaternions `randomize_quaternion_along_z` produced, as z rotations of the new yaws"""
    g = _golden()
    for draws, q_in, q_out in zip(g["d_draws"], g["d_quat_in"], g["d_quat_out"]):
        rs = ReplayRandom(draws)
        yaw = randomize_yaw_along_z(rs, 2 * np.arctan2(q_in[:, 3], q_in[:, 0]))
        q = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
        assert not rs.q and np.minimum(np.abs(q - q_out).max(-1), np.abs(q + q_out).max(-1)).max() < 1e-12


def test_host_recipe_uses_the_domino_goal_emul(emul_lib):
    """the env's host path (`device_reset=False`): `_next_goal` hands the arc's yaws to the goal rows; with randomize_goal_rot the yaws are drawn before the positions"""
    env = BatchedBlockRearrangeEnv(2, device="cpu", lib=emul_lib, goal_kind="dominos", model=load_dominos_model(5), rot_dist_type="mod180", **FAST)
    env.reset()
    assert env.host_placement_failed == 0
    _check_arc(env, env.goal.numpy().astype(np.float64), env.goal_rot.numpy().astype(np.float64), env.qpos_goal.numpy(), tol=2e-6)
    env = BatchedBlockRearrangeEnv(2, device="cpu", lib=emul_lib, randomize_goal_rot=True, **FAST)
    env.reset()
    yaw_obj = 2 * np.arctan2(env.sim.qpos[:, [qa + 6 for qa in env.obj_q]].numpy(), env.sim.qpos[:, [qa + 3 for qa in env.obj_q]].numpy())
    assert np.abs(np.angle(np.exp(1j * (env.goal_rot[..., 2].numpy() - yaw_obj)))).min() > 1e-3


# ------------------------------------------------------------------------------------------------ 4. the device generator's properties
def _area(env):
    (off_x, off_y, _), (width, height, _) = env.placement_area()
    return np.array([off_x, off_y]) - env.table_size[:2] + env.table_pos[:2], np.array([width, height])


def _check_arc(env, goal, goal_rot, qpos_goal, tol=1e-5):
    """goal [B, N, 7], goal_rot [B, N, 3] of a "dominos" env: the arc's geometry.  Returns (offset, delta) per env."""
    B, N = goal.shape[:2]
    yaw = goal_rot[..., 2]
    assert np.abs(goal_rot[..., :2]).max() == 0
    q = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
    assert np.minimum(np.abs(goal[..., 3:] - q).max(-1), np.abs(goal[..., 3:] + q).max(-1)).max() < 2e-6            # the goal quaternion is the z rotation of the goal yaw
    assert np.abs(goal[..., 2] - (env.table_height + env.obj_half[:, 2])).max() < tol                                # z: the box's half height on the table top
    half = env._aabb_half(yaw)[..., :2]
    lo, size = _area(env)
    assert np.all(goal[..., :2] - half >= lo - tol) and np.all(goal[..., :2] + half <= lo + size + tol)              # every yawed box inside the placement area
    for i, qa in enumerate(env.obj_q):
        assert np.abs(qpos_goal[:, qa:qa + 7] - goal[:, i]).max() < 1e-6
    delta = np.zeros(B)
    if N > 1:
        step = np.diff(goal[..., :2], axis=1)
        assert np.abs(np.linalg.norm(step, axis=-1) - env.object_size * env.domino_distance_mul).max() < tol       # consecutive goals one chain step apart
        dyaw = np.angle(np.exp(1j * np.diff(yaw, axis=1)))
        delta = dyaw[:, 0]
        assert np.abs(dyaw - delta[:, None]).max() < 2e-5 and np.abs(delta).max() <= np.pi / 8 + 1e-6                 # one yaw step per env, |delta| <= pi / 8
        # the chain's direction between dominos k and k + 1 is the mean of their yaws: (k + 1) delta + offset
        heading = np.arctan2(step[..., 1], step[..., 0])
        mid = yaw[:, :-1] + 0.5 * delta[:, None]
        assert np.abs(np.angle(np.exp(1j * (heading - mid)))).max() < 2e-3
    # offset = u pi in [0, pi): what is left of the first yaw without its delta / 2 (one domino: delta shows nowhere else, so its yaw itself, within pi / 16 of that range)
    offset = np.mod(yaw[:, 0] - 0.5 * delta + 1e-5, 2 * np.pi) - 1e-5
    if N > 1:
        assert offset.max() <= np.pi + 1e-5
    else:
        assert np.all((offset <= np.pi * 17 / 16 + 1e-5) | (offset >= np.pi * 31 / 16 - 1e-5))
    return offset, delta


def _device_goals(lib, device, B, N, **extra):
    """tests/test_rearrange_tasks.py `_device_goals`: every env is told its episode ended, then (zero-length recipe stages) that it starts -- one launch pair"""
    kw = dict(lib=lib, n_substeps=1) if lib is not None else {}
    env = BatchedBlockRearrangeEnv(B, device=device, num_objects=N, stabilize_steps=0, n_random_initial_steps=0, settle_steps=0, pipelined_reset=True, device_reset=True,
                                   starting_seed=5, **kw, **extra)
    env.stage.zero_(); env.done.fill_(True); env.goal_reset.fill_(False)
    env._advance_recipes_device()
    env.done.fill_(False)
    env._advance_recipes_device()
    env.sync()
    assert bool(env.episode_started.all()) and int(env.placement_failed.max()) == 0
    return env


def _device_arc(lib, device, B, N):
    env = _device_goals(lib, device, B, N, goal_kind="dominos", model=load_dominos_model(N), rot_dist_type="mod180")
    assert env.recipe.goal_kind == 6 and env.post.goal_kind == 0 and env.post.rot_dist_type == 2
    goal, goal_rot = env.goal.cpu().numpy().astype(np.float64), env.goal_rot.cpu().numpy().astype(np.float64)
    offset, delta = _check_arc(env, goal, goal_rot, env.qpos_goal.cpu().numpy())
    assert len(np.unique(np.round(offset, 4))) > 1 and offset.min() < 0.25 * np.pi and offset.max() > 0.75 * np.pi       # the draws span their ranges over the batch
    if N > 1:
        assert len(np.unique(np.round(delta, 4))) > 1 and delta.min() < -np.pi / 16 and delta.max() > np.pi / 16
    # a second goal for everybody (a live env that reached its goal): another arc
    env.goal_reset.fill_(True)
    env._advance_recipes_device()
    env.sync()
    goal2 = env.goal.cpu().numpy().astype(np.float64)
    _check_arc(env, goal2, env.goal_rot.cpu().numpy().astype(np.float64), env.qpos_goal.cpu().numpy())
    assert np.abs(goal2[..., :2] - goal[..., :2]).max() > 1e-3 and int(env.placement_failed.max()) == 0


def _device_random_goal_yaw(lib, device, B, N):
    """kind "object_state" with randomize_goal_rot: goal yaws = the objects' yaws + U(0, 2 pi), the grid placement made for boxes turned by the GOAL yaws"""
    env = _device_goals(lib, device, B, N, randomize_goal_rot=True, model=load_dominos_model(N))      # (a box that is no square from above: the yaw matters to its footprint)
    yaw_obj, yaw = env.yaw.cpu().numpy().astype(np.float64), env.goal_rot[..., 2].cpu().numpy().astype(np.float64)
    turn = np.mod(yaw - yaw_obj, 2 * np.pi)
    assert np.abs(np.angle(np.exp(1j * turn))).min() > 1e-4 and turn.min() < 0.5 and turn.max() > 2 * np.pi - 0.5 and len(np.unique(np.round(turn, 3))) > B // 2
    goal = env.goal.cpu().numpy().astype(np.float64)
    half = env._aabb_half(yaw)[..., :2]
    lo, size = _area(env)
    assert np.all(goal[..., :2] - half >= lo - 1e-5) and np.all(goal[..., :2] + half <= lo + size + 1e-5)
    for i in range(N):
        for j in range(i + 1, N):
            assert (np.abs(goal[:, i, :2] - goal[:, j, :2]) >= half[:, i] + half[:, j] - 1e-6).any(-1).all()
    # the grid's cells are sized by the goal-yawed boxes: the low corner of every box sits on a cell boundary of THAT grid
    ncol = np.floor(size[0] / (2 * half[..., 0].max(1))); cw = size[0] / ncol
    col = (goal[..., 0] - half[..., 0] - lo[0]) / cw[:, None]
    assert np.abs(col - np.round(col)).max() < 1e-3
    q = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
    assert np.minimum(np.abs(goal[..., 3:] - q).max(-1), np.abs(goal[..., 3:] + q).max(-1)).max() < 2e-6


@pytest.mark.parametrize("N", [1, 2, 5])
def test_device_domino_arc_properties_emul(emul_lib, N):
    _device_arc(emul_lib, "cpu", 64, N)
    _device_random_goal_yaw(emul_lib, "cpu", 64, N)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 2, 5])
def test_device_domino_arc_properties_gpu(N):
    _device_arc(None, "cuda:0", 4096, N)
    _device_random_goal_yaw(None, "cuda:0", 4096, N)


def test_device_domino_arc_that_cannot_fit_raises_placement_failed_emul(emul_lib):
    """a chain longer than the placement area: MAX_RETRY attempts, then zero goal positions and placement_failed, as the other kinds raise it"""
    env = BatchedBlockRearrangeEnv(2, device="cpu", lib=emul_lib, num_objects=5, goal_kind="dominos", model=load_dominos_model(5), domino_distance_mul=30.0, n_substeps=1,
                                   stabilize_steps=0, n_random_initial_steps=0, settle_steps=0, pipelined_reset=True, device_reset=True)
    env.stage.zero_(); env.done.fill_(True); env.goal_reset.fill_(False)
    env._advance_recipes_device()
    env.done.fill_(False)
    env._advance_recipes_device()
    assert env.placement_failed.tolist() == [1, 1] and float(env.goal[..., :3].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ 5. "full" stays what it was
def _full_is_unchanged(lib, device, B):
    rows = []
    for extra in ({}, dict(rot_dist_type="full", randomize_goal_rot=False)):
        kw = dict(lib=lib, n_substeps=1) if lib is not None else {}
        env = BatchedBlockRearrangeEnv(B, device=device, stabilize_steps=2, n_random_initial_steps=1, settle_steps=2, max_timesteps_per_goal_per_obj=1, pipelined_reset=True,
                                       device_reset=True, starting_seed=11, **kw, **extra)
        env.reset()
        g = torch.Generator().manual_seed(3)
        out = []
        for _ in range(12):
            env.step((torch.rand((B, env.action_dim), generator=g) * 2 - 1).to(env.device))
            out.append(env.packed.clone())
        env.sync()
        rows.append(torch.stack(out).cpu())
    assert torch.equal(rows[0].view(torch.int32), rows[1].view(torch.int32))
    assert bool(torch.isfinite(rows[0]).all())


def test_full_rot_dist_is_bit_identical_emul(emul_lib):
    _full_is_unchanged(emul_lib, "cpu", 4)


@pytest.mark.gpu
def test_full_rot_dist_is_bit_identical_gpu():
    _full_is_unchanged(None, "cuda:0", 64)


# ------------------------------------------------------------------------------------------------ 6. physics of the domino world against the unchanged oracle
def test_dominos_world_step_matches_oracle_emul(emul_lib, oracle_lib):
    from tests.test_rearrange_env import _check_steps

    mk = lambda: dominos.make_simple_env(batch_size=2, device="cpu", lib=emul_lib, constants={"goal_args": {"rot_dist_type": "full"}}, starting_seed=3, **FAST)
    env = _check_steps(emul_lib, "cpu", B=2, n_substeps=1, nsteps=1, make=mk)
    assert env.N == 5 and abs(env.obj_half[0, 2] - 0.0254 * 1.5) < 5e-7


@pytest.mark.gpu
def test_dominos_world_step_matches_oracle_gpu(oracle_lib):
    """The domino world on rb_step_kernel against the unchanged OracleRearrangeEnv under test_rearrange_env.py's re-synchronised protocol and tolerances (rot_dist_type
    "full": the oracle's goal layer knows only that): B = 16, N = 5, 40 substeps, 6 steps, at least half the (step, env) pairs with the same contact history."""
    from tests.test_rearrange_env import _check_steps

    mk = lambda: dominos.make_simple_env(batch_size=16, device="cuda:0", constants={"goal_args": {"rot_dist_type": "full"}}, n_substeps=40, stabilize_steps=20,
                                         n_random_initial_steps=1, settle_steps=10, starting_seed=3)
    env = _check_steps(None, "cuda:0", B=16, n_substeps=40, nsteps=6, make=mk, min_same_fraction=0.5)
    assert env.N == 5 and env.rot_dist_type == "full"


# ------------------------------------------------------------------------------------------------ 7. through make_env
def _through_make_env(lib, device, B, nsteps, holdout, n_substeps=None):
    kw = dict(lib=lib, n_substeps=1) if lib is not None else {}
    env = dominos.make_env(batch_size=B, device=device, constants={"is_holdout": holdout, "max_timesteps_per_goal_per_obj": 5 if lib is None else 1}, pipelined_reset=True,
                           device_reset=True, starting_seed=2, **(dict(stabilize_steps=1, n_random_initial_steps=1, settle_steps=1) if lib is not None else dict(stabilize_steps=20, n_random_initial_steps=2, settle_steps=10)), **kw)
    assert env.wrapped and env.goal_kind == (6 if holdout else 5) and env.post.rot_dist_type == 2 and env.N == 5
    obs = env.reset()
    ref = blocks_train.make_env(batch_size=1, device=device, **_lib_args(lib))
    assert list(obs) == list(ref.reset())                                      # observation keys: blocks_train's
    g = torch.Generator(device=env.device); g.manual_seed(0)
    ends = torch.zeros((), dtype=torch.int64, device=env.device); starts = torch.zeros_like(ends)
    for _ in range(nsteps):
        idx = torch.randint(0, 11, env.action_shape, device=env.device, generator=g, dtype=torch.int32)
        obs, rew, done, info = env.step(idx)
        ends += done.sum(); starts += info["episode_started"].sum()
    env.sync()
    assert int(env.sim.status.max()) == 0 and int(env.solver_sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
    assert int(env.placement_failed.max()) == 0
    return env, int(ends), int(starts)


@pytest.mark.parametrize("holdout", [False, True])
def test_dominos_make_env_emul(emul_lib, holdout):
    env, ends, starts = _through_make_env(emul_lib, "cpu", 2, 6, holdout)
    assert ends >= 2      # (goal time-out after 5 steps)


@pytest.mark.gpu
@pytest.mark.parametrize("holdout", [False, True])
def test_dominos_make_env_gpu(holdout):
    env, ends, starts = _through_make_env(None, "cuda:0", 256, 120, holdout)
    assert ends >= 256 and starts >= 256, (ends, starts)      # (goal time-out after 25 steps, a 32-step recipe: every env ends and restarts at least once)


# ------------------------------------------------------------------------------------------------ 8. refusals and the surface
def test_dominos_surface_and_refusals_emul(emul_lib):
    kw = dict(batch_size=1, device="cpu", lib=emul_lib, **FAST)
    env = dominos.make_env(**kw)
    assert env.N == 5 and env.goal_kind == 5 and env.rot_dist_type == "mod180" and not env.randomize_goal_rot and env.domino_distance_mul == 4.0
    assert np.abs(env.obj_half - 0.0254 * np.array([1 / 1.5, 1, 1.5])[None]).max() <= 5e-7
    env = dominos.make_simple_env(parameters={"simulation_params": {"num_objects": 2, "domino_eccentricity": 2.5, "domino_distance_mul": 3}},
                                  constants={"is_holdout": True, "goal_args": {"rot_dist_type": "mod90", "randomize_goal_rot": True, "rot_randomize_type": "z_axis"}}, **kw)
    assert env.N == 2 and env.goal_kind == 6 and env.rot_dist_type == "mod90" and env.randomize_goal_rot and env.domino_distance_mul == 3.0 and not env.wrapped
    assert np.abs(env.obj_half - 0.0254 * np.array([1 / 2.5, 1, 2.5])[None]).max() <= 5e-7
    env = dominos.make_env(constants={"goal_args": {"pickup_proba": 0.3, "stacking_proba": 0.2, "height_range": (0.1, 0.2)}}, **kw)
    assert env.pickup_proba == 0.3 and env.stacking_proba == 0.2 and env.height_range == (0.1, 0.2) and env.rot_dist_type == "full"      # (a given goal_args replaces the default)
    for mod in (dominos, blocks, blocks_train):
        with pytest.raises(NotImplementedError, match="rot_dist_type"):
            mod.make_env(constants={"goal_args": {"rot_dist_type": "icp"}}, **kw)
        for kind in ("block", "full"):
            with pytest.raises(NotImplementedError, match="rot_randomize_type"):
                mod.make_env(constants={"goal_args": {"randomize_goal_rot": True, "rot_randomize_type": kind}}, **kw)
        with pytest.raises(NotImplementedError, match="stabilize_goal"):
            mod.make_env(constants={"goal_args": {"stabilize_goal": True}}, **kw)
        e = mod.make_env(constants={"goal_args": {"rot_dist_type": "mod90", "randomize_goal_rot": True}}, **kw)
        assert e.rot_dist_type == "mod90" and e.randomize_goal_rot and e.post.rot_dist_type == 1
    with pytest.raises(NotImplementedError, match="pickup_proba"):
        dominos.make_env(constants={"is_holdout": True, "goal_args": {"pickup_proba": 0.5}}, **kw)      # (the arc has no such argument)
    with pytest.raises(NotImplementedError, match="num_objects"):
        dominos.make_env(parameters={"simulation_params": {"num_objects": 3}}, **kw)
    with pytest.raises(NotImplementedError, match="rot_dist_type"):
        BatchedBlockRearrangeEnv(1, device="cpu", lib=emul_lib, rot_dist_type="icp", **FAST)


# ------------------------------------------------------------------------------------------------ 9. the goal arguments through the other task modules
@pytest.mark.parametrize("device_reset", [False, True])
def test_task_modules_take_the_goal_rotation_arguments_emul(emul_lib, device_reset):
    """`constants.goal_args` {rot_dist_type, randomize_goal_rot} reaches every env built through blocks.make_env: pick-and-place, stack and reach on the host recipe and on
    the device recipe -- tests/test_rearrange_tasks.py `_task_sequence`'s protocol (goal time-outs, a 1 + 1 + 1 step recipe); every goal keeps its task's properties for
    boxes turned by the GOAL yaws, which differ from the objects' own."""
    from robogym_amd.envs.rearrange import blocks_pickandplace, blocks_reach, blocks_stack
    from tests.test_rearrange_tasks import _check_goal_properties

    for mod, N in ((blocks_pickandplace, 1), (blocks_stack, 2), (blocks_reach, 1)):
        env = mod.make_simple_env(batch_size=2, device="cpu", lib=emul_lib, n_substeps=1, stabilize_steps=1, n_random_initial_steps=1, settle_steps=1,
                                  constants={"goal_args": {"rot_dist_type": "mod90", "randomize_goal_rot": True}, "max_timesteps_per_goal_per_obj": 2 if N == 1 else 1},
                                  pipelined_reset=True, device_reset=device_reset, starting_seed=11)
        assert env.N == N and env.post.rot_dist_type == 1 and env.randomize_goal_rot
        env.reset()
        starts = 0
        for _ in range(8):
            obs, rew, done, info = env.step(torch.zeros((2, env.action_dim)))
            assert int(env.sim.status.max()) == 0 and bool(torch.isfinite(env.packed).all())
            st = info["episode_started"]; starts += int(st.sum())
            if bool(st.any()):
                yaw = env.goal_rot[st][..., 2].numpy().astype(np.float64)
                qpos = env.sim.qpos[st].numpy().astype(np.float64)
                _check_goal_properties(env, env.goal[st][..., :3].numpy().astype(np.float64), yaw, qpos)
                yaw_obj = 2 * np.arctan2(qpos[:, [qa + 6 for qa in env.obj_q]], qpos[:, [qa + 3 for qa in env.obj_q]])
                assert np.abs(np.angle(np.exp(1j * (yaw - yaw_obj)))).min() > 1e-3
        assert starts >= 2 and (not device_reset or int(env.placement_failed.max()) == 0)
