"""rearrange/blocks on the MI355X (BASELINE.json configs[3]: UR16e + 2f-85 gripper, table contacts, num_objects = 5, batch 4096).

Host-side mirror of the reference's `BlockRearrangeEnv` (/root/reference/robogym/envs/rearrange/blocks.py:23-40 over
envs/rearrange/common/base.py `RearrangeEnv`), batched: `make_env` / `make_simple_env`, `step(actions[B, 6])`, `reset(mask)`, `observe()`.

`step` = THREE launches, no host synchronisation:
  1. `rb_batch_step_tcp`   the TCP solver's own world: sync to the main arm, forward, mocap target from the action, 40 x mj_step, main ctrl
                           (JointControlledTcpArm.set_position_control, robot/ur16e/mujoco/joint_controlled_tcp_arm.py:89-97)
  2. `rb_batch_step_ex`    the main world: 40 x mj_step + two state-less forwards, the last in full (sensors, final-state stage arrays)
                           (SimulationInterface.step + RobotEnv._observe_sync, simulation_interface.py:176-189, robot_env.py:672-688)
  3. `ra_env_post_step`    observation row, reward, done, goal distances, MultiGoalTracker, gripper hand-over to the solver world
                           (robogym_amd/csrc/ra_env_kernel.h)

Host work (numpy, outside the per-step path): the reset recipe's placement sampling (`place_objects_in_grid`, common/utils.py:719-829: a grid of
cells over the placement area, distinct random cells; restated for boxes, distribution-equivalent, not draw-for-draw) and goal sampling
(`ObjectStateGoal.next_goal`, goals/object_state.py:355-418: targets keep the objects' initial yaw, new grid placement).  The per-episode
"re-creation" of the simulation (common/base.py:850-856) is the same model with new object poses here: blocks have no per-episode shape
parameters at the default `object_scale_low/high = 0`, material `default`.

`control_mode = "joint"` (robot_interface.py:9-20, MujocoURJointGripperCompositeRobot = JointControlledArm + MujocoRobotiqGripper, composite/ur_gripper_arm.py): no TCP
solver world; `step(actions[B, 7])`, the action map (six arm joints relative to their positions, capped by max_position_change; the gripper relative to its control)
runs at the head of the main world's launch (rb_batch_set_action_limits) -- TWO launches per step.

`control_mode = "tcp+wrist"` (FreeWristTcpArm, free_dof_tcp_arm.py:238-246): `step(actions[B, 5])` = xyz, wrist, gripper; the solver world's launch ignores the roll number
and aligns the commanded orientation with the vertical (rb_tcp_args.wrist_only).

`tcp_solver_mode = "mocap"` (MujocoIdealURGripperCompositeRobot, composite/ur_gripper_arm.py:126-128): the main world's arm on the mocap weld, no joint actuators, no solver
world; the hook runs on the env's own world (rb_tcp_args.self_world) -- ONE physics launch per step.  Blocks, synchronous reset.

Duplicated-object groups (`object_groups`; the reference's `_randomize_object_groups` + the greedy matching of `ObjectStateGoal.relative_goal`) are opt-in here: the
default "distinct" keeps every object its own group, where the reference samples groups at every reset.

Per-env object counts (`max_num_objects`; the reference's `simulation_params.max_num_objects` with `num_objects` changing between episodes, simulation/base.py:68-74,
common/base.py:850-856, 919-927): the batch's world is the M-block world, env e uses its first `num_active[e]` blocks, `num_objects_next` is the device row a curriculum
writes, latched at every episode start; unused blocks are parked.

Masks of the placement area (`mask_obs_outside_placement_area`; the reference's `constants.mask_obs_outside_placement_area` with `goal_args.soft_mask` /
`mask_margin`, common/base.py:311-374, simulation/base.py:834-902, goals/object_state.py:373-378): opt-in; the env kernel appends `placement_mask`,
`goal_placement_mask` and the twelve `masked_*` keys to the packed row (MASK_OBS_KEYS), the goal's mask is written with the goal and stays until the next one
(DESIGN.md section 3.6c).

Per-env object subsets (`object_pool`): an env uses n of its world's M objects, drawn per env and per episode on the device (`object_perm`: slot -> world object; the
others parked) -- what lets one compiled mesh world serve 8!/(8-n)! ordered object sets.

Per-object materials (`material_names`; the reference's `RearrangeEnvParameters.material_names`, common/base.py:206-210, 575-585): every episode draws one of the
named materials (envs/rearrange/materials.py) per object -- per group with `object_groups` -- on the device and writes its density, friction, solref, solimp and
joint armature / damping into the env's parameter rows (`object_material`).  The default list, `["default"]`, is the compiled worlds' own material.

Not built for this env: vision, `teleport_to_goal`, per-group `material_args` dictionaries / colours / scales.
"""
import ctypes
import os
from typing import Optional

import numpy as np
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import materials
from robogym_amd.envs.rearrange.xml import load_blocks_model, load_solver_model, object_bounding_boxes
from robogym_amd.mujoco.large_simulation import LargeModelSimulation

TABLETOP_EXPERIMENT_INITIAL_POS = np.deg2rad(np.array([135.0, -90, 135, -100, -240, 135]))   # robot/ur16e/arm_interface.py:27
SPEED_ROLL, SPEED_PITCH = float(np.deg2rad(200)), float(np.deg2rad(600))                      # free_dof_tcp_arm.py:13-17
JOINT_DRIFT_THRESHOLD = float(np.deg2rad(1))
FLAG_FULL_FORWARD = _native.RG_FLAG_SENSORS      # on the large-model stepper: the last state-less forward in full, sensors read from it
#: the goal generators of the rearrange block tasks (ra_post_args.goal_kind): ObjectStateGoal (goals/object_state.py), PickAndPlaceGoal (goals/pickandplace.py),
#: ObjectStackGoal (goals/object_stack_goal.py), ObjectReachGoal / DeterministicReachGoal (goals/object_reach_goal.py)
#: (train: TrainStateGoal, goals/train_state.py; dominos: DominoStateGoal, goals/dominos.py; attached: AttachedBlockStateGoal, goals/attached_block_state.py; fixed:
#: ObjectFixedStateGoal, goals/object_state_fixed.py)
GOAL_KINDS = {"object_state": _native.RA_GOAL_OBJECT_STATE, "pickandplace": _native.RA_GOAL_PICKANDPLACE, "stack": _native.RA_GOAL_STACK, "reach": _native.RA_GOAL_REACH,
              "det-reach": _native.RA_GOAL_DET_REACH, "train": _native.RA_GOAL_TRAIN, "dominos": _native.RA_GOAL_DOMINOS, "attached": _native.RA_GOAL_ATTACHED,
              "fixed": _native.RA_GOAL_FIXED}
#: the reach goals: one object, which the goal itself moves; the target is a point above it
REACH_KINDS = ("reach", "det-reach")
#: the kinds whose generator sets the goals' yaws itself (set_target_quat inside _sample_next_goal_positions): the arc's / init_quats', whatever the goals had
OWN_YAW_KINDS = ("dominos", "attached", "fixed")
#: the kinds built for per-env object counts (max_num_objects)
COUNTED_KINDS = ("object_state", "pickandplace", "stack", "train")
#: the kinds built for per-env object subsets (object_pool)
POOL_KINDS = ("object_state", "pickandplace")
#: the kinds the post kernel knows by number (ra_post_args.goal_kind); the others differ in how a goal is made only and are scored as object_state
POST_KINDS = ("object_state", "pickandplace", "stack", "reach", "det-reach")
#: AttachedBlockStateGoal's cells (goals/attached_block_state.py:34-49), in steps of one block: a row of 2, a row of 4, a row of 2
ATTACHED_LATTICE = np.array([[1, 0], [2, 0], [0, 1], [1, 1], [2, 1], [3, 1], [1, 2], [2, 2]], dtype=np.float64)
#: GoalArgs.rot_dist_type (goals/object_state.py:127-131) -> ra_post_args.rot_dist_type; "icp": one more launch in front of the env kernel (ra_env_icp, csrc/ra_icp_kernel.h)
ROT_DIST_TYPES = {"full": _native.RA_ROT_FULL, "mod90": _native.RA_ROT_MOD90, "mod180": _native.RA_ROT_MOD180, "icp": _native.RA_ROT_ICP}
#: DominoStateGoal's attempts per goal (goals/dominos.py:10)
DOMINO_MAX_RETRY = 1000
#: DeterministicReachGoal's two object positions (goals/object_reach_goal.py:65-66)
DET_REACH_POINTS = np.array([[1.50253879, 0.36960144, 0.5170952], [1.32253879, 0.53960144, 0.5170952]])
#: lambda range of `sample_group_counts` (common/utils.py:47-49, the function's own defaults)
SAMPLE_LAM = (1.0, 8.0)

OBS_KEYS = [("obj_pos", "N3"), ("obj_rel_pos", "N3"), ("obj_vel_pos", "N3"), ("obj_rot", "N3"), ("obj_vel_rot", "N3"), ("robot_joint_pos", 6), ("gripper_pos", 3),
            ("gripper_velp", 3), ("gripper_controls", 1), ("gripper_qpos", 1), ("gripper_vel", 1), ("qpos", "nq"), ("qpos_goal", "nq"), ("goal_obj_pos", "N3"),
            ("goal_obj_rot", "N3"), ("is_goal_achieved", 1), ("rel_goal_obj_pos", "N3"), ("rel_goal_obj_rot", "N3"), ("obj_gripper_contact", "N2"), ("obj_bbox_size", "N3"),
            ("obj_colors", "N4"), ("safety_stop", 1), ("tcp_force", 3), ("tcp_torque", 3)]
#: what `mask_obs_outside_placement_area` appends to the row (common/base.py:311-374), in the env kernel's order: 38 N columns
MASK_OBS_KEYS = [("placement_mask", "N1"), ("goal_placement_mask", "N1"), ("masked_goal_obj_pos", "N3"), ("masked_goal_obj_rot", "N3"), ("masked_rel_goal_obj_pos", "N3"),
                 ("masked_rel_goal_obj_rot", "N3"), ("masked_obj_pos", "N3"), ("masked_obj_rot", "N3"), ("masked_obj_rel_pos", "N3"), ("masked_obj_vel_pos", "N3"),
                 ("masked_obj_vel_rot", "N3"), ("masked_obj_gripper_contact", "N2"), ("masked_obj_bbox_size", "N3"), ("masked_obj_colors", "N4")]
#: the third size of `get_placement_area` (simulation/base.py:1002)
PLACEMENT_AREA_HEIGHT = 0.26


def objects_in_placement_area(pos, lo, hi, margin=0.02, soft=False, u=None):
    """`check_objects_in_placement_area` (simulation/base.py:847-902) for points `pos` [.., 3] against the boundary `lo`, `hi` [3] (or [.., 1, 3] per env): max_dist =
    the largest of max(p - hi, lo - p, 0) over x, y, z; hard: max_dist < margin; soft: u > clip(max_dist / margin, 0, 1) with ONE `u` per env (a scalar, or [.., 1]).
    Host numpy, the goal's mask of the host route; ra_in_area (csrc/ra_env_kernel.h) is the same rule on the device.  -> bool [..]"""
    pos = np.asarray(pos, dtype=np.float64)
    max_dist = np.maximum(np.maximum(pos - hi, lo - pos), 0.0).max(-1)
    return (u > np.clip(max_dist / margin, 0.0, 1.0)) if soft else (max_dist < margin)


def euler2quat(e):
    """robogym/utils/rotation.py:110-126 convention: q = qx(e0) qy(e1) qz(e2) (pinned by tests/golden/rearrange_rotation.npz)"""
    e = np.asarray(e, dtype=np.float64)
    hx, hy, hz = 0.5 * e[..., 0], 0.5 * e[..., 1], 0.5 * e[..., 2]
    cx, sx, cy, sy, cz, sz = np.cos(hx), np.sin(hx), np.cos(hy), np.sin(hy), np.cos(hz), np.sin(hz)
    return np.stack([cx * cy * cz - sx * sy * sz, sx * cy * cz + cx * sy * sz, cx * sy * cz - sx * cy * sz, cx * cy * sz + sx * sy * cz], axis=-1)


def quat2mat(q):
    """robogym/utils/rotation.py quat2mat for quaternions (w, x, y, z) [.., 4] -> [.., 3, 3]"""
    q = np.asarray(q, dtype=np.float64)
    w, x, y, z = (q[..., k] for k in range(4))
    s = 2.0 / (q * q).sum(-1)
    rows = [[1.0 - s * (y * y + z * z), s * (x * y - w * z), s * (x * z + w * y)], [s * (x * y + w * z), 1.0 - s * (x * x + z * z), s * (y * z - w * x)],
            [s * (x * z - w * y), s * (y * z + w * x), 1.0 - s * (x * x + y * y)]]
    return np.stack([np.stack(r, -1) for r in rows], -2)


def mat2euler(mat):
    """robogym/utils/rotation.py mat2euler [.., 3, 3] -> [.., 3], with its gimbal branch below cos(pitch) = 4 eps"""
    mat = np.asarray(mat, dtype=np.float64)
    cy = np.sqrt(mat[..., 2, 2] ** 2 + mat[..., 1, 2] ** 2)
    free = cy > 4.0 * np.finfo(np.float64).eps
    return np.stack([np.where(free, -np.arctan2(mat[..., 1, 2], mat[..., 2, 2]), 0.0), -np.arctan2(-mat[..., 0, 2], cy),
                     np.where(free, -np.arctan2(mat[..., 0, 1], mat[..., 0, 0]), -np.arctan2(-mat[..., 1, 0], mat[..., 1, 1]))], -1)


def rotated_half(half, quat):
    """`rotate_bounding_box` as `get_block_bounding_box` calls it: half extents `half` [N, 3] of boxes turned by the unit quaternions `quat` [.., N, 4] -> the half
    extents of the turned boxes' bounding boxes [.., N, 3], sum_k |R_ik| half_k; `yawed_half` is this for rotations about z"""
    return np.einsum("...ik,...k->...i", np.abs(quat2mat(quat)), np.asarray(half, dtype=np.float64))


def load_state(state, num_objects, key="state"):
    """A recorded object state -- {"obj_pos": [M, 3], "obj_quat": [M, 4] (w, x, y, z)}, the reference's npz format (envs/rearrange/holdouts), or the path of such a
    file -- as [num_objects, 7] float64: the rows beyond `num_objects` cut off as the reference cuts them (holdout.py:98-103), the quaternions normalised.  `key`
    names the argument in the errors."""
    if isinstance(state, (str, os.PathLike)):
        with np.load(state) as f:
            state = {k: f[k] for k in ("obj_pos", "obj_quat")}
    if not (isinstance(state, dict) and "obj_pos" in state and "obj_quat" in state):
        raise ValueError("%s is not a state {\"obj_pos\": [N, 3], \"obj_quat\": [N, 4]} or the path of one" % key)
    pos, quat = np.asarray(state["obj_pos"], dtype=np.float64), np.asarray(state["obj_quat"], dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or quat.shape != (pos.shape[0], 4):
        raise ValueError("%s: obj_pos %r / obj_quat %r are not [N, 3] / [N, 4]" % (key, pos.shape, quat.shape))
    if pos.shape[0] < int(num_objects):
        raise ValueError("%s has %d rows, fewer than num_objects=%d" % (key, pos.shape[0], num_objects))
    pos, quat = pos[:int(num_objects)], quat[:int(num_objects)]
    norm = np.linalg.norm(quat, axis=-1, keepdims=True)
    if not (np.isfinite(pos).all() and np.isfinite(quat).all() and (norm > 1e-9).all()):
        raise ValueError("%s holds a position that is not finite or a zero quaternion" % key)
    return np.concatenate([pos, quat / norm], -1)


def _is_state(s):
    return isinstance(s, (str, os.PathLike, dict))


def sample_group_counts(random_state, total: int, lam_low: float = SAMPLE_LAM[0], lam_high: float = SAMPLE_LAM[1]):
    """`sample_group_counts` (common/utils.py:47-73), draw for draw: counts that sum to `total`; each round lam ~ U(lam_low, lam_high), then a count k in
    1..remaining with probability proportional to exp(-k lam)."""
    remaining, counts = int(total), []
    while remaining > 0:
        ks = np.arange(1, remaining + 1)
        lam = random_state.uniform(lam_low, lam_high)
        probs = np.exp(-ks * lam)
        probs /= probs.sum()
        k = int(random_state.choice(ks, p=probs))
        counts.append(k)
        remaining -= k
    return counts


def group_ids(counts):
    """counts -> the group id of each object: groups are contiguous ranges of object ids (common/base.py:536-547)"""
    return np.repeat(np.arange(len(counts)), counts).astype(np.int32)


def greedy_group_match(obj_pos, goal_pos, groups):
    """The goal each object is measured against (`ObjectStateGoal.relative_goal`, goals/object_state.py:520-554; host numpy, ra_group_match does the same on the
    device; the env itself never evaluates goal distances on the host -- this is the reference restatement for tests and for bindings that want one): inside each
    group of equal ids, n times the closest (object, goal) pair still free, ties to the lowest row-major index.  [N, 3], [N, 3], [N] -> [N]."""
    obj_pos, goal_pos, groups = np.asarray(obj_pos), np.asarray(goal_pos), np.asarray(groups)
    match = np.arange(len(groups))
    for g in np.unique(groups):
        ids = np.nonzero(groups == g)[0]
        dist = np.linalg.norm(obj_pos[ids][:, None, :] - goal_pos[ids][None, :, :], axis=-1)
        for _ in range(len(ids)):
            i, j = np.unravel_index(np.argmin(dist), dist.shape)
            match[ids[i]] = ids[j]
            dist[i, :] = np.inf
            dist[:, j] = np.inf
    return match


def yawed_half(half, yaw):
    """`rotate_bounding_box` for boxes turned about z: half extents `half` [N, 3], yaws [.., N] -> the half extents of the turned boxes' bounding boxes [.., N, 3]"""
    c, s_ = np.abs(np.cos(yaw)), np.abs(np.sin(yaw))
    return np.stack([c * half[:, 0] + s_ * half[:, 1], s_ * half[:, 0] + c * half[:, 1], np.broadcast_to(half[:, 2], np.shape(yaw))], -1)


def yawed_centre(centre, yaw):
    """bounding-box centres `centre` [N, 3] in the body frames, yaws [.., N] -> the centres from the body origins once the bodies are turned about z [.., N, 3]"""
    c, s_ = np.cos(yaw), np.sin(yaw)
    return np.stack([c * centre[:, 0] - s_ * centre[:, 1], s_ * centre[:, 0] + c * centre[:, 1], np.broadcast_to(centre[:, 2], np.shape(yaw))], -1)


def area_to_world(p, area_offset, table_pos, table_size):
    """points [.., 3] measured from the placement area's low corner on the table's bottom face -> world coordinates"""
    return p + [area_offset[0], area_offset[1], 0.0] - table_size + table_pos


def place_targets_with_goal_distance_ratio(random_state, centre, half, table_pos, table_size, area_offset, area_size, object_pos, goal_distance_ratio, goal_distance_min,
                                           max_trials=100, max_trials_per_object=20):
    """`place_targets_with_goal_distance_ratio` over `_place_objects` (common/utils.py:922-994, 623-716), draw for draw, for axis-aligned boxes (`centre`, `half` [N, 3]:
    each object's bounding box in its body frame, as yawed): per object a uniform proposal inside the area pulled toward the object's position, accepted when its box
    overlaps no goal placed before it.  Returns ([N, 3] body origins in world coordinates, valid); on failure the last proposals (the reference returns zeros)."""
    N = len(centre)
    table_pos, table_size = np.asarray(table_pos, dtype=np.float64), np.asarray(table_size, dtype=np.float64)
    shift = area_to_world(np.zeros(3), area_offset, table_pos, table_size)
    width, height = area_size[0], area_size[1]
    last = np.zeros((N, 3))
    for _ in range(max_trials):
        placed, valid = [], True
        for i in range(N):
            z = half[i, 2] + 2 * table_size[2] - centre[i, 2]
            trials = 0
            while True:
                gx, gy = random_state.uniform(low=(half[i, 0], half[i, 1]), high=(width - half[i, 0], height - half[i, 1]))
                place = object_pos[i] - shift
                x, y = place[0] + centre[i, 0], place[1] + centre[i, 1]
                dist = np.linalg.norm([gx - x, gy - y])
                ratio = np.clip(goal_distance_ratio, goal_distance_min / dist if dist >= goal_distance_min else 0.0, 1.0)
                gx, gy = x + (gx - x) * ratio, y + (gy - y) * ratio
                cand = np.array([gx - centre[i, 0], gy - centre[i, 1], z]) + shift
                last[i] = cand
                free = all(abs(cand[0] + centre[i, 0] - q[0] - centre[d, 0]) >= half[i, 0] + half[d, 0] or abs(cand[1] + centre[i, 1] - q[1] - centre[d, 1]) >= half[i, 1] + half[d, 1]
                           for d, q in enumerate(placed))
                if free:
                    break
                trials += 1
                if trials > max_trials_per_object:
                    valid = False
                    break
            if not valid:
                break
            placed.append(cand)
        if valid:
            return np.array(placed), True
    return last, False


def move_one_object_to_the_air_with_restrictions(random_state, placement, height_range, object_size, pickup_proba=0.0, stacking_proba=0.0, goal_distance_ratio=1.0):
    """goals/train_state.py:13-78, draw for draw up to the tower's members: nothing without probabilities; else one uniform p -- above their sum nothing, below
    `pickup_proba` one random object raised by U(height_range) * ratio, otherwise a tower of randint(2, N + 1) objects: the first of a random subset stays, the h-th other
    one gets its x, y and + object_size * (h + 1) * 2.  (The reference takes the subset from the global `np.random`; here it is `random_state`'s.)"""
    if pickup_proba + stacking_proba == 0:
        return placement
    p = random_state.random_sample()
    n = placement.shape[0]
    if p > pickup_proba + stacking_proba:
        return placement
    if p < pickup_proba:
        h = random_state.uniform(low=height_range[0], high=height_range[1])
        placement[random_state.randint(n), -1] += h * goal_distance_ratio
        return placement
    if n >= 2:
        tower = random_state.randint(2, n + 1)
        ids = random_state.permutation(n)[:tower]
        for h, i in enumerate(ids[1:]):
            placement[i, 0], placement[i, 1] = placement[ids[0], 0], placement[ids[0], 1]
            placement[i, 2] += object_size * (h + 1) * 2
    return placement


def randomize_yaw_along_z(random_state, yaw):
    """`randomize_quaternion_along_z` (goals/object_state.py:71-85) on yaw angles, draw for draw: one `uniform(0, 2 pi, size=N)`; the goal's new orientation is that z
    rotation times the one it has, i.e. the sum of the two yaws.  `yaw` [N] -> [N]."""
    yaw = np.asarray(yaw, dtype=np.float64)
    return yaw + random_state.uniform(low=0.0, high=2.0 * np.pi, size=yaw.shape[-1])


def domino_goal(random_state, obj_half, object_distance, table_pos, table_size, area_offset, area_size, max_retry=DOMINO_MAX_RETRY):
    """`DominoStateGoal._sample_next_goal_positions` (goals/dominos.py:20-150), draw for draw: per attempt offset = u pi and delta = u pi / 4 - pi / 8; domino k is turned
    by k delta + offset + delta / 2 about z and stands at the end of k steps of `object_distance` along (cos, sin)(j delta + offset), j = 1..k; the attempt is taken when the
    chain with the yawed half extents (`obj_half` [N, 3] at the identity orientation: boxes) is strictly smaller than the placement area, and then lands at a uniform
    offset inside what is left (two more draws).  Returns ([N, 3] body origins in world coordinates, [N] yaws, valid); after `max_retry` attempts zeros, the last
    attempt's yaws -- the reference leaves the targets turned by them -- and False."""
    obj_half = np.asarray(obj_half, dtype=np.float64)
    N = len(obj_half)
    table_pos, table_size = np.asarray(table_pos, dtype=np.float64), np.asarray(table_size, dtype=np.float64)
    width, height = area_size[0], area_size[1]
    ks = np.arange(N)
    yaws = np.zeros(N)
    for _ in range(max_retry):
        offset = random_state.random_sample() * np.pi
        delta = random_state.random_sample() * (np.pi / 4.0) - (np.pi / 8.0)
        yaws = ks * delta + (offset + delta / 2)
        between = (ks + 1) * delta + offset
        pos = np.zeros((N, 3))
        pos[1:, 0] = (np.cumsum(np.cos(between)) * object_distance)[:N - 1]
        pos[1:, 1] = (np.cumsum(np.sin(between)) * object_distance)[:N - 1]
        half = yawed_half(obj_half, yaws)
        pos[:, 2] = half[:, 2]
        max_x, max_y, _ = np.max(pos + half, axis=0)
        min_x, min_y, _ = np.min(pos - half, axis=0)
        size_x, size_y = max_x - min_x, max_y - min_y
        if size_x < width and size_y < height:
            dx = -min_x + random_state.random_sample() * (width - size_x)
            dy = -min_y + random_state.random_sample() * (height - size_y)
            start = table_pos - table_size
            return pos + [dx + start[0] + area_offset[0], dy + start[1] + area_offset[1], table_pos[2] + table_size[2]], yaws, True
    return np.zeros((N, 3)), yaws, False


def fixed_goal(relative_placements, obj_center, obj_half, table_pos, table_size, area_offset, area_size):
    """`place_targets_with_fixed_position` (common/utils.py:884-919) = `_place_objects_trial` (:653-716) with `run_collision_check=False`: object i's BODY ORIGIN at
    `relative_placements[i] * [width, height]` inside the placement area -- the proposal is not corrected by the bounding box's centre in x and y --, z from the box's
    half height and centre (`obj_center`, `obj_half` [N, 3]) on the table top.  Returns ([N, 3] body origins in world coordinates, True): always valid."""
    rel = np.asarray(relative_placements, dtype=np.float64)
    obj_center, obj_half = np.asarray(obj_center, dtype=np.float64), np.asarray(obj_half, dtype=np.float64)
    table_pos, table_size = np.asarray(table_pos, dtype=np.float64), np.asarray(table_size, dtype=np.float64)
    prop = rel * [area_size[0], area_size[1]]
    z = obj_half[:, 2] + 2 * table_size[2] - obj_center[:, 2]
    placement = np.concatenate([prop, z[:, None]], -1)
    return area_to_world(placement, area_offset, table_pos, table_size), True


def attached_goal(random_state, obj_center, obj_half, object_size, table_pos, table_size, area_offset, area_size):
    """`AttachedBlockStateGoal._sample_next_goal_positions` (goals/attached_block_state.py:17-68), draw for draw: a `permutation` of the eight lattice rows (block i
    goes to the i-th row of the result), one `uniform(low=(rel_w, rel_h), high=(margin_w, margin_h))` for the lattice's origin, then the fixed placement.  `object_size`
    is the blocks' HALF size; rel_w, rel_h = object_size / (width, height).  Returns ([8, 3], True)."""
    width, height = area_size[0], area_size[1]
    rel_w, rel_h = object_size / width, object_size / height
    block_config = random_state.permutation(ATTACHED_LATTICE * [rel_w * 2, rel_h * 2])
    config_w, config_h = block_config.max(axis=0)
    margin_w, margin_h = 1.0 - config_w - rel_w, 1.0 - config_h - rel_h
    ori_x, ori_y = random_state.uniform(low=(rel_w, rel_h), high=(margin_w, margin_h))
    block_config = block_config + np.array([[ori_x, ori_y]])
    return fixed_goal(block_config, obj_center, obj_half, table_pos, table_size, area_offset, area_size)


def z_rotation_yaws(init_quats, num_objects):
    """`init_quats` [N, 4] (w, x, y, z) of ObjectFixedStateGoal -> the yaw of each; the goal rows of this env hold rotations about z only: anything else raises."""
    if init_quats is None:
        return np.zeros(num_objects)
    q = np.asarray(init_quats, dtype=np.float64)
    if q.shape != (num_objects, 4):
        raise ValueError("init_quats has shape %r, not (%d, 4)" % (q.shape, num_objects))
    n = np.linalg.norm(q, axis=-1)
    if not np.all(np.abs(n - 1.0) < 1e-6) or np.abs(q[:, 1:3]).max() > 1e-9:
        raise NotImplementedError("init_quats: only unit quaternions of rotations about z are implemented by the batched rearrange env (the goal rows hold yaws), got %r" % (q.tolist(),))
    return 2.0 * np.arctan2(q[:, 3], q[:, 0])


def _parse_object_groups(object_groups, num_objects):
    """`object_groups` -> (mode, counts): "distinct" (None), "single", "sample" (counts drawn per env and episode), or explicit counts -- a list of ints or of the
    reference's `ObjectGroupConfig` fields as dicts, of which `count` alone is built."""
    if object_groups is None or (isinstance(object_groups, str) and object_groups == "distinct"):
        return "distinct", None
    if isinstance(object_groups, str):
        if object_groups == "single":
            return "fixed", [int(num_objects)]
        if object_groups == "sample":
            return "sample", None
        raise ValueError("object_groups %r is not \"distinct\", \"single\", \"sample\" or a list of counts" % (object_groups,))
    counts = []
    if len(object_groups) == 0:
        raise NotImplementedError("parameters.simulation_params.object_groups: an empty list is not implemented by the batched rearrange env (\"distinct\", \"single\", \"sample\" or counts)")
    for g in object_groups:
        if isinstance(g, dict):
            unset = lambda v: v is None or (isinstance(v, (dict, str, int, float)) and v in ({}, "default", 1, 1.0))      # (arrays, lists: a given value)
            other = sorted(k for k, v in g.items() if k not in ("count", "object_ids") and not unset(v))
            if other:
                raise NotImplementedError("object_groups: per-group %s not implemented by the batched rearrange env (count only)" % ", ".join(other))
            g = g.get("count", 1)
        counts.append(int(g))
    if min(counts, default=0) < 1 or sum(counts) != int(num_objects):
        raise ValueError("object_groups counts %r do not sum to num_objects=%d" % (counts, num_objects))
    return "fixed", counts


#: parking of the objects an env does not use (max_num_objects): cells PARK_SPACING apart in a grid PARK_COLUMNS wide, PARK_HEIGHT above the table's centre -- the
#: floor and table planes are that far below, the arm (reach about 1.3 m from its base), the camera rig and the backdrop (a 2 m half extent) stay more than 2 m away, so
#: the broadphase drops every pair of a parked block by its bounding sphere or its oriented box; |x| stays far below the 1e10 of RG_STATUS_BAD_STATE
PARK_SPACING, PARK_COLUMNS, PARK_HEIGHT = 0.5, 4, 6.0
#: the dof damping of a parked object (N s / m, N m s / rad; the Euler step treats damping implicitly, inv(M + h B): any value is stable)
PARK_DAMPING = 10.0


def _ptr(tensor):
    return ctypes.c_void_p(tensor.data_ptr())


def parking_poses(table_pos, num_objects):
    """[N, 7] (position, quaternion w x y z): slot i's parking cell, identity orientation"""
    i = np.arange(int(num_objects))
    out = np.zeros((len(i), 7))
    out[:, 0] = table_pos[0] + PARK_SPACING * (i % PARK_COLUMNS - 0.5 * (PARK_COLUMNS - 1))
    out[:, 1] = table_pos[1] + PARK_SPACING * (i // PARK_COLUMNS - 0.5 * (PARK_COLUMNS - 1))
    out[:, 2] = table_pos[2] + PARK_HEIGHT
    out[:, 3] = 1.0
    return out


def object_perm_rows(perm, M):
    """`set_object_perm_next`'s argument, checked, as int32 [M] or [R, M]: every row a permutation of 0..M-1 or all -1 (= sampled by the recipe kernel); `None` or -1:
    one row of -1.  Anything else raises ValueError."""
    if perm is None or (np.ndim(perm) == 0 and perm == -1):
        return np.full(M, -1, dtype=np.int32)
    c = np.asarray(perm)
    ok = c.ndim in (1, 2) and c.size > 0 and c.shape[-1] == M and c.dtype.kind in "iuf" and bool(np.all(c == np.round(c)))
    if ok:
        r = c.reshape(-1, M).astype(np.int64)
        ok = bool(np.all(np.all(r == -1, axis=1) | np.all(np.sort(r, axis=1) == np.arange(M), axis=1)))
    if not ok:
        raise ValueError("object_pool: object_perm_next %r is not a permutation of 0..%d per row (or a row of -1: sampled)" % (np.asarray(perm).tolist(), M - 1))
    return c.astype(np.int32)


class BatchedBlockRearrangeEnv:
    #: whether the class takes rot_dist_type "icp".  The block envs keep refusing it (boxes: mod90 / mod180 are their exact distances); the mesh envs of
    #: envs/rearrange/ycb.py, the same class on another model, switch it on
    ICP_ROT_DIST = False

    def __init__(self, batch_size: int, device="cuda:0", num_objects: int = 5, starting_seed: int = 0, max_position_change: float = 0.1,
                 arm_reset_controller_error: bool = True, n_random_initial_steps: int = 10, stabilize_steps: int = 100, settle_steps: int = 100,
                 success_threshold=None, penalty=None, max_timesteps_per_goal_per_obj: int = 200, successes_needed: int = 5, success_reward: float = 5.0,
                 use_goal_distance_reward: bool = True, goal_reward_per_object: float = 1.0, used_table_portion: float = 1.0, lib=None, n_substeps: int = 40,
                 main_model=None, wrappers: bool = False, n_action_bins: int = 11, smooth_alpha: float = 0.3, reward_clip: float = 100.0,
                 pipelined_reset: bool = False, action_spacing: str = "linear", per_env_parameters: bool = True, randomizer_params: Optional[dict] = None,
                 stabilize_object_damping: float = 1.0e-3, control_mode: str = "tcp+roll+yaw", device_reset: bool = False, tcp_solver_mode: str = "mocap_ik",
                 goal_kind: str = "object_state", height_range=(0.05, 0.25), object_size: float = 0.0254, fixed_order: bool = False, target_height: float = 0.1,
                 object_groups="distinct", sample_lam=SAMPLE_LAM, goal_distance_ratio=1.0, goal_distance_min: float = 0.06, pickup_proba: float = 0.0,
                 stacking_proba: float = 0.0, rot_dist_type: str = "full", randomize_goal_rot: bool = False, model=None, domino_distance_mul: float = 4.0,
                 relative_placements=None, init_quats=None, max_num_objects: Optional[int] = None, icp_max_num_vertices: int = 500, icp_error_threshold: float = 0.15,
                 icp_use_bbox_precheck: bool = False, mask_obs_outside_placement_area: bool = False, soft_mask: bool = False, mask_margin: float = 0.02, initial_states=None, goal_states=None,
                 advance_goals: bool = False, object_pool: bool = False, material_names=("default",)):
        """`per_env_parameters`: every env carries its own copy of the randomisable model fields (`self.sim.params`, LargeModelSimulation(env_params=True)) -- what
        the reference's simulation randomizers and `stabilize_objects` write into `sim.model`.  On by default (measured cost: 0.7 % of the step,
        profiles/r05_ab_rb_env_params.txt); off: the model's own arrays, no randomizers, no damping change while the objects stabilise.
        `device_reset`: with `pipelined_reset`, the recipe's stage machine, the begin-of-episode state and the placement / goal sampling run in ONE more launch after the
        env kernel (ra_env_recipe_step, include/rgstep.h) instead of host numpy behind a readback of the done / goal flags: a step call never waits for the GPU.  Without `pipelined_reset`, `step` is the plain step (finished envs stay done) and the synchronous
        `reset(mask)` / `reset_goals()` run that recipe on the device (`on_device`; `_reset_device`): the same kernel, the same draw streams, no readback of the mask.
        `randomizer_params`: name -> parameter of `build_simulation_randomizers` (the reference's ADR-controlled values; all zero by default = identity).
        `goal_kind` (GOAL_KINDS): the task's goal generator -- "object_state" (this env's own), "pickandplace" (`height_range`), "stack" (`object_size`, `fixed_order`),
        "reach" / "det-reach" (one object, `target_height`); envs/rearrange/blocks_pickandplace.py, blocks_stack.py, blocks_reach.py and ycb_pickandplace.py set it.
        `object_groups`: groups of interchangeable duplicates, matched to goals greedily by distance inside the env kernel (`self.obj_group` [B, N], ra_post_args.obj_group):
        "distinct" (default: no row, every object its own goal), "single" (one group; envs/rearrange/blocks_duplicate.py), "sample" (`sample_group_counts` with
        `sample_lam` per env at every episode start, host recipe and device recipe alike) or explicit counts that sum to `num_objects`.
        goal_kind "train" (envs/rearrange/blocks_train.py): `goal_distance_ratio` (a scalar or [B]: `self.goal_distance_ratio`, a device row a curriculum may write per
        env), `goal_distance_min`, `pickup_proba`, `stacking_proba`, with `height_range` and `object_size`.
        `rot_dist_type` (GoalArgs, goals/object_state.py:127-131): "full" (default), "mod90" or "mod180" -- the rotation distance of the env kernel
        (ra_post_args.rot_dist_type; the tables of parallel quaternions are device tensors built from utils/rotation.py) -- or, in a subclass that sets `ICP_ROT_DIST`
        (BatchedYcbRearrangeEnv; this class itself refuses it), "icp": the objects' point clouds are made
        from the model once (envs/rearrange/icp.py object_point_clouds with `icp_max_num_vertices`, `icp_error_threshold`; `self.icp_clouds`, device tensors) and
        `ra_env_icp` runs in front of EVERY launch of the env kernel, one ICP per (env, object), writing `self.icp_rel` [B, N, 3], which the env kernel reads
        (ra_post_args.icp_rel).  `icp_use_bbox_precheck` is accepted and has NO effect: in the reference both "bounding_box" entries the precheck compares are the TARGET's
        box (goals/object_state.py:420-425 and 483-488), so its IoU is 1 and the ICP always runs.  Not with the reach goals (their achieved rotation is zero).  With any
        other `rot_dist_type` there is no launch and no allocation for it.  `randomize_goal_rot`: every goal's yaw is the
        previous one plus U(0, 2 pi) per object (`rot_randomize_type` "z_axis"), its placement made with the boxes turned by the new yaws.
        `model`: a compiled main world in place of `load_blocks_model(num_objects)` (envs/rearrange/dominos.py: the domino world); goal_kind "dominos" places the goals on a
        circle arc, `object_size * domino_distance_mul` apart, with per-object goal yaws (DominoStateGoal).
        goal_kind "fixed" (ObjectFixedStateGoal): `relative_placements` [N, 2] in [0, 1], each object's body origin relative to the placement area, and `init_quats` [N, 4],
        the goals' orientations (rotations about z; default identity) -- the same goal every time.  goal_kind "attached" (envs/rearrange/blocks_attached.py,
        AttachedBlockStateGoal): eight blocks, `object_size` apart from their neighbours' faces, in a 2-4-2 lattice with a random assignment and a random origin.  Both set the
        goal's orientation themselves: `randomize_goal_rot` has no effect on them, as in the reference.
        `max_num_objects` = M (`simulation_params.max_num_objects`, simulation/base.py:73-74): per-env object counts.  The batch's world is the M-block world, env e uses
        its first `self.num_active[e]` <= M objects and `num_objects` is every env's first count.  `self.num_objects_next` (int32 [B], a device row a curriculum may write
        per env; `set_num_objects_next` is the checked host setter) is latched into `num_active` when that env's episode begins -- reset(mask), the host recipe and the
        device recipe alike; values outside 1..M are clamped.  Every per-object observation key keeps [B, M, ...] with zeros in the unused slots; distances, success, off-table
        test, finger contacts, group matching, time-out (`max_timesteps_per_goal_per_obj * n`), placements and the placement area (`placement_area(n)`) follow the env's
        count.  An unused object is parked at `self.park_pose[i]`, its weight cancelled through the env's `xfrc_applied` row and its dof damping raised
        (`_apply_parking`); rb_step_kernel steps it like any other body.  Goal kinds object_state, pickandplace, stack and train; object_groups
        "distinct" / "single" / "sample".
        `mask_obs_outside_placement_area` (the reference's constant of that name; `soft_mask`, `mask_margin`: GoalArgs): the env kernel appends `placement_mask` and
        `goal_placement_mask` [B, N, 1] and a `masked_` copy of the twelve per-object keys, zero for objects (goals) outside the placement area, to every observation it
        writes (MASK_OBS_KEYS; `obs_dim` = 74 N + 23 + 2 nq).  Outside: max over x, y, z of the distance to the area's box (`placement_area_boundary`, of the env's own
        object count) >= `mask_margin`; with `soft_mask` inside with probability 1 - clip(distance / margin, 0, 1), one draw per env and step shared by its objects.  The
        goal's mask (`self.goal_in_area` [B, N] floats; `goal_objects_in_placement_area`, `goal_in_placement_area`) is made with the goal -- ra_recipe_kernel or
        `_write_goal` -- and keeps its value until the next goal; unused slots read 1.  Off (default): no row, no pointer, no draw, the 24 keys.
        Recorded scenes (the reference's holdout envs, envs/rearrange/holdout.py and goals/holdout_object_state.py, as arrays).  A state is
        {"obj_pos": [M, 3], "obj_quat": [M, 4]} or the path of such an npz file (`load_state`: rows beyond `num_objects` cut off, quaternions normalised).
        `initial_states`: one state or a list of S states -- every episode of env e starts from state `self.scene[e]` instead of a drawn placement: position and full
        quaternion into qpos, `obj_bbox_size` the box turned by that rotation, no colour drawn (the rows keep (0, 0, 0, 1)); the rest of the recipe as it is.
        `goal_states`: a list of states (the goals of every scene) or one such list per scene (an empty list: that scene's goals are sampled) -- every goal of an env
        whose scene has goals is a recorded state: `goal` = its position and quaternion, `goal_rot` = the normalised mat2euler of it, `qpos_goal` carries
        euler2quat(goal_rot); `randomize_goal_rot` does not turn it.  `advance_goals` False (default): every goal is the scene's state 0, which is what the
        reference's code does; True: the goals run 0, 1, .. and wrap, from 0 again at every episode start (`self.goal_cursor`).  `self.scene_next` (int32 [B], a device
        row; `set_scene_next` is the checked host setter; env e starts with scene e mod S) is latched into `self.scene` when that env's episode begins, on the host
        route and the device route alike, which read the same tables and agree bit for bit.  A goal sampled after a recorded start begins from yaw 0: the
        reference's holdout reset sets the objects, not the targets.  `success_threshold` may name `rel_dist` (HoldoutObjectStateGoal.goal_distance: each object's
        distance from where the goal puts it relative to the object with the lowest goal z): `self.rel_dist` [B, N] and `info()["goal_dist"]["rel_dist"]` exist
        whenever there are no duplicate groups, and with the threshold an object counts as achieved only below it too.  Block worlds, goal_kind object_state, no
        `max_num_objects`.
        `object_pool`: every env uses a SUBSET of its world's M objects, drawn per env and per episode -- `num_objects` = n objects, the same
        count for the whole batch, out of the M of the world (`model` / `main_model`; without one the n-block world, M = n).  `self.object_perm` (int32 [B, M], a
        permutation of 0..M-1 per env) says which: observation / goal slot i of env e is world object `object_perm[e, i]`, slots i < n are in use, the world objects of
        the other slots are parked at their own `park_pose` as `max_num_objects` parks unused blocks.  `self.object_perm_next` ([B, M]; `set_object_perm_next` is the
        checked host setter) is latched when an env's episode begins; a row of -1 (the default) asks the recipe kernel to SAMPLE a permutation (Fisher-Yates, a draw
        stream of its own), without replacement inside the world's pool.  `object_set()` -> [B, n] world indices (a readback).  `observe()` / `step()` / `reset()`
        return every per-object key with n slots, the reference's shapes for `num_objects` = n; `qpos` / `qpos_goal` keep the world's nq, and `self.packed` keeps the
        world's width, M slots per key with zeros behind the n in use.  Needs `device_reset=True` (pipelined, or the synchronous `reset(mask)` / `reset_goals()`, which
        then run on the device by default; the host route refuses) and per-env parameter rows; goal kinds object_state and pickandplace, object_groups "distinct", no
        recorded scenes, no `max_num_objects`, no mocap arm.
        `material_names`: the materials an object may have, with multiplicity (`None` or an empty list: all five of
        envs/rearrange/materials.py).  A list of nothing but "default" (the default) is the compiled worlds' own material: no row, no pointer, no stage.  Any other
        list: where an env's episode ends, ra_param_rows_kernel draws one material per slot (per group with `object_groups`; a stream of its own) or takes the
        pin `self.object_material_next` ([B, N] int32 indices into materials.MATERIAL_NAMES, -1 = drawn; `set_object_material_next` is the checked host setter; read
        at every episode start, never cleared), writes `self.object_material` ([B, N] int32, device) and the material's rows on top of the restored block: the
        friction / solref / solimp of the object's geoms, body mass and inertia times density / 1000, the six dofs' armature and both `_invweight0` rows;
        `stabilize_objects` restores the material's damping.  The randomizers of geom_friction, geom_solref, geom_solimp, body_mass and body_inertia then start from
        the env's rows as they stand (block + material) instead of the model's.  Needs per-env parameter rows and `device_reset=True` (the host route refuses)."""
        self.B, self.N = int(batch_size), int(num_objects)
        self.material_names = materials.material_list(material_names)
        self.materials_on = not materials.is_default_only(self.material_names)
        if self.materials_on:
            if not per_env_parameters:
                raise ValueError("material_names=%r needs per_env_parameters=True (a material is written into the env's parameter rows)" % (self.material_names,))
            if not device_reset:
                raise NotImplementedError("material_names=%r needs device_reset=True: the materials are drawn and written by the device route's parameter-row launch; the host "
                                          "reset route is not built for them" % (self.material_names,))
            if len(self.material_names) > _native.RA_MAT_MAXCHOICE:
                raise ValueError("material_names: %d entries, at most %d (multiplicity is weight)" % (len(self.material_names), _native.RA_MAT_MAXCHOICE))
        if (initial_states is not None or goal_states is not None) and max_num_objects is not None:
            raise NotImplementedError("max_num_objects (per-env object counts) is not implemented together with initial_states / goal_states (recorded scenes) by the batched rearrange env")
        if (initial_states is not None or goal_states is not None) and (model is not None or main_model is not None or self.ICP_ROT_DIST):
            raise NotImplementedError("initial_states / goal_states (recorded scenes) are built for the block worlds of load_blocks_model, not for the ycb or domino worlds")
        self.mask_obs, self.soft_mask, self.mask_margin = bool(mask_obs_outside_placement_area), bool(soft_mask), float(mask_margin)
        if self.soft_mask and not self.mask_margin > 0:
            raise ValueError("soft_mask=True needs mask_margin > 0 (the probability is clip(distance / mask_margin, 0, 1)), got mask_margin=%r" % (mask_margin,))
        self.max_num_objects = None if max_num_objects is None else int(max_num_objects)
        if self.max_num_objects is not None:
            M = self.max_num_objects
            refuse = lambda what: NotImplementedError("max_num_objects (per-env object counts) is not implemented for %s by the batched rearrange env" % what)
            if goal_kind not in COUNTED_KINDS:
                raise refuse("goal_kind %r (%s)" % (goal_kind, ", ".join(COUNTED_KINDS)))
            if not (object_groups is None or (isinstance(object_groups, str) and object_groups in ("distinct", "single", "sample"))):
                raise refuse("explicit object_groups counts %r (\"distinct\", \"single\", \"sample\")" % (object_groups,))
            if _solver_mode_name(tcp_solver_mode) == "mocap" and _control_mode_name(control_mode) != "joint":
                raise refuse("tcp_solver_mode=\"mocap\"")
            if model is not None or main_model is not None:
                raise refuse("a world other than load_blocks_model (dominos, ycb)")
            if not per_env_parameters:
                raise refuse("per_env_parameters=False (an unused object is held by its env's xfrc_applied and dof_damping rows)")
            if not 1 <= M <= _native.RA_MAXOBJ:
                raise ValueError("max_num_objects=%d is outside 1..%d" % (M, _native.RA_MAXOBJ))
            if not 1 <= self.N <= M:
                raise ValueError("num_objects=%d is outside 1..max_num_objects=%d" % (self.N, M))
            self.num_objects_initial, self.N = self.N, M            # (self.N: the world's count, the width of every per-object array)
        self.object_pool = bool(object_pool)
        if self.object_pool:
            refuse = lambda what: NotImplementedError("object_pool (per-env object subsets) is not implemented for %s by the batched rearrange env" % what)
            if max_num_objects is not None:
                raise refuse("max_num_objects (per-env object counts: with the pool `num_objects` is the count of the whole batch)")
            if initial_states is not None or goal_states is not None:
                raise refuse("initial_states / goal_states (a recorded scene names the world's objects)")
            if goal_kind not in POOL_KINDS:
                raise refuse("goal_kind %r (%s)" % (goal_kind, ", ".join(POOL_KINDS)))
            if not (object_groups is None or (isinstance(object_groups, str) and object_groups == "distinct")):
                raise refuse("object_groups %r (\"distinct\")" % (object_groups,))
            if _solver_mode_name(tcp_solver_mode) == "mocap" and _control_mode_name(control_mode) != "joint":
                raise refuse("tcp_solver_mode=\"mocap\"")
            if not per_env_parameters:
                raise refuse("per_env_parameters=False (a parked object is held by its env's xfrc_applied and dof_damping rows)")
            if not device_reset:
                raise refuse("device_reset=False (the permutation is latched and sampled by the recipe kernel; the host reset route has no twin of it)")
            world = model if model is not None else main_model
            M = self.N if world is None else sum(1 for i in range(_native.RA_MAXOBJ + 1) if "object%d:joint" % i in world.names["joint"])
            if not 1 <= M <= _native.RA_MAXOBJ:
                raise ValueError("object_pool: the world has %d objects, outside 1..%d" % (M, _native.RA_MAXOBJ))
            if not 1 <= self.N <= M:
                raise ValueError("object_pool: num_objects=%d is outside 1..%d, the world's object count" % (self.N, M))
            # (the rows and launches of per-env object counts carry the pool: `num_active` holds n for every env, self.N is the world's count)
            self.num_objects_initial, self.N, self.max_num_objects = self.N, M, M
        if goal_kind not in GOAL_KINDS:
            raise ValueError("goal_kind %r is not one of %s" % (goal_kind, ", ".join(GOAL_KINDS)))
        self.goal_kind_name, self.goal_kind = goal_kind, GOAL_KINDS[goal_kind]
        if rot_dist_type not in ROT_DIST_TYPES:
            raise ValueError("rot_dist_type %r is not one of %s" % (rot_dist_type, ", ".join(ROT_DIST_TYPES)))
        self.rot_dist_type, self.randomize_goal_rot, self.domino_distance_mul = rot_dist_type, bool(randomize_goal_rot), float(domino_distance_mul)
        if goal_kind == "dominos" and not (float(object_size) > 0 and self.domino_distance_mul > 0):
            raise ValueError("goal_kind dominos needs object_size > 0 and domino_distance_mul > 0 (got %r, %r)" % (object_size, domino_distance_mul))
        if goal_kind == "attached" and not (self.N == 8 and float(object_size) > 0):
            raise ValueError("goal_kind attached needs num_objects == 8 and object_size > 0 (got %r, %r)" % (num_objects, object_size))
        if (relative_placements is not None or init_quats is not None) and goal_kind != "fixed":
            raise ValueError("relative_placements / init_quats belong to goal_kind \"fixed\" (ObjectFixedStateGoal), not to %r" % (goal_kind,))
        self.relative_placements, self.init_yaw = None, np.zeros(self.N)
        if goal_kind == "fixed":
            if relative_placements is None:
                raise ValueError("goal_kind fixed needs relative_placements [N, 2]")
            self.relative_placements = np.array(relative_placements, dtype=np.float64)
            if self.relative_placements.shape != (self.N, 2) or not np.all((self.relative_placements >= 0.0) & (self.relative_placements <= 1.0)):
                raise ValueError("relative_placements must be [%d, 2] with every entry in [0, 1], got %r" % (self.N, np.asarray(relative_placements).tolist()))
            self.init_yaw = z_rotation_yaws(init_quats, self.N)
        self.reach = goal_kind in REACH_KINDS
        if rot_dist_type == "icp" and not self.ICP_ROT_DIST:
            raise NotImplementedError("rot_dist_type \"icp\" is built for the mesh worlds (envs/rearrange/ycb.py BatchedYcbRearrangeEnv), not for the block envs "
                                      "(full, mod90, mod180: a box's symmetries are what mod90 / mod180 state exactly)")
        if rot_dist_type == "icp" and self.reach:
            raise NotImplementedError("rot_dist_type \"icp\" with goal_kind %r: the reach goals' achieved rotation is zero, there is no object cloud to fit (full, mod90, mod180)" % (goal_kind,))
        self.icp_max_num_vertices, self.icp_error_threshold, self.icp_use_bbox_precheck = int(icp_max_num_vertices), float(icp_error_threshold), bool(icp_use_bbox_precheck)
        self.goal_distance_min, self.pickup_proba, self.stacking_proba = float(goal_distance_min), float(pickup_proba), float(stacking_proba)
        if not (self.goal_distance_min >= 0 and self.pickup_proba >= 0 and self.stacking_proba >= 0 and self.pickup_proba + self.stacking_proba <= 1.0):
            raise ValueError("goal_distance_min >= 0 and 0 <= pickup_proba + stacking_proba <= 1 (got %r, %r, %r)" % (goal_distance_min, pickup_proba, stacking_proba))
        if self.reach and self.N != 1:
            raise ValueError("the reach goals take exactly one object (ObjectReachGoal: \"reach only supports one objects\"), got num_objects=%d" % self.N)
        self.height_range, self.object_size, self.fixed_order, self.target_height = (float(height_range[0]), float(height_range[1])), float(object_size), bool(fixed_order), float(target_height)
        if not self.height_range[0] <= self.height_range[1]:
            raise ValueError("height_range %r is empty" % (height_range,))
        self.group_mode, self.group_counts = _parse_object_groups(object_groups, self.N)
        self.sample_lam = (float(sample_lam[0]), float(sample_lam[1]))
        if self.group_mode != "distinct" and self.reach:
            raise ValueError("object_groups with a reach goal: one object, nothing to match")
        if not 0.0 <= self.sample_lam[0] <= self.sample_lam[1]:
            raise ValueError("sample_lam %r is not a range of non-negative rates" % (sample_lam,))
        self._L = lib if lib is not None else _native.lib()
        self.control_mode = _control_mode_name(control_mode)
        self.joint_control = self.control_mode == "joint"      # ControlMode.JOINT: no TCP solver world (RobotControlParameters.requires_solver_sim, robot_interface.py:83-91)
        self.wrist_only = self.control_mode == "tcp+wrist"      # ControlMode.TCP_WRIST: FreeWristTcpArm in the solver world, 4 arm numbers + the gripper's
        AD = 7 if self.joint_control else 6                     # the launches' action width (tcp+wrist: the six of tcp+roll+yaw with the roll number ignored)
        self.action_dim = 5 if self.wrist_only else AD          # the env's action width
        self.launch_action_dim = AD
        self.max_position_change = float(max_position_change)
        if model is not None and main_model is not None:
            raise ValueError("model and main_model name the same thing: pass one")
        if goal_kind == "dominos" and model is None and main_model is None:
            raise ValueError("goal_kind \"dominos\" is DominoStateGoal, the goal generator of the domino world only (goals/dominos.py:13-17): pass model=load_dominos_model(...), "
                             "as envs/rearrange/dominos.py make_env does")
        main_model = model if model is not None else main_model
        main = main_model if main_model is not None else load_blocks_model(self.N)   # (main_model: the same world with other objects, envs/rearrange/ycb.py)
        # TcpSolverMode.MOCAP (robot_interface.py:22-29): the MAIN world's arm hangs on the mocap weld itself -- MujocoIdealURGripperCompositeRobot, one world, no joint actuators
        self.tcp_solver_mode = _solver_mode_name(tcp_solver_mode)
        self.ideal_arm = self.tcp_solver_mode == "mocap" and not self.joint_control
        if self.ideal_arm:
            if main_model is not None:
                raise NotImplementedError("tcp_solver_mode mocap is built for the blocks world (its mocap-arm model is shipped; the ycb sets are compiled with joint actuators)")
            if pipelined_reset or device_reset:
                raise NotImplementedError("tcp_solver_mode mocap with pipelined resets: the synchronous reset() only (the reference's sim initialisation steps the world before the recipe)")
            main = load_blocks_model(self.N, mocap_arm=True)
        solver = None if (self.joint_control or self.ideal_arm) else load_solver_model()
        self.randomizer_params = dict(randomizer_params or {})
        self.per_env_parameters = bool(per_env_parameters)
        if self.randomizer_params and not self.per_env_parameters:
            raise ValueError("randomizer_params need per_env_parameters=True")
        self.sim = LargeModelSimulation(main, self.B, device=device, n_substeps=n_substeps, lib=lib, hand=False, env_params=self.per_env_parameters)
        self.solver_sim = None if solver is None else LargeModelSimulation(solver, self.B, device=device, n_substeps=n_substeps, lib=lib, hand=False)
        self.device = self.sim.device
        self._ext_cols = torch.tensor([0, 1, 2, 4, 5], device=self.device) if self.wrist_only else None      # tcp+wrist: the launch's columns without the roll
        self.model, self.solver_model = main, solver
        self.n_random_initial_steps, self.stabilize_steps, self.settle_steps = n_random_initial_steps, stabilize_steps, settle_steps
        self.used_table_portion = used_table_portion
        self._rng = np.random.RandomState(starting_seed)
        self.host_placement_failed = 0      # host recipe: goal placements that ran out of restarts (the device recipe counts per env in `placement_failed`)
        A, jn = main.arrays, main.names["joint"]
        self.arm_q = [int(A["jnt_qposadr"][jn.index("robot0:J%d" % k)]) for k in range(1, 7)]
        self.obj_q = [int(A["jnt_qposadr"][jn.index("object%d:joint" % i)]) for i in range(self.N)]
        self.obj_v = [int(A["jnt_dofadr"][jn.index("object%d:joint" % i)]) for i in range(self.N)]
        self.grip_q = int(A["jnt_qposadr"][jn.index("robot0:r_gripper_RJ0_outer")])
        self.grip_act = main.names["actuator"].index("robot0:r_gripper_finger_joint")
        self.nq, self.nu = self.sim.nq, self.sim.nu
        self.base_obs_dim = 36 * self.N + 23 + 2 * self.nq
        self.obs_dim = self.base_obs_dim + (38 * self.N if self.mask_obs else 0)
        self.obs_keys = OBS_KEYS + (MASK_OBS_KEYS if self.mask_obs else [])
        tb, tg = main.name2id("body", "table"), main.names["geom"].index("table")
        self.table_pos, self.table_size = A["body_pos"][tb].copy(), A["geom_size"][tg].copy()
        self.table_height = float(self.table_pos[2] + self.table_size[2])
        bb = object_bounding_boxes(main, self.N)                        # per object: centre and half extents of its vertices in the body frame
        self.obj_center, self.obj_half = bb[:, :3].copy(), bb[:, 3:].copy()
        # ---- env-level state (device)
        dev, B, N = self.device, self.B, self.N
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
        self.packed = z(B, self.obs_dim + 4)
        self.t, self.steps, self.ssl, self.successes, self.consecutive = (z(B, dt=torch.int32) for _ in range(5))
        self.prev_nsucc, self.prev_valid = z(B), z(B, dt=torch.int32)
        self.goal, self.goal_rot, self.qpos_goal, self.static_obs = z(B, N, 7), z(B, N, 3), z(B, self.nq), z(B, N, 7)
        self.reward, self.goal_dist, self.goal_dist_extra = z(B, 3), z(B, 2), z(B, 2)
        self.goal_index = z(B, dt=torch.int32)                  # DeterministicReachGoal.idx, per env
        self.goal_distance_ratio = torch.as_tensor(np.broadcast_to(np.asarray(goal_distance_ratio, dtype=np.float32), (B,)).copy(), device=dev)      # per env (train)
        self.done, self.goal_reset, self.trial_success, self.sub_goal_ok, self.env_crash, self.objects_off_table = (z(B, dt=torch.bool) for _ in range(6))
        self.info_ssl = z(B, dt=torch.int32)
        self.goal[:, :, 3] = 1.0
        self.goal_in_area = torch.ones(B, N, dtype=torch.float32, device=dev) if self.mask_obs else None      # (until the first goal is made: as the padded slots)
        self._mask_step = 0           # ra_post_args.step: + 1 per step() / reset(); the re-observations in between carry the same value
        self.obj_group = None
        if self.group_mode != "distinct":      # ("sample": all distinct until the first reset draws the rows)
            ids = group_ids(self.group_counts if self.group_mode == "fixed" else [1] * N)
            self.obj_group = torch.tensor(np.tile(ids, (B, 1)), dtype=torch.int32, device=dev).contiguous()
        # per-env object counts (max_num_objects): the latched counts, the row a curriculum writes, where an unused object is parked
        self.num_active = self.num_objects_next = self.park_pose = None
        if self.max_num_objects is not None:
            self.num_active = torch.full((B,), self.num_objects_initial, dtype=torch.int32, device=dev)
            self.num_objects_next = self.num_active.clone()
            self.park_pose = parking_poses(self.table_pos, N)
            self._obj_bodies = torch.tensor([main.name2id("body", "object%d" % i) for i in range(N)], device=dev, dtype=torch.long)
            self._slot = torch.arange(N, device=dev, dtype=torch.int32)
        # per-env object subsets (object_pool): slot -> world object of the running episode, and the row the next episode latches (-1: sampled by the recipe kernel)
        self.object_material = self.object_material_next = None      # per-object materials: made with the parameter-row launch's arguments (_fill_material_args)
        self.object_perm = self.object_perm_next = None
        if self.object_pool:
            self.object_perm = torch.arange(N, dtype=torch.int32, device=dev).repeat(B, 1).contiguous()
            self.object_perm_next = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        # pipelined resets: an env whose episode ended runs the reset recipe INSIDE the following step calls (the stepper's launches take everybody
        # along; a synchronous reset of a few envs costs ~210 launch pairs at the latency of a full batch).  The recipe's bookkeeping is host numpy (one
        # readback of the flags per step -- a step is 70 ms of GPU work), its physics goes through the same three launches as the live envs': `hold` /
        # `scripted` feed the recipe's actions to the solver world's launch, `frozen` keeps the env kernel from scoring those envs.
        self.pipelined = bool(pipelined_reset)
        self._stage, self._left = np.zeros(B, dtype=np.int8), np.zeros(B, dtype=np.int32)      # _native.RA_STAGE_*
        self._yaw = np.zeros((B, N))
        self.ended_rows = np.zeros(0, dtype=np.int64)          # rows whose episode ended on the last step (pipelined resets)
        self.hold, self.scripted, self.frozen, self.solver_active = z(B, dt=torch.int32), z(B, AD), z(B, dt=torch.uint8), torch.ones(B, dtype=torch.int32, device=dev)
        self.hold_ctrl = z(B, dt=torch.int32)      # joint control, pipelined resets: envs whose objects stabilise keep their stored controls (no action reaches the robot)
        self.resetting, self.episode_started = z(B, dt=torch.bool), z(B, dt=torch.bool)
        self.nticks = torch.full((B,), 2, dtype=torch.int32, device=dev)       # state-less forwards (controller ticks) per env of the main world's launch
        self.wrapped = bool(wrappers)
        self._fill_scenes(initial_states, goal_states, advance_goals)
        # ---- the arguments of the TCP hook, the env kernel and, for rot_dist_type icp, the launch in front of it
        self._fill_tcp_args(max_position_change, arm_reset_controller_error)
        st = dict(success_threshold or {"obj_pos": 0.04, "obj_rot": 0.2})
        if "rel_dist" in st and self.group_mode != "distinct":
            raise ValueError("success_threshold names rel_dist together with object_groups=%r: the relative distance is defined for distinct objects only "
                             "(goals/holdout_object_state.py:67-69)" % (object_groups,))
        if "rel_dist" in st and self.reach:
            raise ValueError("success_threshold names rel_dist with a reach goal (one object, measured at the grip site)")
        # (HoldoutObjectStateGoal.goal_distance: rel_dist whenever every object is its own group; here: where the threshold or a recorded scene asks for it)
        self.rel_dist = z(B, N) if ("rel_dist" in st or self.num_scenes) and self.group_mode == "distinct" and not self.reach else None
        self._fill_post_args(st, dict(penalty or dict(table_collision=0.0, objects_off_table=1.0, wrist_collision=0.0)),
                             goal_reward_per_object, success_reward, max_timesteps_per_goal_per_obj, successes_needed, use_goal_distance_reward, reward_clip, starting_seed)
        self.icp = self.icp_rel = self.icp_clouds = None
        if rot_dist_type == "icp":
            self._fill_icp_args()
        self.action_shape = (self.B, self.action_dim)
        self._zero_action = z(B, AD)
        # ---- per-env model parameters: the reference's simulation randomizers (applied after _reset, robot_env.py:779-783) and stabilize_objects' damping change
        self.stabilize_object_damping = float(stabilize_object_damping)
        self.obj_dofs = torch.tensor([d for v in self.obj_v for d in range(v, v + 6)], device=dev, dtype=torch.long)
        self.randomizers = build_simulation_randomizers(main, self.randomizer_params) if self.per_env_parameters else []
        self._rand_gen = torch.Generator(device=dev); self._rand_gen.manual_seed(int(starting_seed) + 90001)
        if self.per_env_parameters:
            self._param_defaults = {k: self.sim.params[k][0].clone() for k in self.sim.params.keys()}
            self._param_block_default = self.sim.params.block[0].clone()
        # ---- RearrangeEnv.apply_wrappers (common/base.py:986-996): SmoothActionWrapper(alpha = 0.3) -> ClipRewardWrapper -> DiscretizeActionWrapper, all inside
        # the launches: the solver world's launch maps bin indices to actions and smooths them (rb_tcp_args), the post kernel clips the reward
        self.n_action_bins = int(n_action_bins)
        self.ema_value, self.ema_t, self.action_ema = z(B, AD), z(B, dt=torch.int32), z(B, AD)
        self.bins = torch.tensor(np.tile(action_bin_array(-1.0, 1.0, self.n_action_bins, action_spacing), (AD, 1)).astype(np.float32), device=dev).contiguous()   # over Box(-1, 1)
        tw = self.tcp_wrapped = _native.RbTcpArgs()
        ctypes.memmove(ctypes.byref(tw), ctypes.byref(self.tcp), ctypes.sizeof(tw))
        tw.bins, tw.nbins = self.bins.data_ptr(), self.n_action_bins
        self.ema_alpha = tw.ema_alpha = float(np.power(smooth_alpha, float(np.asarray(A["opt_timestep"]).reshape(-1)[0]) * n_substeps / 0.08))       # SmoothActionWrapper.reset (wrappers/util.py:203-211)
        tw.ema_value, tw.ema_t, tw.action_out = self.ema_value.data_ptr(), self.ema_t.data_ptr(), self.action_ema.data_ptr()
        # ---- the device recipe: its state and the recipe kernel's arguments
        self.device_reset = bool(device_reset)
        if self.device_reset:
            self.stage, self.left, self.yaw, self.placement_failed = z(B, dt=torch.int32), z(B, dt=torch.int32), z(B, N), z(B, dt=torch.int32)
            self.reobserve, self.ended, self.stabilised = torch.full((B,), _native.RA_OBS_SKIP, dtype=torch.uint8, device=dev), z(B, dt=torch.bool), z(B, dt=torch.bool)
            self._fill_recipe_args(starting_seed)
            self._fill_sync_reset_args()

    def _fill_scenes(self, initial_states, goal_states, advance_goals):
        """Recorded scenes: the state tables of `initial_states` / `goal_states` and what is derived from them once, in float64 -- the turned boxes of the starts
        (`rotated_half`), the goals' normalised Euler angles and euler2quat of those -- as float32 host arrays (the host route) and device tensors (ra_recipe_args), and
        the per-env rows `scene_next`, `scene`, `goal_cursor`.  Without tables: no row, no pointer."""
        self.num_scenes, self.advance_goals = 0, bool(advance_goals)
        self.scene_init = self.scene_init_half = self.scene_goal = self.scene_goal_rot = self.scene_num_goals = self.scene_next = self.scene = self.goal_cursor = None
        if initial_states is None and goal_states is None:
            if self.advance_goals:
                raise ValueError("advance_goals=True without goal_states: there is no list of recorded goals to step through")
            return
        if self.goal_kind_name != "object_state":      # (the constructor's head has refused max_num_objects and the worlds that are no block worlds)
            raise ValueError("initial_states / goal_states belong to goal_kind \"object_state\" (HoldoutObjectStateGoal is an ObjectStateGoal), not to %r" % (self.goal_kind_name,))
        N, dev = self.N, self.device
        init = goals = None
        if initial_states is not None:
            given = [initial_states] if _is_state(initial_states) else list(initial_states)
            if not given:
                raise ValueError("initial_states is an empty list")
            init = np.stack([load_state(s, N, "initial_states[%d]" % i) for i, s in enumerate(given)])
        if goal_states is not None:
            given = [goal_states] if _is_state(goal_states) else list(goal_states)
            per_scene = len(given) > 0 and not _is_state(given[0])
            S = len(init) if init is not None else (len(given) if per_scene else 1)
            if per_scene and len(given) != S:
                raise ValueError("goal_states lists the goals of %d scenes, initial_states has %d" % (len(given), S))
            per = [list(g) for g in given] if per_scene else [given] * S
            goals = [[load_state(s, N, "goal_states[%d][%d]" % (i, j)) for j, s in enumerate(g)] for i, g in enumerate(per)]
            if not any(goals):
                raise ValueError("goal_states holds no state")
        if self.advance_goals and goals is None:
            raise ValueError("advance_goals=True without goal_states: there is no list of recorded goals to step through")
        S = self.num_scenes = len(init) if init is not None else len(goals)
        f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        up = lambda x: torch.as_tensor(x, device=dev).contiguous()
        if init is not None:
            self._scene_init, self._scene_init_half = f32(init), f32(rotated_half(self.obj_half, init[..., 3:]))
            self.scene_init, self.scene_init_half = up(self._scene_init), up(self._scene_init_half)
            self.static_obs[:, :, 6] = 1.0      # (no colour is applied to a recorded start, HoldoutRearrangeEnv._apply_object_colors: the rows keep this)
        if goals is not None:
            G = max(len(g) for g in goals)
            table = np.zeros((S, G, N, 7)); table[..., 3] = 1.0
            for i, g in enumerate(goals):
                if g:
                    table[i, :len(g)] = np.stack(g)
            eul = mat2euler(quat2mat(table[..., 3:]))
            eul = np.mod(eul + np.pi, 2 * np.pi) - np.pi                    # get_target_rot + normalize_angles
            self._scene_goal, self._scene_goal_rot = f32(table), f32(np.concatenate([eul, euler2quat(eul)], -1))
            self._scene_num_goals = np.array([len(g) for g in goals], dtype=np.int32)
            self.max_scene_goals = G
            self.scene_goal, self.scene_goal_rot, self.scene_num_goals = up(self._scene_goal), up(self._scene_goal_rot), up(self._scene_num_goals)
            self.goal_cursor = torch.zeros(self.B, dtype=torch.int32, device=dev)
        self.scene_next = (torch.arange(self.B, dtype=torch.int32, device=dev) % S).contiguous()
        self.scene = self.scene_next.clone()

    def set_scene_next(self, scenes, rows=None):
        """The scene of the NEXT episode of the envs `rows` (default: every env), checked: an int or one per env, each in 0..S-1.  (Writing `self.scene_next`
        directly, as a curriculum on the device does, is clamped to that range where it is latched.)"""
        if not self.num_scenes:
            raise ValueError("set_scene_next: the env was built without initial_states / goal_states")
        c = np.asarray(scenes)
        if c.size == 0 or not np.all(c == np.round(c)) or c.min() < 0 or c.max() >= self.num_scenes:
            raise ValueError("scene_next %r: a scene index is outside 0..%d" % (np.asarray(scenes).tolist(), self.num_scenes - 1))
        t = torch.as_tensor(c.astype(np.int32), device=self.device)
        if rows is None:
            self.scene_next.copy_(t.expand(self.B) if t.dim() == 0 else t)
        else:
            self.scene_next[torch.as_tensor(rows, device=self.device, dtype=torch.long)] = t

    def record_state(self, rows=None):
        """The live objects of the envs `rows` (default: every env; an int: that env alone, without the batch axis) as a state dict {"obj_pos", "obj_quat"} of
        float64 arrays -- what the reference's `create_holdout` tool saves, and what `initial_states` / `goal_states` take."""
        one = np.isscalar(rows)
        idx = torch.arange(self.B, device=self.device) if rows is None else torch.as_tensor(np.atleast_1d(rows), device=self.device, dtype=torch.long)
        q = self.sim.qpos[idx].cpu().numpy().astype(np.float64)
        pose = np.stack([q[:, qa:qa + 7] for qa in self.obj_q], 1)
        pose = pose[0] if one else pose
        return {"obj_pos": pose[..., :3].copy(), "obj_quat": pose[..., 3:].copy()}

    def _fill_tcp_args(self, max_position_change, arm_reset_controller_error):
        """`self.tcp`, rb_tcp_args of the TCP hook: on the solver world, or (`ideal_arm`) on the env's own world (rb_tcp_args.self_world: TCP pose + denormalised action ->
        mocap target, gripper target into this world's ctrl, then its mj_steps).  Joint control has no hook: the main world's launch maps the action itself."""
        main, solver = self.model, self.solver_model
        A, jn = main.arrays, main.names["joint"]
        t = self.tcp = _native.RbTcpArgs()
        t.hold, t.scripted = self.hold.data_ptr(), self.scripted.data_ptr()      # (the recipe's rows; zero unless a pipelined or a device reset is under way)
        self.solver_arm_q, self.solver_grip_q, self.solver_grip_act = [], -1, -1
        if self.joint_control:
            # JointControlledArm drives ctrl[:6] from the six arm joints (joint_controlled_arm.py:186-190), MujocoRobotiqGripper its own actuator; relative actions:
            # arm joint k around its position, +- min(ctrl range / 2, max_position_change); the gripper around its control, +- ctrl range / 2
            assert self.grip_act == 6 and self.nu == 7 and list(np.diff(self.arm_q)) == [1] * 5, "joint control: ctrl[:6] = the arm's joints, ctrl[6] = the gripper"
            assert [int(np.ravel(A["actuator_trnid"][u])[0]) for u in range(6)] == [jn.index("robot0:J%d" % k) for k in range(1, 7)], main.names["actuator"]
            P = np.zeros((7, 6), dtype=np.float32); P[:6] = np.eye(6)
            self.sim.set_action_map(self.arm_q[0], P, relative_action=True, max_position_change=float(max_position_change), ctrl_centre_mask=1 << self.grip_act)
            return
        world = main if self.ideal_arm else solver      # the world the hook runs on
        wj = world.names["joint"]
        for k in range(6):
            t.arm_qposadr[k] = int(world.arrays["jnt_qposadr"][wj.index("robot0:J%d" % (k + 1))]); t.main_arm_qposadr[k] = self.arm_q[k]
        t.main_gripper_actuator = self.grip_act; t.tcp_body = world.name2id("body", "robot0:gripper_tcp"); t.wrist_joint = wj.index("robot0:J6")
        t.wrist_only = 1 if self.wrist_only else 0
        t.max_position_change = max_position_change; t.speed_roll = SPEED_ROLL; t.speed_pitch = SPEED_PITCH; t.joint_drift_threshold = JOINT_DRIFT_THRESHOLD
        t.gripper_ctrl_lo, t.gripper_ctrl_hi = float(A["actuator_ctrlrange"][self.grip_act, 0]), float(A["actuator_ctrlrange"][self.grip_act, 1])
        if self.ideal_arm:
            assert self.nu == 1 and self.grip_act == 0 and int(A["body_mocapid"][main.name2id("body", "robot0:mocap")]) == 0
            t.reset_controller_error = 0; t.self_world = 1
            self._tcp_body, self._gripper_base_body = int(t.tcp_body), main.name2id("body", "robot0:gripper_base")
        else:
            t.reset_controller_error = 1 if arm_reset_controller_error else 0
            self.solver_arm_q = [int(t.arm_qposadr[k]) for k in range(6)]
            self.solver_grip_q = int(solver.arrays["jnt_qposadr"][wj.index("robot0:r_gripper_RJ0_outer")])
            self.solver_grip_act = solver.names["actuator"].index("robot0:r_gripper_finger_joint")

    def _fill_post_args(self, st, pen, goal_reward_per_object, success_reward, max_timesteps_per_goal_per_obj, successes_needed, use_goal_distance_reward, reward_clip, starting_seed=0):
        """`self.post`, ra_post_args of the env kernel (csrc/ra_env_kernel.h): the env-level rows, where the robot, the objects and the table are in the main world, the
        thresholds `st`, the rewards and the penalties `pen`"""
        main, N = self.model, self.N
        A, jn, gn, sn = main.arrays, main.names["joint"], main.names["geom"], main.names["sensor"]
        a = self.post = _native.RaPostArgs()
        a.obs, a.obs_dim, a.num_objects = _ptr(self.packed), self.obs_dim, N
        for name, ten in (("t", self.t), ("steps", self.steps), ("steps_since_last_goal", self.ssl), ("successes_so_far", self.successes), ("consecutive", self.consecutive),
                          ("prev_nsucc", self.prev_nsucc), ("prev_valid", self.prev_valid), ("goal", self.goal), ("goal_rot", self.goal_rot), ("qpos_goal", self.qpos_goal),
                          ("static_obs", self.static_obs), ("reward", self.reward), ("goal_dist", self.goal_dist), ("done", self.done), ("goal_reset", self.goal_reset),
                          ("trial_success", self.trial_success), ("sub_goal_ok", self.sub_goal_ok), ("env_crash", self.env_crash), ("objects_off_table", self.objects_off_table),
                          ("info_ssl", self.info_ssl)):
            setattr(a, name, _ptr(ten))
        for i in range(N):
            a.obj_body[i] = main.name2id("body", "object%d" % i)
        a.tcp_body = main.name2id("body", "robot0:gripper_tcp")
        for k in range(6):
            a.arm_qposadr[k] = self.arm_q[k]
        a.grip_qposadr, a.grip_dofadr, a.grip_act = self.grip_q, int(A["jnt_dofadr"][jn.index("robot0:r_gripper_RJ0_outer")]), self.grip_act
        a.finger_geom[0], a.finger_geom[1] = gn.index("robot0:left_contact_v"), gn.index("robot0:right_contact_v")
        a.table_plane_geom = gn.index("table_collision_plane")
        a.force_adr, a.torque_adr = int(A["sensor_adr"][sn.index("toolhead_force")]), int(A["sensor_adr"][sn.index("toolhead_torque")])
        mask = 0
        for bname in ("robot0:gripper_base", "left_gripper", "left_inner_follower", "left_outer_driver", "right_gripper", "right_inner_follower", "right_outer_driver"):
            bid = main.name2id("body", bname)
            for g in range(len(gn)):
                if A["geom_bodyid"][g] == bid:
                    if g >= 64:      # (the env kernel's gripper - table scan keeps the gripper's geoms in one 64-bit mask)
                        raise ValueError("gripper geom %r has id %d: the env kernel needs the gripper's geoms below id 64" % (gn[g], g))
                    mask |= 1 << g
        a.gripper_geom_mask = mask
        lo, hi = self.table_pos - self.table_size, self.table_pos + self.table_size
        a.table_min[0], a.table_min[1], a.table_max[0], a.table_max[1], a.table_height = float(lo[0]), float(lo[1]), float(hi[0]), float(hi[1]), self.table_height
        a.pos_threshold, a.rot_threshold, a.goal_pos_offset, a.goal_rot_weight = st["obj_pos"], st["obj_rot"], 0.0, 1.0
        a.goal_reward_per_object, a.success_reward = goal_reward_per_object, success_reward
        a.penalty_table_collision, a.penalty_objects_off_table, a.penalty_safety_stop = pen.get("table_collision", 0.0), pen.get("objects_off_table", 0.0), pen.get("safety_stop", 0.0)
        a.safety_stop_force = 150.0                                      # robot/ur16e/arm_interface.py:46
        a.max_timesteps_per_goal, a.successes_needed, a.use_goal_distance_reward = max_timesteps_per_goal_per_obj * N, successes_needed, int(use_goal_distance_reward)
        a.solver_grip_qposadr, a.solver_grip_act = self.solver_grip_q, self.solver_grip_act
        a.goal_kind = self.goal_kind if self.goal_kind_name in POST_KINDS else GOAL_KINDS["object_state"]
        a.grip_site, a.goal_dist_extra = main.names["site"].index("robot0:grip"), _ptr(self.goal_dist_extra)
        self._grip_site = int(a.grip_site)
        a.rot_dist_type = ROT_DIST_TYPES[self.rot_dist_type]
        if a.rot_dist_type:      # the tables euler_angle_difference_single_pair walks, in the reference's order (constant data: built once on the host)
            from robogym_amd.utils.rotation import parallel_quat_table
            self.parallel_quats = {m: torch.tensor(parallel_quat_table(m), dtype=torch.float32, device=self.device).contiguous() for m in ("mod90", "mod180")}
            a.parallel_quats, a.parallel_quats_180 = _ptr(self.parallel_quats["mod90"]), _ptr(self.parallel_quats["mod180"])
        if self.obj_group is not None:
            a.obj_group = _ptr(self.obj_group)
        if self.max_num_objects is not None:
            a.num_active, a.max_timesteps_per_goal_per_obj = _ptr(self.num_active), int(max_timesteps_per_goal_per_obj)
        if self.object_pool:
            a.obj_perm = _ptr(self.object_perm)
        if self.wrapped:
            a.reward_clip = float(reward_clip)
        if self.pipelined:
            a.frozen = self.frozen.data_ptr()
        if self.rel_dist is not None:
            a.rel_dist, a.rel_threshold = _ptr(self.rel_dist), float(st.get("rel_dist", 0.0))
        if self.mask_obs:
            a.mask_obs = 1
            self._fill_area_args(a)
            a.seed, a.step = (int(starting_seed) * 2654435761 + 40503) & 0xFFFFFFFF, 0

    def _fill_area_args(self, a):
        """The fields ra_post_args (mask_obs) and ra_recipe_args share, into either: the placement area of an env that uses all N objects, the table,
        `used_table_portion` (read with per-env object counts only: ra_area, csrc/ra_env_kernel.h) and, with the masks, the goal's mask row and its rule"""
        (off_x, off_y, _), (width, height, _) = self.placement_area(self.N)
        a.area_offset[0], a.area_offset[1], a.area_size[0], a.area_size[1], a.used_table_portion = float(off_x), float(off_y), float(width), float(height), float(self.used_table_portion)
        for k in range(3):
            a.table_pos[k], a.table_size[k] = float(self.table_pos[k]), float(self.table_size[k])
        if self.mask_obs:
            a.goal_in_area, a.soft_mask, a.mask_margin, a.area_height = _ptr(self.goal_in_area), int(self.soft_mask), self.mask_margin, PLACEMENT_AREA_HEIGHT

    def _fill_icp_args(self):
        """rot_dist_type icp: the clouds (constant, per object), the angles ra_env_icp leaves for the env kernel, and `self.icp`, its arguments"""
        from robogym_amd.envs.rearrange.icp import object_point_clouds
        a, N = self.post, self.N
        src, src_num, tgt, tgt_adr, tgt_num = object_point_clouds(self.model, N, self.icp_error_threshold, self.icp_max_num_vertices)
        self.icp_clouds = tuple(torch.as_tensor(x, device=self.device).contiguous() for x in (src, src_num, tgt, tgt_adr, tgt_num))
        self.icp_rel = torch.zeros(self.B, N, 3, device=self.device)
        c = self.icp = _native.RaIcpArgs()
        c.icp_rel, c.goal, c.num_objects = _ptr(self.icp_rel), _ptr(self.goal), N
        for i in range(N):
            c.obj_body[i] = a.obj_body[i]
        c.src, c.src_stride, c.src_num = _ptr(self.icp_clouds[0]), int(src.shape[1]), _ptr(self.icp_clouds[1])
        c.tgt, c.tgt_total, c.tgt_adr, c.tgt_num = _ptr(self.icp_clouds[2]), int(tgt.shape[0]), _ptr(self.icp_clouds[3]), _ptr(self.icp_clouds[4])
        c.error_threshold = self.icp_error_threshold
        c.obj_group, c.num_active, c.obj_perm = a.obj_group, a.num_active, a.obj_perm
        a.icp_rel = _ptr(self.icp_rel)

    def _fill_recipe_args(self, starting_seed):
        """`self.recipe`, ra_recipe_args of the recipe kernel (ra_env_recipe_step, include/rgstep.h): the stage machine's rows, the placement geometry, the goal kind's numbers"""
        N = self.N
        r = self.recipe = _native.RaRecipeArgs()
        r.num_objects, r.action_dim = N, self.launch_action_dim
        for name, ten in (("stage", self.stage), ("left", self.left), ("yaw", self.yaw), ("done", self.done), ("goal_reset", self.goal_reset), ("hold", self.hold),
                          ("hold_ctrl", self.hold_ctrl), ("solver_active", self.solver_active), ("nticks", self.nticks), ("scripted", self.scripted), ("frozen", self.frozen),
                          ("resetting", self.resetting), ("episode_started", self.episode_started), ("reobserve", self.reobserve), ("ended", self.ended),
                          ("stabilised", self.stabilised), ("placement_failed", self.placement_failed), ("t", self.t), ("steps", self.steps), ("steps_since_last_goal", self.ssl),
                          ("successes_so_far", self.successes), ("consecutive", self.consecutive), ("prev_valid", self.prev_valid), ("ema_t", self.ema_t),
                          ("ema_value", self.ema_value), ("action_ema", self.action_ema), ("goal", self.goal), ("goal_rot", self.goal_rot), ("qpos_goal", self.qpos_goal),
                          ("static_obs", self.static_obs)):
            setattr(r, name, _ptr(ten))
        for i in range(N):
            r.obj_qposadr[i] = self.obj_q[i]
            for k in range(3):
                r.obj_center[i][k], r.obj_half[i][k] = float(self.obj_center[i, k]), float(self.obj_half[i, k])
        for k in range(6):
            r.arm_qposadr[k], r.arm_start[k] = self.arm_q[k], float(TABLETOP_EXPERIMENT_INITIAL_POS[k])
            r.solver_arm_qposadr[k] = self.solver_arm_q[k] if self.solver_arm_q else 0
        self._fill_area_args(r)
        r.stabilize_steps, r.n_random_initial_steps, r.settle_steps = int(self.stabilize_steps), int(self.n_random_initial_steps), int(self.settle_steps)
        r.seed, r.step = (int(starting_seed) * 2654435761 + 40503) & 0xFFFFFFFF, 0
        r.goal_kind, r.height_range[0], r.height_range[1], r.object_size = self.goal_kind, self.height_range[0], self.height_range[1], self.object_size
        r.fixed_order, r.target_height, r.goal_index = int(self.fixed_order), self.target_height, _ptr(self.goal_index)
        for j in range(2):
            for k in range(3):
                r.det_points[j][k] = float(DET_REACH_POINTS[j, k])
        r.goal_distance_ratio, r.goal_distance_min, r.pickup_proba, r.stacking_proba = _ptr(self.goal_distance_ratio), self.goal_distance_min, self.pickup_proba, self.stacking_proba
        if self.obj_group is not None:
            r.obj_group, r.group_mode = _ptr(self.obj_group), _native.RA_GROUPS_SAMPLE if self.group_mode == "sample" else _native.RA_GROUPS_KEEP
            r.sample_lam[0], r.sample_lam[1] = self.sample_lam
        r.randomize_goal_rot, r.domino_distance_mul = int(self.randomize_goal_rot), self.domino_distance_mul
        if self.goal_kind_name == "fixed":
            for i in range(N):
                r.fixed_xy[i][0], r.fixed_xy[i][1], r.fixed_yaw[i] = float(self.relative_placements[i, 0]), float(self.relative_placements[i, 1]), float(self.init_yaw[i])
        if self.max_num_objects is not None:
            r.num_active, r.num_objects_next = _ptr(self.num_active), _ptr(self.num_objects_next)
            for i in range(N):
                for k in range(7):
                    r.park_pose[i][k] = float(self.park_pose[i, k])
        if self.object_pool:
            r.obj_perm, r.obj_perm_next = _ptr(self.object_perm), _ptr(self.object_perm_next)
        if self.num_scenes:
            r.num_scenes, r.scene_next, r.scene = self.num_scenes, _ptr(self.scene_next), _ptr(self.scene)
            if self.scene_init is not None:
                r.scene_init, r.scene_init_half = _ptr(self.scene_init), _ptr(self.scene_init_half)
            if self.scene_goal is not None:
                r.scene_goal, r.scene_goal_rot, r.scene_num_goals, r.max_scene_goals = _ptr(self.scene_goal), _ptr(self.scene_goal_rot), _ptr(self.scene_num_goals), self.max_scene_goals
                r.goal_cursor, r.advance_goals = _ptr(self.goal_cursor), int(self.advance_goals)

    def _fill_sync_reset_args(self):
        """What the device route has beside the recipe's arguments: the `active` row of the synchronous launches (`reset(mask, on_device=True)`) and
        `self.param_rows` (ra_param_rows_args, include/rgstep_sync_reset.h: the per-env parameter rows on the recipe's masks; its `active`: `_param_rows_launch`)."""
        self.active_row = torch.zeros(self.B, dtype=torch.uint8, device=self.device)
        self.param_rows = None
        if self.per_env_parameters:
            a = self.param_rows = _native.RaParamRowsArgs()
            a.ended, a.stabilised, a.episode_started = _ptr(self.ended), _ptr(self.stabilised), _ptr(self.episode_started)
            self._param_block_default = self._param_block_default.contiguous()
            a.block_default, a.num_objects = _ptr(self._param_block_default), self.N
            for i in range(self.N):
                a.obj_dofadr[i], a.obj_body[i] = self.obj_v[i], self.model.name2id("body", "object%d" % i)
            a.stabilize_damping, a.park_damping = self.stabilize_object_damping, PARK_DAMPING
            if self.max_num_objects is not None:
                a.num_active = _ptr(self.num_active)
            if self.object_pool:
                a.obj_perm = _ptr(self.object_perm)
            if self.materials_on:
                self._fill_material_args(a)
        for rz in self.randomizers:      # (their index tables: uploaded here, not inside a reset that must not wait for the device)
            rz.prepare(self.sim)

    def _fill_material_args(self, a):
        """Per-object materials: the table, the list a draw picks from, the rows `object_material` / `object_material_next`, and what the stage needs of the model --
        every object's geoms, the lever of its centre of mass, the offsets of the fields it writes (ra_param_rows_args, include/rgstep_sync_reset.h)."""
        dev, B, N, A = self.device, self.B, self.N, self.model.arrays
        self.material_table = torch.tensor(materials.material_table(), device=dev).contiguous()
        self.object_material = torch.full((B, N), materials.MATERIAL_NAMES.index("default"), dtype=torch.int32, device=dev)
        self.object_material_next = torch.full((B, N), -1, dtype=torch.int32, device=dev)
        a.mat_table, a.num_materials, a.num_choice = _ptr(self.material_table), len(materials.MATERIAL_NAMES), len(self.material_names)
        for k, name in enumerate(self.material_names):
            a.mat_choice[k] = materials.MATERIAL_NAMES.index(name)
        a.obj_material, a.obj_material_next, a.mat_seed = _ptr(self.object_material), _ptr(self.object_material_next), int(self.recipe.seed)
        if self.obj_group is not None:
            a.obj_group = _ptr(self.obj_group)
        parents, gb = np.asarray(A["body_parentid"]), np.asarray(A["geom_bodyid"])
        for i in range(N):
            body = int(a.obj_body[i])
            geoms = np.nonzero(gb == body)[0]
            if len(geoms) == 0 or not np.array_equal(geoms, np.arange(geoms[0], geoms[0] + len(geoms))) or np.any(parents == body) or int(parents[body]) != 0:
                raise NotImplementedError("material_names: object%d is not one free body with one run of geoms (its _invweight0 rows are written in closed form)" % i)
            a.obj_geomadr[i], a.obj_geomnum[i] = int(geoms[0]), len(geoms)
            axes, r = quat2mat(np.asarray(A["body_iquat"][body], dtype=np.float64)), np.asarray(A["body_ipos"][body], dtype=np.float64)
            for k in range(3):
                a.obj_lever2[i][k] = float(np.sum(np.cross(r, axes[:, k]) ** 2))
        rows, P = self.sim.view(_native.RG_F_DEBUG), self.sim.params
        for k, name in enumerate(("geom_friction", "geom_solref", "geom_solimp", "body_mass", "body_inertia", "dof_armature", "dof_invweight0", "body_invweight0")):
            a.mat_off[k] = (P[name].data_ptr() - rows.data_ptr()) // 4
        #: the randomizers that would put the model's row in place of the material's: they start from the env's own rows (`_randomize`)
        self._material_fields = ("geom_friction", "geom_solref", "geom_solimp", "body_mass", "body_inertia")

    # ------------------------------------------------------------------ launches
    def _stream(self):
        return None if self.sim._emul else ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _post(self, frozen=None):
        """The env kernel.  `frozen`: the [B] uint8 codes THIS launch goes by, in place of the ones the arguments point to (which they point to again afterwards)."""
        if frozen is not None:
            had, self.post.frozen = self.post.frozen, frozen.data_ptr()
        if self.icp is not None:     # rot_dist_type icp: the angles of this state, for the envs this launch of the env kernel scores (the same frozen codes)
            self.icp.frozen = self.post.frozen
            _native.check(self._L, self._L.ra_env_icp(self.sim._bh, ctypes.byref(self.icp), self._stream()), "ra_env_icp")
        _native.check(self._L, self._L.ra_env_post_step(self.sim._bh, None if self.solver_sim is None else self.solver_sim._bh, ctypes.byref(self.post), self._stream()), "ra_env_post_step")
        if frozen is not None:
            self.post.frozen = had

    def _joint_action(self, actions, wrapped, recipe_rows=None):
        """Joint control: the [B, 7] action that reaches `RobotEnv._set_action`.  With the wrapper stack: bin index -> value (DiscretizeActionWrapper.action,
        wrappers/util.py:66-70) -> exponential moving average with bias correction (SmoothActionWrapper.step / IncrementalExpAvg, util.py:142-160, 213-218) -- a few
        elementwise device ops here (in TCP mode the solver world's launch does them).  `recipe_rows` (`_physics`): envs inside their recipe take its scripted action."""
        recipe_rows = self.pipelined if recipe_rows is None else recipe_rows
        if wrapped:
            x = self.bins[torch.arange(self.action_dim, device=self.device)[None, :], actions.long()]
            live = (self.hold == 0) if recipe_rows else torch.ones(self.B, dtype=torch.bool, device=self.device)
            al = self.ema_alpha
            v = torch.where(live[:, None], self.ema_value * al + (1.0 - al) * x, self.ema_value)
            self.ema_value.copy_(v)
            self.ema_t += live.to(torch.int32)
            out = v / (1.0 - torch.pow(torch.full_like(v[:, :1], al), self.ema_t[:, None].to(torch.float32))).clamp_min(1.0e-30)
            self.action_ema.copy_(torch.where(live[:, None], out, self.action_ema))
            actions = self.action_ema
        if recipe_rows:
            actions = torch.where(self.hold[:, None] != 0, self.scripted, actions)
        return actions.contiguous()

    def _physics(self, actions, active=None, wrapped=False, solver_active=None, phase=None, recipe_rows=None):
        """`phase`: None = both physics launches; "solver" / "main" = one of them (envs/rearrange/ycb.py GroupedYcbRearrangeEnv records the same phase of every group and
        issues it as ONE launch, rb_multi_begin / rb_multi_launch).  `recipe_rows`: the launches go by the rows the reset recipe maintains -- `nticks`, joint control's
        `hold_ctrl` and scripted actions (the TCP hook reads `hold` / `scripted` anyway: zero rows outside a recipe) -- as every step of a pipelined env (the
        default, None: `self.pipelined`; bench.py wraps this method with the step's five arguments) and every iteration of `_reset_device` (True) does."""
        recipe_rows = self.pipelined if recipe_rows is None else recipe_rows
        if phase == "solver" and (self.joint_control or self.ideal_arm):
            return                        # one-world robots have no solver phase
        nticks = self.nticks if recipe_rows else None
        if self.joint_control:     # CompositeRobot.set_position_control at the head of the main world's launch; no solver world
            self._keep_act = self._joint_action(actions, wrapped, recipe_rows)
            self.sim.env_step(action=self._keep_act, nforward_ticks=2, flags=FLAG_FULL_FORWARD, active=active, nticks=nticks, hold=self.hold_ctrl if recipe_rows else None)
            return
        if self.ideal_arm:         # one launch: the hook on this world, its mj_steps, the two state-less forwards (the last in full)
            args = self.tcp_wrapped if wrapped else self.tcp
            if wrapped:
                args.action_index = actions.data_ptr(); self._keep_idx = actions
            args.nforward_ticks = 2
            self.sim.step_tcp(self.sim, None if wrapped else actions, args, flags=FLAG_FULL_FORWARD, active=active)
            return
        sa = active if solver_active is None else solver_active      # (pipelined resets: envs that are settling their objects skip the solver world)
        if phase == "main":
            pass
        elif wrapped:       # `actions`: int32 bin indices through the wrapper stack's action path
            self.tcp_wrapped.action_index = actions.data_ptr()
            self._keep_idx = actions
            self.solver_sim.step_tcp(self.sim, None, self.tcp_wrapped, active=sa)
        else:
            self._keep_actions = actions
            self.solver_sim.step_tcp(self.sim, actions, self.tcp, active=sa)
        if phase == "solver":
            return
        # live envs: sim.step's forward + _observe_sync's forward = two controller ticks, the last forward in full; envs inside their reset recipe (pipelined
        # resets): `mujoco_simulation.step()` only = one tick, `self.nticks` (the recipe's last step gets the second tick: the _observe_sync that ends a reset)
        self.sim.env_step(nforward_ticks=2, flags=FLAG_FULL_FORWARD, active=active, nticks=nticks)

    def _recipe_physics(self, actions, active):
        """One step of the reset recipe's robot moves, `self._set_action(action); self.mujoco_simulation.step()` (common/base.py:484-496): the TCP solver world's
        launch, the main world's mj_steps with ONE state-less forward (MjSim.step), no _observe_sync: no second forward, no gripper hand-over to the solver world."""
        if self.joint_control:
            self.sim.env_step(action=actions, nforward_ticks=1, active=active)
            return
        if self.ideal_arm:
            self.tcp.nforward_ticks = 1
            self.sim.step_tcp(self.sim, actions, self.tcp, active=active)
            return
        self.solver_sim.step_tcp(self.sim, actions, self.tcp, active=active)
        self.sim.env_step(nforward_ticks=1, active=active)

    def step(self, actions: torch.Tensor):
        """RobotEnv.step (robot_env.py:804-844): returns (obs dict of [B, ...] views, reward [B, 3], done [B], info dict of tensors).
        Unwrapped: `actions` float32 [B, 6] in [-1, 1].  With the wrapper stack (`make_env`'s default): integer bin indices [B, 6] in [0, n_action_bins)."""
        self._step_launch(actions)
        return self._step_finish()

    def _step_launch(self, actions, phase=None):
        """The step's three launches, nothing that waits for them (envs/rearrange/ycb.py GroupedYcbRearrangeEnv enqueues several groups before it finishes any; with
        `phase` = "solver" / "main" / "post" one of the three, the action prepared by the first)."""
        if phase in (None, "solver"):
            assert actions.shape == self.action_shape and actions.device == self.device
            if self.wrist_only:      # [x, y, z, wrist, gripper] -> the launch's six columns (the roll column is ignored by the hook)
                actions = torch.cat([actions[:, :3], torch.zeros_like(actions[:, :1]), actions[:, 3:]], 1)
            if self.wrapped:
                assert not actions.dtype.is_floating_point, "the wrapped env takes MultiDiscrete actions (bin indices)"
                actions = actions.to(torch.int32).contiguous()
            else:
                assert actions.dtype == torch.float32 and actions.is_contiguous()
            self._phase_actions = actions
        if phase in (None, "post"):
            self._next_mask_step()
        if phase == "post":
            return self._post()
        sa = self.solver_active if self.pipelined else None
        self._physics(self._phase_actions, wrapped=self.wrapped, solver_active=sa, phase=phase)
        if phase is None:
            self._post()

    def _next_mask_step(self):
        """A new step() or reset(): the soft mask of the objects draws again (ra_post_args.step; the re-observations that follow carry the same value)"""
        if self.mask_obs:
            self._mask_step = (self._mask_step + 1) & 0xFFFFFFFF
            self.post.step = self._mask_step

    @property
    def goal_objects_in_placement_area(self):
        """[B, N] bool: the goal dict's `goal_objects_in_placement_area` (goals/object_state.py:404), an op on the device row; None without the masks"""
        return None if self.goal_in_area is None else self.goal_in_area != 0

    @property
    def goal_in_placement_area(self):
        """[B] bool: the goal dict's `goal_in_placement_area` (goals/object_state.py:403); None without the masks"""
        return None if self.goal_in_area is None else (self.goal_in_area != 0).all(dim=1)

    def placement_area_boundary(self, n=None):
        """`extract_placement_area_boundary` (simulation/base.py:834-845) for an env that uses `n` objects: (lo [3], hi [3]) of the placement area's box in world coordinates"""
        offset, size = self.placement_area(n)
        lo = np.asarray(offset, dtype=np.float64) + self.table_pos - self.table_size
        return lo, lo + np.asarray(size, dtype=np.float64)

    def _step_finish(self):
        if self.object_pool and self.pipelined:      # (the recipe launch below latches the next episode's row where an episode ended: the step's own row, for `info`)
            self._perm_of_step = self.object_perm.clone()
        if self.pipelined and self.device_reset:
            self._advance_recipes_device()
        elif self.pipelined:
            self._advance_recipes()
        return self.observe(), self.reward, self.done, self.info()

    def info(self):
        out = {"goal_dist_obj_pos": self.goal_dist[:, 0], "goal_dist_obj_rot": self.goal_dist[:, 1], "goal_reset": self.goal_reset, "trial_success": self.trial_success,
               "sub_goal_is_successful": self.sub_goal_ok, "env_crash": self.env_crash, "objects_off_table": self.objects_off_table, "successes_so_far": self.successes,
               "steps_since_last_goal": self.info_ssl, "resetting": self.resetting, "episode_started": self.episode_started}
        if self.rel_dist is not None:      # HoldoutObjectStateGoal.goal_distance's key, per object as the reference's goal_distance has it
            out["goal_dist"] = {"rel_dist": self.rel_dist}
        if self.goal_kind_name == "stack":      # ObjectStackGoal.goal_distance's two more keys, summed as goal_info["goal_dist"] sums every key (robot_env.py:611)
            out["goal_dist_gripper_pos"], out["goal_dist_grasped"] = self.goal_dist_extra[:, 0], self.goal_dist_extra[:, 1]
        return out

    def observe(self, packed=None, action_ema=None):
        """Views into the packed row, keys / shapes of `RearrangeEnv._observe_simple` (common/base.py:376-421), with `mask_obs_outside_placement_area` followed by
        MASK_OBS_KEYS (the two masks as [B, N, 1]).  (`packed` / `action_ema`: rows of several envs put together by the caller, envs/rearrange/ycb.py.)"""
        out, o, N = {}, 0, self.N
        used = self.num_objects_initial if self.object_pool else N      # object_pool: the n slots in use (the row keeps the world's width, zeros behind them)
        packed = self.packed if packed is None else packed
        for k, w in self.obs_keys:
            if isinstance(w, str):
                n = self.nq if w == "nq" else N * int(w[1])
                v = packed[:, o:o + n]
                out[k] = v if w == "nq" else v.view(packed.shape[0], N, int(w[1]))[:, :used]
            else:
                n = w
                out[k] = packed[:, o:o + n]
            o += n
        assert o == self.obs_dim
        if self.wrapped:
            ema = self.action_ema if action_ema is None else action_ema
            out["action_ema"] = ema[:, self._ext_cols] if self.wrist_only else ema      # SmoothActionWrapper's observation: the smoothed action of the last step (zeros after reset)
        return out

    # ------------------------------------------------------------------ reset (host work + physics launches)
    def _grid_placement(self, yaw, rows, n=None):
        """place_objects_in_grid (common/utils.py:719-829) for boxes: AABB of each yawed block, a grid of cells sized by the largest block over the
        placement area (simulation/base.py:992-1010), distinct random cells.  `n`: the first n objects only (`yaw` [len(rows), n]), in the placement area of that count."""
        if n is None:
            n = self.N
        B, N = len(rows), int(n)
        obj_half = self.obj_half[:N]
        half = self._aabb_half(yaw, N)
        offset, (width, height, _) = self.placement_area(N)
        xy = np.zeros((B, N, 2))
        ncol, nrow = (width // (2 * half[:, :, 0].max(1))).astype(int), (height // (2 * half[:, :, 1].max(1))).astype(int)
        crowded = ncol * nrow < N
        for r in np.nonzero(~crowded)[0]:
            cw, ch = width / ncol[r], height / nrow[r]
            cells = self._rng.permutation(ncol[r] * nrow[r])[:N]
            row_i, col_i = cells // ncol[r], cells % ncol[r]
            xy[r] = np.stack([cw * col_i + half[r, :, 0], ch * row_i + half[r, :, 1]], -1)
        if crowded.any():
            # fewer cells than objects (large mesh objects): place_objects_with_no_constraint (common/utils.py:829-880, _place_objects :623-716) --
            # uniform proposals inside the area, rejected while the object's box overlaps a placed one; a set restarts when one of its objects runs
            # out of trials (the reference gives up after max_placement_trial_count restarts and resamples the episode; this keeps trying).
            # All crowded rows are sampled together; the objects of a row are placed largest first (the reference goes in object order: with a table this
            # full that mostly runs out of trials on the last large object and starts over).
            pending = np.nonzero(crowded)[0]
            area = np.array([width, height])
            order = np.argsort(-(obj_half[:, 0] * obj_half[:, 1]), kind="stable")
            rounds = 0
            while len(pending):
                rounds += 1
                if rounds > 200:      # (the reference gives up after max_placement_trial_count restarts as well, common/utils.py:623-716)
                    raise RuntimeError("no collision-free placement for %d envs: the objects' bounding boxes cover %.0f %% of the placement area" % (
                        len(pending), 100 * float((4 * obj_half[:, 0] * obj_half[:, 1]).sum()) / (width * height)))
                h = half[pending]
                cur, alive = np.zeros((len(pending), N, 2)), np.ones(len(pending), dtype=bool)
                done_objs = []
                for i in order:
                    placed = np.zeros(len(pending), dtype=bool)
                    for _ in range(100):
                        need = np.nonzero(alive & ~placed)[0]
                        if len(need) == 0:
                            break
                        c_ = self._rng.uniform(h[need, i, :2], area - h[need, i, :2])
                        free = np.ones(len(need), dtype=bool)
                        if done_objs:
                            apart = (np.abs(c_[:, None, :] - cur[need][:, done_objs]) >= h[need, i, None, :2] + h[need][:, done_objs, :2]).any(-1)
                            free = apart.all(1)
                        cur[need[free], i] = c_[free]
                        placed[need[free]] = True
                    alive &= placed
                    done_objs.append(i)
                xy[pending[alive]] = cur[alive]
                pending = pending[~alive]
        p = np.concatenate([xy, half[:, :, 2:3] + 2 * self.table_size[2]], -1)
        return area_to_world(p, offset, self.table_pos, self.table_size) - yawed_centre(self.obj_center[:N], yaw)      # (the body origin, from the centre of its bounding box)

    def placement_area(self, n=None):
        """RearrangeSimulationInterface.get_placement_area / get_table_setting (simulation/base.py:980-1010): (offset, size) of the box objects and goals are placed
        in, offset measured from the table's low corner; `used_table_portion` is clipped to at least a tenth per object.  `n`: the area of an env that uses n objects
        (per-env object counts; default: all of them)."""
        if n is None:
            n = self.N
        tsx, tsy = 2 * self.table_size[0], 2 * self.table_size[1]
        portion = float(np.clip(self.used_table_portion, int(n) * 0.1, 1.0))
        width, height = 0.5 * tsx * portion, 0.38 * tsy * portion
        return (0.5 * tsx - width / 2.0, 0.44 * tsy - height / 2.0, 2 * self.table_size[2]), (width, height, 0.26)

    def _next_goal(self, rows, yaw):
        """`_update_simulation_for_next_goal` (goals/object_state.py:333-358) for the envs `rows`, whose goals have the yaws `yaw` [len(rows), N]: with
        `randomize_goal_rot` new yaws first (per env, over its active objects, in the reference's draw order; an unused slot keeps yaw 0), then the positions for boxes
        turned by them; the kinds of OWN_YAW_KINDS set yaws of their own.  -> `_write_goal`'s arguments: positions, and from the yaws the Euler angles (mat2euler of a
        z-rotation, normalised as get_target_rot + normalize_angles give it) and euler2quat of them, the quaternion of the goal rows and of qpos_goal alike."""
        counts = self._counts(rows)
        if self.randomize_goal_rot and len(rows):
            yaw = np.array(yaw, dtype=np.float64)
            for r, c in enumerate(counts):
                yaw[r, :c] = randomize_yaw_along_z(self._rng, yaw[r, :c])
        if self.goal_kind_name in OWN_YAW_KINDS:
            pos, yaw = self._own_yaw_goals(len(rows))
        else:
            pos = self._by_count(rows, yaw, counts, self._goal_positions)
        eul =np.zeros(pos.shape); eul[..., 2] = np.mod(yaw + np.pi, 2 * np.pi) - np.pi
        quat = euler2quat(eul)
        return pos, eul, quat, quat

    def _own_yaw_goals(self, R):
        """The goals of `R` envs for the kinds that turn the goals themselves, AFTER the randomisation (host numpy; ra_recipe_kernel does the same on the device):
        DominoStateGoal's circle arc with its yaws, AttachedBlockStateGoal's lattice (a permutation and an origin per env) and ObjectFixedStateGoal's table with
        init_quats' yaws, always -> ([R, N, 3], yaws [R, N])"""
        table = (self.table_pos, self.table_size) + self.placement_area(self.N)
        pos, yaws = np.zeros((R, self.N, 3)), np.tile(self.init_yaw, (R, 1))
        for r in range(R):
            if self.goal_kind_name == "dominos":
                pos[r], yaws[r], ok = domino_goal(self._rng, self.obj_half, self.object_size * self.domino_distance_mul, *table)
            elif self.goal_kind_name == "attached":
                pos[r], ok = attached_goal(self._rng, self.obj_center, self.obj_half, self.object_size, *table)
            else:
                pos[r], ok = fixed_goal(self.relative_placements, self.obj_center, self.obj_half, *table)
            if not ok:
                self.host_placement_failed += 1
        return pos, yaws

    def _counts(self, rows):
        """The object counts of the envs `rows` as host integers: N without max_num_objects (no device access), else the latched counts (the host recipe reads flags
        back anyway)"""
        if self.max_num_objects is None:
            return np.full(len(rows), self.N)
        return self.num_active[torch.as_tensor(rows, device=self.device, dtype=torch.long)].cpu().numpy().astype(np.int64)

    def _parked(self):
        """[N, 7] what fills an unused slot: its parking pose (zeros without max_num_objects, where no slot is unused and the fill is never read)"""
        return np.zeros((self.N, 7)) if self.park_pose is None else self.park_pose

    def _by_count(self, rows, yaw, counts, fn):
        """`fn(rows_n, yaw_n, n)` -> [len(rows_n), n, 3] for the rows of each count n (ascending), put together as [len(rows), N, 3] with the unused slots at their
        parking positions."""
        rows = np.asarray(rows)
        out = np.tile(self._parked()[None, :, :3], (len(rows), 1, 1))
        for n in np.unique(counts):
            sel = np.nonzero(counts == n)[0]
            out[sel, :n] = fn(rows[sel], yaw[sel, :n], int(n))
        return out

    def _goal_positions(self, rows, yaw, n=None):
        """`_sample_next_goal_positions` of the env's goal generator for the envs `rows` (host numpy; ra_recipe_kernel does the same on the device), for the first `n`
        objects (default: all of them) in the placement area of that count, `yaw` [len(rows), n] -> [len(rows), n, 3].  Every kind but those of OWN_YAW_KINDS
        (`_own_yaw_goals`).  Reach also moves the object itself (`set_object_pos`: position only) -- the caller's forward makes the observation see it."""
        if n is None:
            n = self.N
        R, N, kind = len(rows), int(n), self.goal_kind_name
        if kind in ("train",) + REACH_KINDS:
            idx = torch.as_tensor(rows, device=self.device, dtype=torch.long)
        if kind == "train":    # TrainStateGoal: goals near the objects' current positions, then one in the air or a tower (goals/train_state.py:81-113)
            qpos = self.sim.qpos[idx].cpu().numpy().astype(np.float64)
            ratios = self.goal_distance_ratio[idx].cpu().numpy().astype(np.float64)
            half, centre = self._aabb_half(yaw, N), yawed_centre(self.obj_center[:N], yaw)
            offset, size = self.placement_area(N)
            pos = np.zeros((R, N, 3))
            for r in range(R):
                op = np.array([qpos[r, qa:qa + 3] for qa in self.obj_q[:N]])
                pos[r], ok = place_targets_with_goal_distance_ratio(self._rng, centre[r], half[r], self.table_pos, self.table_size, offset, size, op, ratios[r], self.goal_distance_min)
                if not ok:
                    self.host_placement_failed += 1
                move_one_object_to_the_air_with_restrictions(self._rng, pos[r], self.height_range, self.object_size, self.pickup_proba, self.stacking_proba, ratios[r])
            return pos
        if kind in ("object_state", "pickandplace"):
            pos = self._grid_placement(yaw, rows, N)
            if kind == "pickandplace":      # move_one_object_to_the_air (goals/pickandplace.py:30-52): a height, then the object it raises
                h = self._rng.uniform(self.height_range[0], self.height_range[1], R)
                pos[np.arange(R), self._rng.randint(N, size=R), 2] += h
            return pos
        if kind == "det-reach":      # DeterministicReachGoal: the next of its two points, per env
            gi = (self.goal_index[idx] + 1) % 2
            self.goal_index[idx] = gi
            bottom = DET_REACH_POINTS[gi.cpu().numpy()]
        else:                        # place_objects_with_no_constraint on object 0's box alone
            bottom = self._free_placement_of_object0(yaw[:, 0], N)
        if kind == "stack":          # ObjectStackGoal: the others on top of object 0's placement, in a shuffled block order unless fixed_order
            pos = np.repeat(bottom[:, None, :], N, 1)
            for r in range(R):
                order = np.arange(N) if self.fixed_order else self._rng.permutation(N)
                pos[r, order, 2] += np.arange(N) * 2 * self.object_size
            return pos
        assert kind in REACH_KINDS, kind
        qa = self.obj_q[0]
        self.sim.qpos[idx, qa:qa + 3] = torch.tensor(bottom.astype(np.float32), device=self.device)
        pos = bottom[:, None, :].copy()
        pos[:, 0, 2] += self.target_height
        return pos

    def _free_placement_of_object0(self, yaw0, n=None):
        """place_objects_with_no_constraint (common/utils.py:829-880) for object 0 alone: a uniform proposal inside the placement area (one object: always free);
        the body origin in world coordinates, as _grid_placement gives it.  `yaw0` [R]; `n`: in the placement area of that object count."""
        offset, (width, height, _) = self.placement_area(n)
        h = yawed_half(self.obj_half[:1], yaw0[:, None])[:, 0]
        x, y = self._rng.uniform(h[:, 0], width - h[:, 0]), self._rng.uniform(h[:, 1], height - h[:, 1])
        p = np.stack([x, y, h[:, 2] + 2 * self.table_size[2]], -1)
        return area_to_world(p, offset, self.table_pos, self.table_size) - yawed_centre(self.obj_center[:1], yaw0[:, None])[:, 0]

    def _forward_rows(self, rows):
        """_observe_sync's forward (one controller tick, the full stage arrays) for the envs `rows` only."""
        if len(rows) == 0:
            return
        self.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=FLAG_FULL_FORWARD, active=self._mask_of(rows, torch.int32))

    def _write_goal(self, rows, goal_pos, eul, quat, qpos_quat):
        """The goal of the envs `rows`, sampled or recorded: positions [R, N, 3], Euler angles -> `goal_rot`, `quat` -> the goal rows, `qpos_quat` -> `qpos_goal`
        (a recorded goal keeps its own quaternion in the goal row and carries euler2quat of its angles in qpos_goal); the tracker's `prev_valid`, the goal's mask."""
        dev = self.device
        idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
        eul = np.array(eul, dtype=np.float32)
        g, q = (np.concatenate([goal_pos, x], -1).astype(np.float32) for x in (quat, qpos_quat))
        unused = np.arange(self.N)[None, :] >= self._counts(rows)[:, None]      # an unused slot: its parked pose in qpos_goal, a zero goal row (identity orientation)
        q[unused] = np.broadcast_to(self._parked().astype(np.float32)[None], q.shape)[unused]
        g[unused] = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32)
        eul[unused] = 0.0
        self.goal_rot[idx] = torch.tensor(eul, device=dev)
        qg = self.sim.qpos[idx].clone()                                   # qpos_goal: the current qpos with the objects at their goals (object_state.py:381-389)
        for i, qa in enumerate(self.obj_q):
            qg[:, qa:qa + 7] = torch.tensor(q[:, i], device=dev)
        self.qpos_goal[idx] = qg
        self.goal[idx] = torch.tensor(g, device=dev)
        self.prev_valid[idx] = 0
        self._write_goal_mask(rows, idx, g[..., :3], unused)

    def _write_goal_mask(self, rows, idx, goal_pos, unused):
        if self.mask_obs and len(rows):
            # the goal's mask of the placement area (goals/object_state.py:373-378), from the goal rows as written, in the area of each env's count; an unused slot
            # reads 1.  soft_mask: one draw per env, after the positions' draws (the reference's np.random.random() inside check_objects_in_placement_area)
            bounds = [self.placement_area_boundary(int(c)) for c in self._counts(rows)]
            lo, hi = np.array([b[0] for b in bounds])[:, None, :], np.array([b[1] for b in bounds])[:, None, :]
            u = self._rng.random(len(rows))[:, None] if self.soft_mask else None
            inside = objects_in_placement_area(goal_pos, lo, hi, self.mask_margin, self.soft_mask, u) | unused
            self.goal_in_area[idx] = torch.tensor(inside.astype(np.float32), device=self.device)

    def _make_goal(self, rows, yaw, first):
        """The next goal of the envs `rows`, whose goals (`first`: objects, at an episode start) have the yaws `yaw`: sampled (`_next_goal`), or for the envs whose
        scene has recorded goals state `goal_cursor` of the scene's list -- no draw; what ra_sample_goal does on the device, from the same tables."""
        rows = np.asarray(rows)
        if self.scene_goal is None or len(rows) == 0:
            return self._write_goal(rows, *self._next_goal(rows, yaw))
        dev = self.device
        idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
        sc = self.scene[idx].cpu().numpy().clip(0, self.num_scenes - 1)
        ng = self._scene_num_goals[sc]
        rec = ng > 0
        if (~rec).any():
            self._write_goal(rows[~rec], *self._next_goal(rows[~rec], np.asarray(yaw)[~rec]))
        if not rec.any():
            return
        rows, idx, sc, ng = rows[rec], idx[torch.as_tensor(rec, device=dev)], sc[rec], ng[rec]
        cur = np.zeros(len(rows), dtype=np.int64)
        if self.advance_goals and not first:      # (HoldoutObjectStateGoal.goal_idx never moves in the reference: advance_goals False)
            cur = self.goal_cursor[idx].cpu().numpy().astype(np.int64)
            cur = np.where((cur < 0) | (cur >= ng), 0, cur)
        self.goal_cursor[idx] = torch.as_tensor((((cur + 1) % ng) if self.advance_goals else 0 * cur).astype(np.int32), device=dev)
        g, rot = self._scene_goal[sc, cur], self._scene_goal_rot[sc, cur]      # [R, N, 7]: position | quaternion, Euler angles | euler2quat of them
        self._write_goal(rows, g[..., :3], rot[..., :3], g[..., 3:], rot[..., 3:])

    def _begin_episode_state(self, rows, idx):
        """What RearrangeEnv._reset writes before anything is simulated (common/base.py:897-932): both worlds as freshly made, the arm's start pose, object
        rotations about z and their placement, bounding boxes / colours of the static observation.  Returns the drawn yaw angles [len(rows), N]."""
        dev, N = self.device, self.N
        A = self.model.arrays
        if self.max_num_objects is not None:      # the count of the episode that begins: _recreate_sim builds the simulation with the current num_objects (common/base.py:850-856, 904)
            self.num_active[idx] = self.num_objects_next[idx].clamp(1, N)
        if self.scene is not None:                 # ... and its scene (recorded scenes), latched the same way
            self.scene[idx] = self.scene_next[idx].clamp(0, self.num_scenes - 1)
        counts = self._counts(rows)
        unused = np.arange(N)[None, :] >= counts[:, None]
        if self.group_mode == "sample":      # _randomize_object_groups: the first act of RearrangeEnv._reset (common/base.py:903), over the env's own count; an unused slot belongs to no group: -1
            rows_ids = np.stack([np.concatenate([group_ids(sample_group_counts(self._rng, int(c), *self.sample_lam)), np.full(N - int(c), -1, dtype=np.int32)]) for c in counts])
            self.obj_group[idx] = torch.tensor(rows_ids, dtype=torch.int32, device=dev)
        worlds = [(self.sim, A)] + ([] if self.solver_sim is None else [(self.solver_sim, self.solver_model.arrays)])
        if self.per_env_parameters:      # _recreate_sim (common/base.py:850-856): a fresh model -- the previous episode's randomised values are gone
            for k, v in self._param_defaults.items():
                self.sim.params[k][idx] = v
        # MjSim of a fresh model: qpos0, zero velocities / controller state / time; robot.reset()
        for sim, model in worlds:
            sim.qpos[idx] = torch.tensor(model["qpos0"].astype(np.float32), device=dev)
            for f in (sim.qvel, sim.ctrl, sim.pid, sim.qacc_warmstart):
                f[idx] = 0
            sim.view(_native.RG_F_TIME)[idx] = 0
            sim.view(_native.RG_F_STATUS)[idx] = 0
        arm0 = torch.tensor(TABLETOP_EXPERIMENT_INITIAL_POS.astype(np.float32), device=dev)
        if self.ideal_arm:
            self._initialize_mocap_world(idx)
        self.sim.qpos[idx[:, None], torch.tensor(self.arm_q, device=dev)] = arm0
        if self.ideal_arm:       # IdealJointControlledTcpArm.reset: joint positions, then solver.reset() = reset_mocap_welds (with its forward) + reset_mocap2body_xpos
            self._mocap_to_body(idx, self._tcp_body)
        else:
            self.sim.ctrl[idx, :6] = arm0
        if self.solver_sim is not None:
            self.solver_sim.qpos[idx[:, None], torch.tensor(self.solver_arm_q, device=dev)] = arm0
            self.solver_sim.eq_data[idx, :7] = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=dev)     # reset_mocap_welds
        if self.scene_init is not None:
            # HoldoutRearrangeEnv._randomize_object_initial_states (holdout.py:93-106): the recorded state -- the objects only, the targets keep the model's
            # orientation (the yaws a sampled first goal starts from: 0) --, the boxes turned by the recorded rotations, no colours; no draw
            sc = self.scene[idx].cpu().numpy()
            pose = self._scene_init[sc]
            for i, qa in enumerate(self.obj_q):
                self.sim.qpos[idx, qa:qa + 7] = torch.tensor(pose[:, i], device=dev)
            self.static_obs[idx, :, :3] = torch.tensor(self._scene_init_half[sc], device=dev)
            return np.zeros((len(rows), N))
        # object rotations about z and grid placement (common/base.py:613-640, 797-822): the env's first n objects in the placement area of n objects, the others
        # parked (identity orientation: yaw 0)
        yaw = self._rng.uniform(0.0, 2 * np.pi, (len(rows), N))
        yaw[unused] = 0.0
        pos = self._by_count(rows, yaw, counts, lambda rows_n, yaw_n, n: self._grid_placement(yaw_n, rows_n, n))
        quat = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], -1)
        for i, qa in enumerate(self.obj_q):
            self.sim.qpos[idx, qa:qa + 7] = torch.tensor(np.concatenate([pos[:, i], quat[:, i]], -1).astype(np.float32), device=dev)
        colors = self._rng.random_sample((len(rows), N, 4)); colors[..., 3] = 1.0
        so = np.concatenate([np.broadcast_to(self._aabb_half(yaw), (len(rows), N, 3)), colors], -1)
        so[unused] = 0.0
        if self.max_num_objects is not None:
            self._apply_parking(self._mask_of(idx))      # (after the block's restore above: a fresh model has no wrench and the model's damping)
        self.static_obs[idx] = torch.tensor(so.astype(np.float32), device=dev)
        return yaw

    def _mocap_to_body(self, idx, body):
        """reset_mocap_welds + "mocap pose <- that body's pose" for the envs `idx`: the weld's relative pose back to identity, one forward (kinematics + the controller
        tick of mj_forward), the mocap row from the body's frame (gym.envs.robotics.utils.reset_mocap_welds / reset_mocap2body_xpos)."""
        self.sim.eq_data[idx, :7] = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device=self.device)
        self.sim.env_step(nsubsteps=0, nforward_ticks=1, active=self._mask_of(idx, torch.int32))
        xp, xq = self.sim.scratch("xpos"), self.sim.scratch("xquat")
        self.sim.mocap[idx] = torch.cat([xp[idx, 3 * body:3 * body + 3], xq[idx, 4 * body:4 * body + 4]], 1)

    def _initialize_mocap_world(self, idx):
        """RearrangeEnv._initialize_sim_state for a mocap-actuated arm (common/base.py:448-465): welds reset, forward, the mocap body put at the pose of
        robot0:gripper_base, ten simulation steps (the weld pulls the TCP there)."""
        active = self._mask_of(idx, torch.int32)
        self._mocap_to_body(idx, self._gripper_base_body)
        for _ in range(10):
            self.sim.env_step(nforward_ticks=1, active=active)

    def _on_device(self, on_device):
        """Which recipe `reset` / `reset_goals` run: None = the device recipe exactly when the env was built with `device_reset` and without `pipelined_reset` (every
        other env keeps the path it had), True needs `device_reset`, False = the host recipe."""
        if on_device is None:
            return self.device_reset and (not self.pipelined or self.object_pool or self.materials_on)
        if not on_device and self.materials_on:
            raise NotImplementedError("material_names=%r: the host reset route is not built for materials (they are drawn and written by the device route's "
                                      "parameter-row launch); on_device=None or True" % (self.material_names,))
        if not on_device and self.object_pool:
            raise NotImplementedError("object_pool (per-env object subsets): the host reset route is not built for it (the permutation is latched and sampled by the "
                                      "recipe kernel); on_device=None or True")
        if on_device and not self.device_reset:
            raise ValueError("on_device=True needs an env built with device_reset=True (the recipe kernel's rows and arguments are made by the constructor)")
        return bool(on_device)

    def sync_reset_iterations(self):
        """Launch chains between the forced end and the episode start of a synchronous device reset: the stage machine's own count (ra_recipe_kernel: a stage of zero
        steps still takes one launch; without a random action there is no settling stage, as in `reset`'s host recipe)"""
        n = max(int(self.stabilize_steps), 1)
        if self.n_random_initial_steps >= 1:
            n += int(self.n_random_initial_steps) + max(int(self.settle_steps), 1)
        return n

    def _recipe_launch(self):
        r = self.recipe
        r.step = (int(r.step) + 1) & 0xFFFFFFFF
        _native.check(self._L, self._L.ra_env_recipe_step(self.sim._bh, None if self.solver_sim is None else self.solver_sim._bh, ctypes.byref(r), self._stream()), "ra_env_recipe_step")

    def _param_rows_launch(self, stages, active=None):
        """The per-env parameter rows of the device route on the masks the last recipe launch left (ra_param_rows_kernel, csrc/ra_env_kernel.h; the host route's twin:
        the `_param_defaults` restore, `_set_object_damping`, `_apply_parking`).  `active`: the [B] uint8 row of a synchronous reset; None = every env."""
        self.param_rows.stages, self.param_rows.active = stages, None if active is None else _ptr(active)
        if self.materials_on:      # (the draw of an episode that ended: the counter of the recipe launch whose masks these are)
            self.param_rows.mat_step = int(self.recipe.step)
        _native.check(self._L, self._L.ra_env_param_rows(self.sim._bh, ctypes.byref(self.param_rows), self._stream()), "ra_env_param_rows")

    def _row_stages(self):
        """the stages of the parameter-row launch that follows a recipe launch: the material stage with `material_names` only"""
        return _native.RA_ROWS_RESTORE | _native.RA_ROWS_PARK | (_native.RA_ROWS_MATERIAL if self.materials_on else 0)

    def _randomize(self, mask):
        """The simulation randomizers for the envs `mask` ([B] bool, device).  With materials the randomizers of the fields a material writes start from the env's
        rows as they stand -- the restored block plus the material, as the reference's start from the rebuilt world -- instead of the model's row."""
        for rz in self.randomizers:
            field = getattr(rz, "field_name", rz.name)
            if self.materials_on and field in self._material_fields:      # (`randomize` makes the new values before it writes the field: no copy needed)
                rz.randomize(self.sim, self._rand_gen, mask, initial=self.sim.params[field])
            else:
                rz.randomize(self.sim, self._rand_gen, mask)

    def _finish_recipe_launch(self, active=None, started=True):
        """What follows the last recipe launch of a step, of a synchronous reset (`active`: its [B] uint8 row, the envs outside it are left alone) or of a regoal-only
        launch (`started` False: that mode leaves the masks as they were, so nothing may go by them and no randomizer draws): the simulation randomizers for the envs
        whose episode starts, and the park stage after them (gravity and body masses may have changed: the cancelling force follows them); the reach goals' forward
        (the object the goal moved: _observe_sync's forward) and the env kernel, both over the `reobserve` codes -- first observation of a new episode / the new
        goal's entries / skip.  No readback."""
        act = None if active is None else active != 0
        if started and self.randomizers:
            mask = self.episode_started if act is None else self.episode_started & act
            self._randomize(mask)
            if self.max_num_objects is not None:
                self._param_rows_launch(_native.RA_ROWS_PARK, active)
        codes = self.reobserve if act is None else torch.where(act, self.reobserve, torch.full_like(self.reobserve, _native.RA_OBS_SKIP))
        if self.reach:
            self.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=FLAG_FULL_FORWARD, active=(codes != _native.RA_OBS_SKIP).to(torch.int32))
        self._post(frozen=codes)

    def _reset_device(self, mask):
        """`reset(mask)` without the host: one forced-end launch of the recipe kernel for the envs of the mask (ra_recipe_args.sync_mode; whatever recipe they were in
        ends), then `sync_reset_iterations()` times the pipelined step's launch chain restricted to those envs -- solver world and main world under the rows the recipe
        kernel maintains (hold / hold_ctrl / scripted / nticks / solver_active), the recipe launch (its `step` counter + 1 per launch: the draw streams of the pipelined
        recipe), ra_env_param_rows -- and, once the last launch has started the episodes, the randomizers, the reach goals' forward and the env kernel over the
        `reobserve` codes of those rows.  No readback: the number of iterations is known here, every mask stays on the device."""
        dev = self.device
        if mask is None:
            act = torch.ones(self.B, dtype=torch.bool, device=dev)
        else:
            assert mask.shape == (self.B,)
            if mask.device.type == "cpu" and not bool(mask.any()):      # (a mask that lives on the host: nothing to launch; a device mask is not read back -- its launches skip every env)
                return self.observe()
            act = mask.to(device=dev) != 0
        act32 = act.to(torch.int32)
        self.active_row.copy_(act)
        r = self.recipe
        r.active, r.sync_mode = _ptr(self.active_row), _native.RA_SYNC_FORCED_END
        both = self._row_stages()
        try:
            self._recipe_launch()
            r.sync_mode = _native.RA_SYNC_PIPELINED
            if self.param_rows is not None:
                self._param_rows_launch(both, self.active_row)
            iterations, stabilising = self.sync_reset_iterations(), max(int(self.stabilize_steps), 1)
            for it in range(iterations):
                # the envs of the mask run the stages in lockstep, so the host knows what the recipe's rows hold: `solver_active` is 0 for all of them while the
                # objects stabilise (no solver world launch: it would skip every env) and 1 afterwards, where the mask restricts that launch too (the row is 1 for
                # the live envs outside it)
                if it < stabilising and self.stabilize_steps <= 0 and self.scene_init is not None:
                    # a recorded start without stabilisation: the stage of zero steps is counted, not simulated -- the episode starts AT the recorded state, as on the
                    # host route; where it is the recipe's last launch, the forward of _observe_sync that the last physics launch would have carried
                    if it == iterations - 1:
                        self.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=FLAG_FULL_FORWARD, active=act32)
                else:      # every env of these launches is inside its recipe (`hold`): none takes the zero action handed over, unwrapped so that no live env's filter moves
                    self._physics(self._zero_action, active=act32, phase="main" if it < stabilising else None, recipe_rows=True)
                self._recipe_launch()
                if self.param_rows is not None:
                    self._param_rows_launch(both, self.active_row)
        finally:
            r.active, r.sync_mode = None, _native.RA_SYNC_PIPELINED
        self._finish_recipe_launch(self.active_row)      # the last launch started the episodes (the envs of the mask run the stages in lockstep)
        self.episode_started.masked_fill_(act, False)      # (as after the host recipe: the flag belongs to the step calls of a pipelined env)
        self.ended_rows = np.zeros(0, dtype=np.int64)
        return self.observe()

    def reset(self, mask: Optional[torch.Tensor] = None, on_device: Optional[bool] = None):
        """RobotEnv.reset -> RearrangeEnv._reset (common/base.py:897-932): robot start pose, object rotations + grid placement, stabilisation
        (100 simulation steps), n_random_initial_steps of one random action then 100 zero-action steps, tracker reset, first goal.
        `on_device` (`_on_device`): the same recipe in ra_recipe_kernel with its draws (`_reset_device`: no readback of the mask, no host sampling) instead of the
        host recipe below."""
        self._next_mask_step()
        if self._on_device(on_device):
            return self._reset_device(mask)
        rows = np.arange(self.B) if mask is None else np.nonzero(mask.cpu().numpy())[0]
        if len(rows) == 0:
            return self.observe()
        dev = self.device
        idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
        active = self._mask_of(idx, torch.int32)
        if self.pipelined:       # a synchronous reset ends whatever recipe those envs were in
            self._stage[rows] = _native.RA_STAGE_LIVE; self._left[rows] = 0
            if self.device_reset:
                self.stage[idx] = _native.RA_STAGE_LIVE; self.left[idx] = 0
            self.hold[idx] = 0; self.hold_ctrl[idx] = 0; self.frozen[idx] = _native.RA_OBS_STEP; self.solver_active[idx] = 1; self.resetting[idx] = False; self.episode_started[idx] = False
            self.nticks[idx] = 2; self._nticks_host = None
        yaw = self._begin_episode_state(rows, idx)
        # stabilize_objects (common/utils.py:76-92): the objects' dof damping is lowered to 1e-3 while they settle and restored afterwards -- with per-env parameter
        # rows; without them the model's own damping (0.01) stays (blocks at rest on the table need no help; mesh objects settle a little slower)
        self._set_object_damping(idx, self.stabilize_object_damping)
        for _ in range(self.stabilize_steps):
            self.sim.env_step(nforward_ticks=1, active=active)
        self._set_object_damping(idx, None)
        # _randomize_robot_initial_position (common/base.py:498-510)
        if self.n_random_initial_steps >= 1:
            act = torch.zeros(self.B, self.launch_action_dim, device=dev)
            act[idx] = torch.tensor(self._rng.uniform(-1, 1, (len(rows), self.launch_action_dim)).astype(np.float32), device=dev)
            for _ in range(self.n_random_initial_steps):
                self._recipe_physics(act, active)
            for _ in range(self.settle_steps):
                self._recipe_physics(self._zero_action, active)
        self._start_episode(rows, idx, yaw)
        self.sim.env_step(nsubsteps=0, nforward_ticks=1, flags=FLAG_FULL_FORWARD, active=active)       # the forward of _observe_sync, after the goal is written
        # the first observation of the new episodes: the env kernel for exactly those rows (observation + gripper hand-over, zeroed reward / done, the success count
        # the first step's goal reward is measured from); the rows of everybody else -- and the reward / done / info tensors their last step() returned -- stay
        self._reobserve(rows, np.zeros(0, dtype=np.int64))
        return self.observe()

    def _start_episode(self, rows, idx, yaw):
        """The end of the reset recipe for the envs `rows` (`idx`: the same as a device index), whose objects were placed with the yaws `yaw`: tracker reset and the
        first goal (robot_env.py:780-792; ObjectStateGoal.next_goal; randomize_goal_rot: _next_goal)."""
        for f in (self.t, self.steps, self.ssl, self.successes, self.consecutive, self.ema_t):
            f[idx] = 0
        self.ema_value[idx] = 0; self.action_ema[idx] = 0          # SmoothActionWrapper.reset: a fresh filter, action_ema = 0
        self._randomize_simulation(idx)                               # simulation_randomizer.randomize AFTER _reset (robot_env.py:779-783)
        self._make_goal(rows, yaw, first=True)

    def _regoal(self, rows):
        """ObjectStateGoal.next_goal for the live envs `rows`: the next goal, from the yaws of the one they have"""
        yaw = self.goal_rot[torch.as_tensor(rows, device=self.device, dtype=torch.long), :, 2].cpu().numpy().astype(np.float64)
        self._make_goal(rows, yaw, first=False)

    # ------------------------------------------------------------------ pipelined resets
    def _reobserve(self, started, regoaled):
        """The observation rows of these envs again, after their goal changed, every other env skipped by the env kernel: `started` (first observation of a new
        episode: reward 0, done 0) and `regoaled` (live envs with a new goal: the observation entries only, this step's reward / done / flags stay)."""
        if len(started) + len(regoaled) == 0:
            return
        saved = self.frozen.clone()
        self.frozen.fill_(_native.RA_OBS_SKIP)
        self.frozen[torch.as_tensor(started, device=self.device, dtype=torch.long)] = _native.RA_OBS_EPISODE_START
        self.frozen[torch.as_tensor(regoaled, device=self.device, dtype=torch.long)] = _native.RA_OBS_NEW_GOAL
        self._post(frozen=self.frozen)
        self.frozen.copy_(saved)

    def _advance_recipes(self):
        """After the step's three launches: start the reset recipe of the envs whose episode ended, move the envs inside it one step on (stabilise ->
        random action -> settle -> episode start: tracker reset, first goal, first observation), give the live envs that reached their goal a new one."""
        dev = self.device
        done = self.done.cpu().numpy()                       # (the one host synchronisation of a step)
        newgoal = self.goal_reset.cpu().numpy()
        self.episode_started.zero_()
        st, left = self._stage, self._left
        # ---- envs inside the recipe: this step counted
        inside = st != _native.RA_STAGE_LIVE
        left[inside] -= 1
        nxt = np.nonzero(inside & (left <= 0))[0]
        started = []
        was = st[nxt].copy()
        for stage in (_native.RA_STAGE_STABILISE, _native.RA_STAGE_RANDOM_ACTION, _native.RA_STAGE_SETTLE):
            rows = nxt[was == stage]
            if len(rows) == 0:
                continue
            idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
            if stage == _native.RA_STAGE_STABILISE:
                self._set_object_damping(idx, None)                     # stabilize_objects restores the objects' damping
            if stage == _native.RA_STAGE_STABILISE and self.n_random_initial_steps >= 1:         # -> one random action for n_random_initial_steps steps
                st[rows], left[rows] = _native.RA_STAGE_RANDOM_ACTION, self.n_random_initial_steps
                self.scripted[idx] = torch.tensor(self._rng.uniform(-1, 1, (len(rows), self.launch_action_dim)).astype(np.float32), device=dev)
                self.solver_active[idx] = 1; self.hold_ctrl[idx] = 0
            elif stage == _native.RA_STAGE_RANDOM_ACTION:                                            # -> zero action while everything settles
                st[rows], left[rows] = _native.RA_STAGE_SETTLE, self.settle_steps
                self.scripted[idx] = 0
            else:                                                       # -> the episode starts
                started.append(rows)
        if started:
            rows = np.concatenate(started)
            idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
            st[rows], left[rows] = _native.RA_STAGE_LIVE, 0
            self.hold[idx] = 0; self.scripted[idx] = 0; self.frozen[idx] = _native.RA_OBS_STEP; self.solver_active[idx] = 1; self.hold_ctrl[idx] = 0
            self.resetting[idx] = False; self.episode_started[idx] = True
            self._start_episode(rows, idx, self._yaw[rows])
        # ---- live envs with a reached goal: ObjectStateGoal.next_goal (what reset_goals() does on request)
        grows = np.nonzero(newgoal.astype(bool) & (st == _native.RA_STAGE_LIVE) & ~done.astype(bool))[0]     # (an episode that ends on the same step keeps the reached goal's entries in its terminal observation: ra_recipe_kernel)
        if len(grows):
            self._regoal(grows)
        if self.reach:      # (one forward and one re-observation for the rows that start and the rows with a new goal)
            self._forward_rows(np.concatenate(started + [grows]))
        self._reobserve(np.concatenate(started) if started else np.zeros(0, dtype=np.int64), grows)
        # ---- episodes that ended on this step: their recipe begins (the returned observation / reward / done are the terminal ones)
        rows = np.nonzero(done.astype(bool) & (st == _native.RA_STAGE_LIVE))[0]
        self.ended_rows = rows                              # (envs/rearrange/ycb.py hands these slots out again, to other envs of the batch)
        if len(rows):
            idx = torch.as_tensor(rows, device=dev, dtype=torch.long)
            self._yaw[rows] = self._begin_episode_state(rows, idx)
            self._set_object_damping(idx, self.stabilize_object_damping)
            st[rows], left[rows] = _native.RA_STAGE_STABILISE, self.stabilize_steps
            self.hold[idx] = 1; self.scripted[idx] = 0; self.frozen[idx] = _native.RA_OBS_IN_RECIPE; self.solver_active[idx] = 0; self.hold_ctrl[idx] = 1
            self.resetting[idx] = True
            if self.stabilize_steps <= 0:        # (degenerate configuration: straight to the next stage on the following step)
                left[rows] = 1
        # controller ticks of the NEXT step's main-world launch: two for live envs, one inside the recipe, two on the recipe's last step (see _physics)
        last_stage = _native.RA_STAGE_SETTLE if self.n_random_initial_steps >= 1 else _native.RA_STAGE_STABILISE
        # (reach: one on the recipe's last step -- its goal moves the object, the forward of _observe_sync comes after that, _forward_rows)
        want = np.where(st != _native.RA_STAGE_LIVE, np.where((st == last_stage) & (left <= 1) & (not self.reach), 2, 1), 2).astype(np.int32)
        if not np.array_equal(want, getattr(self, "_nticks_host", None)):
            self._nticks_host = want
            self.nticks.copy_(torch.as_tensor(want, device=dev))

    def _advance_recipes_device(self):
        """`_advance_recipes` without the host: the recipe kernel (stage machine, begin-of-episode state, placement and goal sampling), one launch on its masks for the
        per-env parameter rows (the block restored for an episode that ended = `_recreate_sim`'s fresh model, mjData.xfrc_applied at zero among it; stabilize_objects'
        damping change; the unused objects' parking rows), and `_finish_recipe_launch`: the simulation randomizers for the envs whose episode starts, the env kernel
        once more over the `reobserve` codes."""
        self._recipe_launch()
        if self.param_rows is not None:
            self._param_rows_launch(self._row_stages())
        self._finish_recipe_launch()
        self.ended_rows = np.zeros(0, dtype=np.int64)

    def _set_object_damping(self, idx, value):
        """RearrangeSimulationInterface.set_object_damping for the envs `idx` (simulation/base.py:753-770): `value` on the objects' six dofs, None = the model's own."""
        if not self.per_env_parameters:
            return
        d = self.sim.params["dof_damping"]
        cols = self.obj_dofs
        d[idx[:, None], cols[None, :]] = self._param_defaults["dof_damping"][cols] if value is None else float(value)
        if self.max_num_objects is not None:      # (a parked object keeps its own damping)
            self._apply_parking(self._mask_of(idx))

    def _mask_of(self, idx, dtype=torch.bool):
        """[B] mask of the envs `idx` (rows or a device index): bool, or int32 as the launches' `active` argument"""
        mask = torch.zeros(self.B, dtype=dtype, device=self.device)
        mask[torch.as_tensor(idx, device=self.device, dtype=torch.long)] = 1
        return mask

    def _apply_parking(self, mask):
        """Per-env object counts: what holds the unused objects of the envs `mask` ([B] bool, a device mask: tensor ops, no readback) at their parking poses -- their
        weight cancelled by a force at the body's centre of mass, `xfrc_applied` = - body_mass x gravity from THAT env's rows (so it has to follow the block's restore
        and the randomizers, which may change both), and the dof damping PARK_DAMPING on their six dofs (so it has to follow stabilize_objects' damping changes).  The
        poses themselves and zero velocities are written where the episode begins (`_begin_episode_state`, ra_recipe_kernel)."""
        P, N = self.sim.params, self.N
        unused = (self._slot[None, :] >= self.num_active[:, None]) & mask[:, None]                       # [B, N]
        x = P["xfrc_applied"]
        force = -P["body_mass"][:, self._obj_bodies, None] * P["gravity"][:, None, :]                     # [B, N, 3]
        cur = x[:, self._obj_bodies]
        cur[..., :3] = torch.where(unused[..., None], force, cur[..., :3])
        x[:, self._obj_bodies] = cur
        d = P["dof_damping"]
        dc = d[:, self.obj_dofs]
        d[:, self.obj_dofs] = torch.where(unused.repeat_interleave(6, dim=1), torch.full_like(dc, PARK_DAMPING), dc)

    def set_object_perm_next(self, perm, rows=None):
        """object_pool: the permutation of the NEXT episode of the envs `rows` (default: every env), checked: [M] or one row per env, each a permutation of 0..M-1 --
        slot i of the env will be world object perm[i], the first `num_objects` slots in use -- or all -1 = sampled by the recipe kernel; `None` or -1: sample
        everywhere.  Anything else raises ValueError.  (A row written to `self.object_perm_next` directly, as a curriculum on the device does, is checked where it is
        latched: one that is no permutation is replaced by a sampled one.)"""
        if not self.object_pool:
            raise ValueError("set_object_perm_next: the env was built without object_pool")
        M = self.N
        t = torch.as_tensor(object_perm_rows(perm, M), device=self.device)
        if rows is None:
            self.object_perm_next.copy_(t.expand(self.B, M) if t.dim() == 1 else t)
        else:
            self.object_perm_next[torch.as_tensor(rows, device=self.device, dtype=torch.long)] = t

    def set_object_material_next(self, names_or_indices, rows=None):
        """material_names: the material of every slot in the NEXT episodes of the envs `rows` (default: every env), checked: names of envs/rearrange/materials.py or
        indices into its MATERIAL_NAMES, -1 / None = drawn from `material_names`; one entry, [N], or one row per env.  The pin stays until it is written again.  With
        `object_groups` the slots of a group take the material of the group's lowest slot.  Anything else raises ValueError.  (A value written to
        `self.object_material_next` directly that names no material is drawn.)"""
        if not self.materials_on:
            raise ValueError("set_object_material_next: the env was built with material_names=%r (the compiled world's own material only)" % (self.material_names,))
        t = torch.as_tensor(materials.material_indices(names_or_indices, self.N), device=self.device)
        if rows is None:
            self.object_material_next.copy_(t.expand(self.B, self.N) if t.dim() == 1 else t)
        else:
            self.object_material_next[torch.as_tensor(rows, device=self.device, dtype=torch.long)] = t

    def object_set(self):
        """object_pool: [B, num_objects] the world objects on every env's table, in slot order (a host query: a readback)"""
        if not self.object_pool:
            raise ValueError("object_set: the env was built without object_pool")
        return self.object_perm[:, :self.num_objects_initial].cpu().numpy().astype(np.int64)

    def set_num_objects_next(self, counts, rows=None):
        """The object count of the NEXT episode of the envs `rows` (default: every env), checked: an int or one per env, each in 1..max_num_objects.  (Writing
        `self.num_objects_next` directly, as a curriculum on the device does, is clamped to that range where it is latched.)"""
        if self.object_pool:
            raise NotImplementedError("set_num_objects_next: object_pool (per-env object subsets) keeps one count for the whole batch; per-env counts together with subsets are not built")
        if self.max_num_objects is None:
            raise ValueError("set_num_objects_next: the env was built without max_num_objects")
        c = np.asarray(counts)
        if c.size == 0 or not np.all(c == np.round(c)) or c.min() < 1 or c.max() > self.N:
            raise ValueError("num_objects_next %r is outside 1..max_num_objects=%d" % (np.asarray(counts).tolist(), self.N))
        t = torch.as_tensor(c.astype(np.int32), device=self.device)
        if rows is None:
            self.num_objects_next.copy_(t.expand(self.B) if t.dim() == 0 else t)
        else:
            self.num_objects_next[torch.as_tensor(rows, device=self.device, dtype=torch.long)] = t

    def _randomize_simulation(self, idx):
        """`randomization.simulation_randomizer.randomize(mj_sim, random_state)` for the envs `idx` (robot_env.py:779-783): every randomizer draws new values of its
        model field from the model's own (the block was restored at the start of the reset), on the device."""
        if not self.randomizers:
            return
        mask = self._mask_of(idx)
        self._randomize(mask)
        if self.max_num_objects is not None:      # (gravity and body masses may have changed: the cancelling force follows them)
            self._apply_parking(mask)

    def _aabb_half(self, yaw, n=None):
        """half extents [.., N, 3] of the objects' bounding boxes after a rotation by `yaw` [.., N] about z (`n`: of the first n objects, `yaw` [.., n])"""
        return yawed_half(self.obj_half[:n], yaw)

    def _observe_only(self, rows=None):
        """The observation rows of `rows` (default: everybody) from the state as it is, without a step: observation entries, gripper hand-over, zeroed
        reward / done, and -- as `_observe_sync` does through `update_goal_info` -- the success count the next step's goal reward is measured from."""
        self._reobserve(np.arange(self.B) if rows is None else np.asarray(rows), np.zeros(0, dtype=np.int64))

    def reset_goals(self, on_device: Optional[bool] = None):
        """`reset_goal` for the envs the tracker flagged (robot_env.py:893-909): a new ObjectStateGoal placement; host sampling, or (`on_device`, `_on_device`) one
        regoal-only launch of the recipe kernel over the live envs with `goal_reset` and not `done`, the reach goals' forward, the env kernel over the `reobserve` codes."""
        if self._on_device(on_device):
            r = self.recipe
            r.active, r.sync_mode = None, _native.RA_SYNC_REGOAL_ONLY
            try:
                self._recipe_launch()
            finally:
                r.sync_mode = _native.RA_SYNC_PIPELINED
            self._finish_recipe_launch(started=False)
            return
        rows = np.nonzero(self.goal_reset.cpu().numpy())[0]
        if len(rows) == 0:
            return
        self._regoal(rows)
        if self.reach:
            self._forward_rows(rows)
        self._reobserve(np.zeros(0, dtype=np.int64), rows)      # robot_env.py:893-909: the observation returned after a goal reset carries the new goal

    def sync(self):
        self.sim.sync()


def build_simulation_randomizers(model, params: Optional[dict] = None):
    """`RearrangeEnv.build_simulation_randomizers` (common/base.py:1008-1092) on the batched randomizers of robogym_amd/randomization/sim.py: the same list, names,
    fields, prefixes, apply modes and coefficients; `params[name]` is the randomizer's parameter (what ADR controls in the reference; 0 = identity)."""
    from robogym_amd.randomization.sim import GenericSimRandomizer, GeomSolimpRandomizer, GeomSolrefRandomizer, GravityRandomizer, JointMarginRandomizer, PidRandomizer

    P = dict(params or {})
    A, names = model.arrays, model.names
    robot_jnt = [j for j, n in enumerate(names["joint"]) if n.startswith("robot0:")]
    robot_dof = [d for d in range(len(A["dof_jntid"])) if int(A["dof_jntid"][d]) in set(robot_jnt)]
    robot_body = [b for b, n in enumerate(names["body"]) if n.startswith("robot0:")]
    g = lambda name, default=(0.0, 0.0): P.get(name, default)
    G = GenericSimRandomizer
    out = [
        GravityRandomizer(param=float(np.atleast_1d(g("gravity", 0.0))[0])),
        JointMarginRandomizer(param=float(np.atleast_1d(g("jnt_margin", 0.0))[0])),
        G("dof_frictionloss_robot", "dof_frictionloss", "uncoupled_mean_variance", param=g("dof_frictionloss_robot"), ids=robot_dof),
        G("dof_damping_robot", "dof_damping", "uncoupled_mean_variance", param=g("dof_damping_robot"), ids=robot_dof),
        G("dof_armature_robot", "dof_armature", "uncoupled_mean_variance", param=g("dof_armature_robot"), ids=robot_dof),
        G("jnt_stiffness_robot", "jnt_stiffness", "variance_mean_additive", param=g("jnt_stiffness_robot"), coef=0.005, ids=robot_jnt, positive_only=True),
        G("body_pos_robot", "body_pos", "variance_additive", param=g("body_pos_robot", (0.0,)), coef=0.02, ids=robot_body),
    ]
    for name in ("pid_kp", "pid_ti", "pid_td", "pid_imax_clamp", "pid_error_deadband"):
        mean, std = (list(np.atleast_1d(g(name))) + [0.0, 0.0])[:2]
        out.append(PidRandomizer(name, mean=float(mean), std=float(std)))
    out += [
        G("actuator_forcerange", "actuator_forcerange", "uncoupled_mean_variance", param=g("actuator_forcerange")),
        GeomSolimpRandomizer(param=g("geom_solimp", (0.0,) * 6)),
        GeomSolrefRandomizer(param=g("geom_solref", (0.0,) * 4)),
        G("geom_margin", "geom_margin", "variance_additive", param=g("geom_margin", (0.0,)), coef=0.0005),
        G("geom_pos", "geom_pos", "variance_additive", param=g("geom_pos", (0.0,)), coef=0.002),
        G("geom_gap", "geom_gap", "max_additive", param=g("geom_gap", (0.0,)), coef=0.01),
        G("geom_friction", "geom_friction", "uncoupled_mean_variance", param=g("geom_friction")),
        G("body_mass", "body_mass", "uncoupled_mean_variance", param=g("body_mass")),
        G("body_inertia", "body_inertia", "variance_additive", param=g("body_inertia", (0.0,))),
    ]
    unknown = sorted(set(P) - {r.name for r in out})
    if unknown:
        raise KeyError("randomizer_params: no simulation randomizer named %s (known: %s)" % (", ".join(unknown), ", ".join(r.name for r in out)))
    return out


def action_bin_array(lower_bound, upper_bound, n_bins, spacing="linear"):
    """BinSpacing.get_bin_array (wrappers/util.py:17-33): the table DiscretizeActionWrapper maps a bin index through.  "linear": n_bins evenly spaced values;
    "exponential" (symmetric range, odd n_bins): -1, -1/2, -1/4, ... 0 ... 1/4, 1/2, 1 times the bound."""
    spacing = str(spacing).lower().split(".")[-1]
    if spacing == "linear":
        return np.linspace(lower_bound, upper_bound, n_bins)
    if spacing != "exponential":
        raise NotImplementedError("action_spacing %r" % spacing)
    assert lower_bound == -upper_bound and n_bins % 2 == 1, "Exponential binning is only supported on symmetric action space with an odd number of bins"
    half = np.array([2.0 ** (-n) for n in range(n_bins // 2)]) * lower_bound
    return np.concatenate([half, [0.0], -half[::-1]])


SUPPORTED_PARAMETERS = {"simulation_params", "robot_control_params", "n_random_initial_steps", "material_names"}
SUPPORTED_SIMULATION_PARAMS = {"num_objects", "max_num_objects", "penalty", "used_table_portion", "object_groups", "goal_distance_ratio", "goal_distance_min"}
SUPPORTED_ROBOT_CONTROL_PARAMS = {"max_position_change", "arm_reset_controller_error", "control_mode", "tcp_solver_mode"}
SUPPORTED_CONSTANTS = {"success_threshold", "successes_needed", "success_reward", "max_timesteps_per_goal_per_obj", "n_action_bins", "action_spacing", "use_goal_distance_reward",
                       "goal_reward_per_object", "normalize_mesh", "randomize", "sample_lam_low", "sample_lam_high", "mask_obs_outside_placement_area"}


def _control_mode_name(mode) -> str:
    """`ControlMode` value or name (robot_interface.py:9-20) -> "tcp+roll+yaw" | "tcp+wrist" | "joint"."""
    name = str(getattr(mode, "value", mode)).lower().split(".")[-1]
    if name in ("tcp+roll+yaw", "tcp_roll_yaw"):
        return "tcp+roll+yaw"
    if name in ("tcp+wrist", "tcp_wrist"):
        return "tcp+wrist"
    if name == "joint":
        return "joint"
    raise ValueError("control_mode %r is not one of the reference's ControlMode values (joint, tcp+roll+yaw, tcp+wrist; robot_interface.py:9-20)" % (mode,))


def _solver_mode_name(mode) -> str:
    """`TcpSolverMode` value or name (robot_interface.py:22-29) -> "mocap_ik" | "mocap"."""
    name = str(getattr(mode, "value", mode)).lower().split(".")[-1]
    if name in ("mocap_ik", "mocap"):
        return name
    raise ValueError("tcp_solver_mode %r is not one of the reference's TcpSolverMode values (mocap, mocap_ik)" % (mode,))


def _check_supported(parameters, sp, rc, constants):
    """A parameter or constant of the reference's env that this env does not implement is an error, not a silently ignored key (the reference's attrs classes reject
    unknown names the same way; the supported subset keeps the reference's names and meaning)."""
    for got, known, where in ((parameters, SUPPORTED_PARAMETERS, "parameters"), (sp, SUPPORTED_SIMULATION_PARAMS, "parameters.simulation_params"),
                              (rc, SUPPORTED_ROBOT_CONTROL_PARAMS, "parameters.robot_control_params"), (constants, SUPPORTED_CONSTANTS, "constants")):
        unknown = sorted(set(got) - known)
        if unknown:
            raise NotImplementedError("%s: %s not implemented by the batched rearrange env (supported: %s)" % (where, ", ".join(unknown), ", ".join(sorted(known))))
    _control_mode_name(rc.get("control_mode", "tcp+roll+yaw"))
    _solver_mode_name(rc.get("tcp_solver_mode", "mocap_ik"))


def goal_rot_args(goal_args, where="constants.goal_args", other=(), icp=False):
    """The constructor's keywords from the `GoalArgs` keys that concern the goal's orientation (goals/object_state.py:122-149): `rot_dist_type` (full / mod90 / mod180 /
    icp), `randomize_goal_rot`, `rot_randomize_type` ("z_axis" only: "block" and "full" need goal boxes for orientations that are no yaw), and icp's
    `icp_max_num_vertices`, `icp_error_threshold`, `icp_use_bbox_precheck`.  The last is accepted and has NO effect: the precheck compares current_state["bounding_box"]
    with goal_state["bounding_box"], and the reference fills BOTH from get_target_bounding_boxes_in_table_coordinates (goals/object_state.py:420-425 and 483-488) -- the
    IoU is 1 > 0.75, the ICP always runs.  `icp=True` (ycb.make_env) lets rot_dist_type "icp" and its three keys through; the block envs' surfaces keep refusing them by name.
    `soft_mask` / `mask_margin` (:159-161; the placement-area masks, acting with constants.mask_obs_outside_placement_area) pass through under their own names.
    A key outside these and `other` raises, named."""
    goal_args = dict(goal_args or {})
    icp_keys = ("icp_max_num_vertices", "icp_error_threshold", "icp_use_bbox_precheck")
    known = {"rot_dist_type", "randomize_goal_rot", "rot_randomize_type", "soft_mask", "mask_margin"} | set(other) | (set(icp_keys) if icp else set())
    unknown = sorted(set(goal_args) - known)
    if unknown:
        raise NotImplementedError("%s: %s not implemented by the batched rearrange env (supported: %s)" % (where, ", ".join(unknown), ", ".join(sorted(known))))
    out = {}
    if "rot_dist_type" in goal_args:
        allowed = [k for k in ROT_DIST_TYPES if icp or k != "icp"]
        if goal_args["rot_dist_type"] not in allowed:
            raise NotImplementedError("%s.rot_dist_type %r is not implemented by the batched rearrange env (%s)" % (where, goal_args["rot_dist_type"], ", ".join(allowed)))
        out["rot_dist_type"] = goal_args["rot_dist_type"]
    for k in icp_keys:
        if k in goal_args:
            out[k] = goal_args[k]
    if goal_args.get("rot_randomize_type", "z_axis") != "z_axis":
        raise NotImplementedError("%s.rot_randomize_type %r is not implemented by the batched rearrange env (z_axis)" % (where, goal_args["rot_randomize_type"]))
    if "randomize_goal_rot" in goal_args:
        out["randomize_goal_rot"] = bool(goal_args["randomize_goal_rot"])
    if "soft_mask" in goal_args:      # the placement-area masks' two keys (they act with constants.mask_obs_outside_placement_area)
        out["soft_mask"] = bool(goal_args["soft_mask"])
    if "mask_margin" in goal_args:
        out["mask_margin"] = float(goal_args["mask_margin"])
    return out


def group_args(sp, constants):
    """The constructor's group keywords from `simulation_params.object_groups` ("distinct" / "single" / "sample" / counts) and `constants.sample_lam_low / _high`."""
    out = {}
    if "object_groups" in sp:
        out["object_groups"] = sp["object_groups"]
    if "sample_lam_low" in constants or "sample_lam_high" in constants:
        out["sample_lam"] = (constants.get("sample_lam_low", SAMPLE_LAM[0]), constants.get("sample_lam_high", SAMPLE_LAM[1]))
    return out


def make_env_args(parameters, constants, starting_seed, apply_wrappers, num_objects, icp=False):
    """The constructor's keywords from the reference's `parameters` / `constants` -- what `make_env` here and in envs/rearrange/ycb.py share.  `num_objects`: the
    env's default count; `icp`: `goal_rot_args`.  A name outside the supported subset raises (`_check_supported`).  -> (keywords, simulation_params, constants): the
    two dicts as copies, `goal_args` taken out, for what a caller maps itself."""
    parameters, constants = dict(parameters or {}), dict(constants or {})
    sp, rc = dict(parameters.get("simulation_params", {})), dict(parameters.get("robot_control_params", {}))
    rot_args = goal_rot_args(constants.pop("goal_args", None), icp=icp)      # constants.goal_args: rot_dist_type, randomize_goal_rot (the task modules take their own keys out first)
    _check_supported(parameters, sp, rc, constants)
    args = dict(num_objects=sp.get("num_objects", num_objects), max_position_change=rc.get("max_position_change", 0.1), arm_reset_controller_error=rc.get("arm_reset_controller_error", True),
                n_random_initial_steps=parameters.get("n_random_initial_steps", 10), starting_seed=starting_seed, wrappers=bool(apply_wrappers),
                n_action_bins=constants.get("n_action_bins", 11), control_mode=rc.get("control_mode", "tcp+roll+yaw"), tcp_solver_mode=rc.get("tcp_solver_mode", "mocap_ik"))      # (+ pipelined_reset=True through **kw: episodes restart inside the step calls)
    if "action_spacing" in constants:
        args["action_spacing"] = constants["action_spacing"]
    if "material_names" in parameters:      # (None or an empty list: all five, as the reference's code loads them)
        args["material_names"] = parameters["material_names"]
    for k in ("success_threshold", "successes_needed", "success_reward", "max_timesteps_per_goal_per_obj", "use_goal_distance_reward", "goal_reward_per_object"):
        if k in constants:
            args[k] = constants[k]
    if "mask_obs_outside_placement_area" in constants:      # the placement-area masks (goal_args.soft_mask / mask_margin come through goal_rot_args)
        args["mask_obs_outside_placement_area"] = bool(constants["mask_obs_outside_placement_area"])
    for k in ("penalty", "used_table_portion"):      # (a given penalty dict replaces the default one as a whole, as the reference's attrs field does)
        if k in sp:
            args[k] = sp[k]
    args.update(group_args(sp, constants))
    args.update(rot_args)
    return args, sp, constants


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`BlockRearrangeEnv.build` surface (robot_env.py:1081-1089) for the batched env; `apply_wrappers` (default True, as in the reference) = the rearrange
    wrapper stack of common/base.py:986-996 (MultiDiscrete actions of `constants.n_action_bins` = 11 bins, action smoothing, reward clipping).  `parameters` / `constants` accept the subset this env
    implements (`SUPPORTED_*` below, and `constants.goal_args` {rot_dist_type, randomize_goal_rot, rot_randomize_type, soft_mask, mask_margin}: `goal_rot_args`); any other
    name raises NotImplementedError.  `constants.mask_obs_outside_placement_area`: the masks of the placement area and the masked observation keys (MASK_OBS_KEYS)."""
    args, sp, constants = make_env_args(parameters, constants, starting_seed, apply_wrappers, num_objects=5)
    for k in ("goal_distance_ratio", "goal_distance_min", "max_num_objects"):      # (max_num_objects: per-env object counts, num_objects the first count of every env)
        if k in sp:
            args[k] = sp[k]
    if constants.get("randomize", True) is False:    # RobotEnvConstants.randomize (robot_env.py:155): no simulation randomizers at all
        kw = dict(kw); kw.pop("randomizer_params", None)      # (the rows stay: stabilize_objects' damping change is not a randomizer)
    args.update(kw)
    return BatchedBlockRearrangeEnv(batch_size, device=device, **args)


def make_simple_env(*a, **kw):
    """make_env(apply_wrappers=False) (robot_env.py:1137-1139)"""
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)


class SingleEnvView:
    """B = 1 view of a batched rearrange env with the reference's types (robot_env.py:757-844): observations as numpy arrays without the batch dimension, the reward as a
    LIST of three floats (env, goal, success), a Python bool `done`, an info dict of Python scalars / arrays -- what a caller of `BlockRearrangeEnv` sees.  For porting
    single-env code and tests; not the fast path.  `step` takes the action of the env's mode: floats in [-1, 1] (`make_simple_env`) or bin indices (`make_env`)."""

    def __init__(self, env: BatchedBlockRearrangeEnv):
        assert env.B == 1
        self.env = env
        self.unwrapped = self
        self.mujoco_simulation = self.sim = env.sim
        self.action_shape = env.action_shape[1:]

    @staticmethod
    def _np(t):
        a = t[0].detach().cpu().numpy()
        return a.astype(np.float32) if a.dtype.kind == "f" else a

    def _obs(self, obs):
        return {k: self._np(v) for k, v in obs.items()}

    def reset(self):
        return self._obs(self.env.reset())

    def observe(self):
        return self._obs(self.env.observe())

    def reset_goals(self):
        self.env.reset_goals()
        return self.observe()

    def step(self, action):
        a = np.asarray(action)
        t = torch.as_tensor((a.astype(np.int64) if self.env.wrapped else a.astype(np.float32))[None], device=self.env.device)
        obs, reward, done, info = self.env.step(t.contiguous())
        one = lambda v: {k: one(x) for k, x in v.items()} if isinstance(v, dict) else (v[0].item() if v[0].dim() == 0 else self._np(v))      # (goal_dist: a dict of per-object rows)
        return self._obs(obs), [float(x) for x in reward[0]], bool(done[0]), {k: one(v) for k, v in info.items()}
