"""Golden vectors for the recorded scenes of the rearrange family (tests/golden/rearrange_holdout.npz): the reference's own holdout goal code, executed as it stands
on stubs (its import chain -- gym.envs.robotics, _jsonnet, trimesh, ... -- is not installed here); nothing of it is copied.

Four goal states of N = 2 objects: the recorded `holdouts/states/sample/goal_state_20200422_232013.npz` (its first object is rotated off the z axis) and three
random ones with cos(pitch) >= 0.1 (no gimbal orientation: the float32 mat2euler of the env kernel branches at another cos(pitch) than the float64 reference).
  goal_*   `HoldoutObjectStateGoal.next_goal` over `ObjectStateGoal.next_goal` (goals/holdout_object_state.py:45-63, goals/object_state.py:333-406) on a stub
           simulation: obj_pos, obj_rot, the object entries of qpos_goal.
  bbox     `rotate_bounding_box` as `get_block_bounding_box` calls it (common/utils.py:400-412, 1069-1093) for a block of half size 0.0254 in the goal's orientation.
  per rot_dist_type full / mod90 / mod180 and T = 8 current states per goal state: `HoldoutObjectStateGoal.goal_distance` (relative goal, obj_pos, obj_rot,
           rel_dist) and the per-object success bits of `RearrangeEnv._calculate_num_success` (common/base.py:824-841) under THRESHOLD.  Every distance keeps 1e-3
           from its threshold; for mod90 / mod180 the best candidate is > 1e-3 rad ahead of the second best.
Also copies the two recorded state files the tests start from, as data, to tests/golden/.  Needs /root/reference; the fixtures travel.

    python tools/gen_golden_rearrange_holdout.py
"""
import ast
import os
import shutil
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
np.float = float      # (the reference's rotation module predates numpy 1.24)
sys.path.insert(0, "/root/reference")
from robogym.utils import rotation  # noqa: E402

from gen_golden_rearrange_dominos import exec_source  # noqa: E402

REF = "/root/reference/robogym/envs/rearrange"
STATES = REF + "/holdouts/states"
COPIED = {"physics_tests/block_stacking4/initial_state_4_blocks_stacked.npz": "rearrange_holdout_initial_state_4_blocks_stacked.npz",
          "sample/goal_state_20200422_232013.npz": "rearrange_holdout_goal_state_20200422_232013.npz"}
THRESHOLD = {"obj_pos": 0.04, "obj_rot": 0.2, "rel_dist": 0.03}
N, T, HALF, MARGIN = 2, 8, 0.0254, 1e-3


def holdout_goal_class(osns):
    """HoldoutObjectStateGoal's methods as a subclass of the ObjectStateGoal compiled in `osns` (its zero-argument super() needs the real base)"""
    path = REF + "/goals/holdout_object_state.py"
    cls = [n for n in ast.parse(open(path).read()).body if isinstance(n, ast.ClassDef) and n.name == "HoldoutObjectStateGoal"][0]
    meths = [m for m in cls.body if isinstance(m, ast.FunctionDef) and m.name != "__init__"]
    assert sorted(m.name for m in meths) == ["_sample_next_goal_orientations", "_sample_next_goal_positions", "goal_distance", "next_goal"]
    for m in meths:
        m.returns = None
        for a in m.args.args:
            a.annotation = None
    module = ast.Module(body=[ast.ClassDef(name="HoldoutObjectStateGoal", bases=[ast.Name(id="ObjectStateGoal", ctx=ast.Load())], keywords=[], body=meths, decorator_list=[])],
                        type_ignores=[])
    ast.fix_missing_locations(module)
    ns = {"np": np, "ObjectStateGoal": osns["ObjectStateGoal"]}
    exec(compile(module, path, "exec"), ns)
    return ns["HoldoutObjectStateGoal"]


class StubSim:
    """What next_goal / goal_distance read of RearrangeSimulationInterface: the targets' poses as set, their Euler angles as get_target_rot makes them (mat2euler of the
    body's matrix), a qpos with the objects' free joints behind 10 robot entries"""

    def __init__(self):
        self.num_objects = self.num_groups = self.max_num_objects = N
        self.goal_pos_offset, self.goal_rot_weight = 0.0, 1.0
        self.qpos = np.arange(10 + 7 * N, dtype=np.float64) * 0.01
        self.mj_sim = types.SimpleNamespace(model=types.SimpleNamespace(get_joint_qpos_addr=lambda name: (10 + 7 * int(name[len("object"):-len(":joint")]), 0)))
        self.target_pos, self.target_quat = np.zeros((N, 3)), np.tile([1.0, 0, 0, 0], (N, 1))

    def set_target_pos(self, p):
        self.target_pos = np.array(p, dtype=np.float64)

    def set_target_quat(self, q):
        self.target_quat = np.array(q, dtype=np.float64)

    def forward(self):
        pass

    def get_target_pos(self, pad=True):
        return self.target_pos

    def get_target_rot(self, pad=True):
        return np.array([rotation.mat2euler(rotation.quat2mat(q)) for q in self.target_quat])

    def check_objects_off_table(self, pos):
        return np.zeros(len(pos), dtype=bool)

    def check_objects_in_placement_area(self, pos, margin=0.0, soft=False):
        return np.ones(len(pos), dtype=bool)


def make_goal(osns, Holdout, mode, pos, quat):
    g = Holdout.__new__(Holdout)
    g.mujoco_simulation = StubSim()
    g.args = types.SimpleNamespace(rot_dist_type=mode, randomize_goal_rot=True, stabilize_goal=False, mask_margin=0.02, soft_mask=False)
    g.rot_dist_func = (lambda a, b: osns["euler_angle_difference"](a, b, mode)) if mode != "full" else osns["full_euler_angle_difference"]
    g.goal_pos, g.goal_quat, g.goal_idx = [pos], [quat], 0
    return g


def random_quats(rng, n):
    """unit quaternions with cos(pitch) >= 0.1 in the reference's Euler convention"""
    out = []
    while len(out) < n:
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        if np.cos(rotation.quat2euler(q)[1]) >= 0.1 and abs(np.cos(rotation.quat2euler(q)[1])) < 0.98:
            out.append(q if q[0] >= 0 else -q)
    return np.array(out)


def small_rotation(rng, scale):
    v = rng.normal(size=3); v *= scale * rng.uniform(0.2, 1.0) / np.linalg.norm(v)
    a = np.linalg.norm(v)
    return np.concatenate([[np.cos(a / 2)], np.sin(a / 2) * v / a])


def candidate_gap(osns, mode, goal_rot, cur_rot):
    """how far the best parallel candidate of mod90 / mod180 is ahead of the second best (inf for full)"""
    if mode == "full":
        return np.inf
    tab = np.array(osns["PARALLEL_QUATS"] if mode == "mod90" else osns["PARALLEL_QUATS_180"])
    gap = np.inf
    for gr, cr in zip(goal_rot, cur_rot):
        qg, qc = rotation.euler2quat(gr), rotation.euler2quat(cr)
        mags = np.sort([rotation.quat_magnitude(rotation.quat_difference(rotation.quat_mul(qg, p), qc)) for p in tab])
        gap = min(gap, mags[1] - mags[0])
    return gap


def main():
    osns = exec_source(REF + "/goals/object_state.py", functions=("euler_angle_difference_single_pair", "euler_angle_difference", "full_euler_angle_difference"),
                       assigns=("PARALLEL_QUATS", "PARALLEL_QUATS_180"),
                       classes={"ObjectStateGoal": ("next_goal", "_update_simulation_for_next_goal", "_randomize_goal_orientation", "relative_goal", "goal_distance")},
                       ns={"np": np, "rotation": rotation, "dict": dict, "List": list, "Optional": None, "deepcopy": None})
    Holdout = holdout_goal_class(osns)
    utils = exec_source(REF + "/common/utils.py", functions=("rotate_bounding_box",), ns={"np": np, "quat2mat": rotation.quat2mat, "Tuple": tuple})
    base = exec_source(REF + "/common/base.py", classes={"RearrangeEnv": ("_calculate_num_success",)}, ns={"np": np})
    env = types.SimpleNamespace(constants=types.SimpleNamespace(success_threshold=THRESHOLD, goal_reward_per_object=1.0))
    num_success = lambda dist: base["RearrangeEnv"]._calculate_num_success(env, dist)

    rng = np.random.RandomState(20200422)
    sample = np.load(STATES + "/sample/goal_state_20200422_232013.npz")
    goal_pos, goal_quat = [sample["obj_pos"][:N].astype(np.float64)], [sample["obj_quat"][:N].astype(np.float64)]
    for c in range(3):      # three more orientations, the objects spread over the table top (one of them lowest: the anchor is not always object 0)
        p = np.array([1.3, 0.6, 0.52]) + rng.uniform(-0.15, 0.15, (N, 3)) * [1, 1, 0.2]
        goal_pos.append(p); goal_quat.append(random_quats(rng, N))
    goal_pos, goal_quat = np.array(goal_pos), np.array(goal_quat)
    C = len(goal_pos)
    out = dict(goal_state_pos=goal_pos, goal_state_quat=goal_quat, half=np.array(HALF), margin=np.array(MARGIN),
               **{"threshold_" + k: np.array(v) for k, v in THRESHOLD.items()})
    # ---- next_goal and the turned boxes
    g_pos, g_rot, g_qpos, bbox = [], [], [], []
    for c in range(C):
        g = make_goal(osns, Holdout, "full", goal_pos[c], goal_quat[c])
        goal = g.next_goal(None, {})
        assert goal["goal_valid"] and g.goal_idx == 0
        g_pos.append(goal["obj_pos"]); g_rot.append(goal["obj_rot"]); g_qpos.append(np.array([goal["qpos_goal"][10 + 7 * i:17 + 7 * i] for i in range(N)]))
        # get_block_bounding_box: the geom's box (at the body's origin) turned by quat_conjugate(mat2quat(xmat)), the body's orientation
        bbox.append([utils["rotate_bounding_box"]((np.zeros(3), np.full(3, HALF)), rotation.quat_conjugate(np.array(q)))[1] for q in goal_quat[c]])
    out.update(goal_obj_pos=np.array(g_pos), goal_obj_rot=np.array(g_rot), qpos_goal_obj=np.array(g_qpos), bbox=np.array(bbox))
    assert np.cos(out["goal_obj_rot"][..., 1]).min() >= 0.1
    # ---- current states: near the goal and away from it, rigidly shifted and not; the same states for the three modes, each kept MARGIN from every threshold
    cur_pos, cur_quat = np.zeros((C, T, N, 3)), np.zeros((C, T, N, 4))
    res = {m: {k: np.zeros((C, T, N, 3)) if k.startswith("rel_") and k != "rel_dist" else np.zeros((C, T, N)) for k in ("rel_pos", "rel_rot", "dist_pos", "dist_rot", "rel_dist", "success")}
           for m in ("full", "mod90", "mod180")}
    for c in range(C):
        goals = {m: make_goal(osns, Holdout, m, goal_pos[c], goal_quat[c]) for m in res}
        goal_state = {"obj_pos": out["goal_obj_pos"][c], "obj_rot": out["goal_obj_rot"][c]}
        t = 0
        while t < T:
            near = rng.rand(N) < 0.6
            shift = rng.uniform(-0.05, 0.05, 3) if t % 2 else np.zeros(3)
            p = goal_pos[c] + shift + np.where(near[:, None], rng.uniform(-0.012, 0.012, (N, 3)), rng.uniform(-0.08, 0.08, (N, 3)))
            q = np.array([rotation.quat_mul(small_rotation(rng, 0.12 if near[i] else 1.5), goal_quat[c][i]) for i in range(N)])
            if t == 0:      # at the goal up to a rigid shift: rel_dist 0 while obj_pos is not
                p, q = goal_pos[c] + np.array([0.1, -0.07, 0.0]), goal_quat[c].copy()
            cur = {"obj_pos": p, "obj_rot": rotation.normalize_angles(np.array([rotation.mat2euler(rotation.quat2mat(x)) for x in q]))}
            if np.cos(cur["obj_rot"][:, 1]).min() < 0.1:
                continue
            ok, got = True, {}
            for m, g in goals.items():
                d = g.goal_distance(goal_state, cur)
                got[m] = d
                for k in THRESHOLD:
                    ok = ok and np.abs(d[k] - THRESHOLD[k]).min() > MARGIN
                ok = ok and candidate_gap(osns, m, goal_state["obj_rot"], cur["obj_rot"]) > MARGIN
            if not ok:
                continue
            cur_pos[c, t], cur_quat[c, t] = p, q
            for m, d in got.items():
                r = res[m]
                r["rel_pos"][c, t], r["rel_rot"][c, t] = d["relative_goal"]["obj_pos"], d["relative_goal"]["obj_rot"]
                r["dist_pos"][c, t], r["dist_rot"][c, t], r["rel_dist"][c, t] = d["obj_pos"], d["obj_rot"], d["rel_dist"]
                r["success"][c, t] = [num_success({k: d[k][i:i + 1] for k in THRESHOLD}) for i in range(N)]
            t += 1
    out.update(cur_pos=cur_pos, cur_quat=cur_quat)
    for m, r in res.items():
        assert set(np.unique(r["success"])) == {0.0, 1.0}, m
        out.update({"%s_%s" % (m, k): v for k, v in r.items()})
    golden = os.path.join(HERE, "..", "tests", "golden")
    path = os.path.join(golden, "rearrange_holdout.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; success rate", {m: float(r["success"].mean()) for m, r in res.items()},
          "anchors", np.argmin(goal_pos[..., 2], -1).tolist())
    for src, dst in COPIED.items():      # recorded state files: data the reference's programs read, kept as fixtures
        shutil.copyfile(os.path.join(STATES, src), os.path.join(golden, dst))
        print("copied", dst, os.path.getsize(os.path.join(golden, dst)), "bytes")


if __name__ == "__main__":
    main()
