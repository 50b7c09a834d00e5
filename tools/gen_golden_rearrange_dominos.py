"""Golden vectors for rearrange/dominos and the goal-orientation axis of the rearrange family (tests/golden/rearrange_dominos.npz, rearrange_dominos_worlds.json).  The
reference's source is executed as it stands on stubs (its import chain -- gym.envs.robotics, _jsonnet, trimesh, ... -- is not installed here); nothing of it is copied.

  (a) `ObjectStateGoal.relative_goal / goal_distance` with rot_dist_type "mod90" and "mod180" (/root/reference/robogym/envs/rearrange/goals/object_state.py:25-64,
      492-599) on random current / goal Euler states of N = 5 objects: pure-yaw rows, rows near a goal turned by a parallel rotation, rows with exactly equal states.  Every
      pair is either identical or differs by > 1e-3 in a quaternion component AND has its best candidate > 1e-3 rad ahead of the second best (so the reference's
      np.allclose shortcut and near-ties play no part), and keeps 1e-3 from both success thresholds.  `a_tie_*`: exact-tie yaw cases (distance only).
  (b) the angle -> distance tables of envs/rearrange/tests/test_object_rotation.py:75-157, the angles read from that file, the distances evaluated by goal_distance.
  (c) `DominoStateGoal._sample_next_goal_positions` (goals/dominos.py) on a stub simulation, N in {1, 2, 5}, with the log of every draw.
  (d) `randomize_quaternion_along_z` (goals/object_state.py:71-85): draws, target quaternions in, quaternions out.
  worlds: the MJCF build of the domino world (envs/rearrange/xml.py build_dominos_xml) per array, as tools/gen_golden_blocks_worlds.py records the blocks worlds.

Needs /root/reference; the fixtures travel.

    python tools/gen_golden_rearrange_dominos.py
"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
np.float = float      # (the reference's rotation module predates numpy 1.24)
sys.path.insert(0, "/root/reference")
from robogym.utils import rotation  # noqa: E402

REF = "/root/reference/robogym/envs/rearrange"
THRESHOLD = {"obj_pos": 0.04, "obj_rot": 0.2}


def exec_source(path, functions=(), assigns=(), classes=None, ns=None):
    """The named top-level functions / assignments and the named methods of the named classes of `path`, compiled from its source and executed in `ns`."""
    tree = ast.parse(open(path).read())
    body = []
    for n in tree.body:
        if isinstance(n, ast.FunctionDef) and n.name in functions:
            n.returns = None
            for a in n.args.args + n.args.kwonlyargs:
                a.annotation = None
            body.append(n)
        elif isinstance(n, ast.Assign) and any(isinstance(t, ast.Name) and t.id in assigns for t in n.targets):
            body.append(n)
        elif isinstance(n, ast.ClassDef) and classes and n.name in classes:
            meths = [m for m in n.body if isinstance(m, ast.FunctionDef) and m.name in classes[n.name]]
            assert len(meths) == len(classes[n.name]), (n.name, [m.name for m in meths])
            for m in meths:
                m.returns = None
                for a in m.args.args + m.args.kwonlyargs:
                    a.annotation = None
            body.append(ast.ClassDef(name=n.name, bases=[], keywords=[], body=meths, decorator_list=[]))
    module = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(module)
    ns = dict(ns or {})
    exec(compile(module, path, "exec"), ns)
    return ns


class LoggedRandom:
    """np.random.RandomState whose scalar / vector draws are recorded"""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def random(self):
        v = self.rs.random_sample(); self.log.append(v); return v

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self.rs.uniform(low=low, high=high, size=size); self.log.extend(np.atleast_1d(v).tolist()); return v


def goal_layer(ns, mode, N=5):
    sim = types.SimpleNamespace(num_objects=N, num_groups=N, max_num_objects=N, goal_pos_offset=0.0, goal_rot_weight=1.0)
    g = ns["ObjectStateGoal"].__new__(ns["ObjectStateGoal"])
    g.mujoco_simulation, g.args = sim, types.SimpleNamespace(rot_dist_type=mode)
    g.rot_dist_func = (lambda a, b: ns["euler_angle_difference"](a, b, mode)) if mode != "full" else ns["full_euler_angle_difference"]
    return g


def candidate_gap(ns, mode, goal_rot, cur_rot):
    """per pair: the second smallest minus the smallest candidate magnitude, and the largest component difference of the two quaternions"""
    tab = ns["PARALLEL_QUATS"] if mode == "mod90" else ns["PARALLEL_QUATS_180"]
    q1, q2 = rotation.euler2quat(goal_rot), rotation.euler2quat(cur_rot)
    gap, far = np.zeros(len(q1)), np.zeros(len(q1))
    for i in range(len(q1)):
        d = np.sort([rotation.quat_magnitude(rotation.quat_difference(rotation.quat_mul(q1[i], p), q2[i])) for p in tab])
        gap[i], far[i] = d[1] - d[0], np.abs(q1[i] - q2[i]).max()
    return gap, far


def cases_a(ns, mode, rng, T=96, N=5):
    g = goal_layer(ns, mode)
    tab = np.array(ns["PARALLEL_QUATS"] if mode == "mod90" else ns["PARALLEL_QUATS_180"])
    out = {k: [] for k in ("cur_pos", "cur_rot", "goal_pos", "goal_rot", "rel_pos", "rel_rot", "dist_pos", "dist_rot", "gap")}
    t = 0
    while t < T:
        cur_pos, goal_pos = rng.uniform(-0.3, 0.3, (N, 3)), rng.uniform(-0.3, 0.3, (N, 3))
        cur_rot, goal_rot = rng.uniform(-np.pi, np.pi, (N, 3)), rng.uniform(-np.pi, np.pi, (N, 3))
        kind = t % 6
        if kind == 1:                  # pure yaw (objects flat on the table)
            cur_rot[:, :2] = 0; goal_rot[:, :2] = 0
        elif kind in (2, 3):           # at the goal up to a parallel rotation and a small turn; kind 2: every object inside both thresholds
            small = rotation.quat_from_angle_and_axis(rng.uniform(0.01, 0.15 if kind == 2 else 0.4, N), rng.normal(size=(N, 3)))
            q = rotation.quat_mul(rotation.quat_mul(rotation.euler2quat(goal_rot), tab[rng.randint(len(tab), size=N)]), small)
            cur_rot = rotation.quat2euler(q)
            cur_pos = goal_pos + rng.uniform(-0.02, 0.02, (N, 3))
        elif kind == 4:                # exactly equal states
            cur_rot, cur_pos = goal_rot.copy(), goal_pos.copy()
        res = g.goal_distance({"obj_pos": goal_pos, "obj_rot": goal_rot}, {"obj_pos": cur_pos, "obj_rot": cur_rot})
        gap, far = candidate_gap(ns, mode, goal_rot, cur_rot)
        same = np.all(goal_rot == cur_rot, axis=-1)
        keep = same | ((far > 1e-3) & (gap > 1e-3))
        clear = (np.abs(res["obj_pos"] - THRESHOLD["obj_pos"]) > 1e-3) & (np.abs(res["obj_rot"] - THRESHOLD["obj_rot"]) > 1e-3)
        if not (keep.all() and clear.all()):
            continue
        for k, v in (("cur_pos", cur_pos), ("cur_rot", cur_rot), ("goal_pos", goal_pos), ("goal_rot", goal_rot), ("rel_pos", res["relative_goal"]["obj_pos"]),
                     ("rel_rot", res["relative_goal"]["obj_rot"]), ("dist_pos", res["obj_pos"]), ("dist_rot", res["obj_rot"]), ("gap", gap)):
            out[k].append(np.array(v))
        t += 1
    return {k: np.array(v) for k, v in out.items()}


def cases_tie(ns, mode, rng, T=16, N=5):
    """pure-yaw states whose yaw difference sits exactly between two candidates: the reference picks the first, in fp32 either may win -- the distance is the same"""
    g = goal_layer(ns, mode)
    step = np.pi / 4 if mode == "mod90" else np.pi / 2
    goal_rot, cur_rot = np.zeros((T, N, 3)), np.zeros((T, N, 3))
    goal_rot[..., 2] = rng.uniform(-1.0, 1.0, (T, N))
    cur_rot[..., 2] = goal_rot[..., 2] + step * rng.choice([-3, -1, 1, 3] if mode == "mod90" else [-1, 1], size=(T, N))
    pos = rng.uniform(-0.3, 0.3, (T, N, 3))
    dist = np.array([g.goal_distance({"obj_pos": pos[t], "obj_rot": goal_rot[t]}, {"obj_pos": pos[t], "obj_rot": cur_rot[t]})["obj_rot"] for t in range(T)])
    return dict(goal_rot=goal_rot, cur_rot=cur_rot, pos=pos, dist_rot=dist)


def tables_b(ns):
    """test_object_rotation.py's angle -> distance tables: the angles from its dict literals, the distances from goal_distance on a pure-yaw pair"""
    tree = ast.parse(open(REF + "/tests/test_object_rotation.py").read())
    out = {}
    for mode in ("mod90", "mod180", "full"):
        fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "test_%s_rotation_blocks" % mode][0]
        lit = [n.value for n in fn.body if isinstance(n, ast.Assign) and n.targets[0].id == "angles_to_dists"][0]
        table = eval(compile(ast.Expression(lit), "angles_to_dists", "eval"), {"np": np})
        angles = np.array(list(table))
        g = goal_layer(ns, mode, N=1)
        base = 0.3
        dist = np.array([g.goal_distance({"obj_pos": np.zeros((1, 3)), "obj_rot": np.array([[0, 0, base + a]])}, {"obj_pos": np.zeros((1, 3)), "obj_rot": np.array([[0, 0, base]])})["obj_rot"][0]
                         for a in angles])
        assert np.abs(dist - np.array(list(table.values()))).max() < 1e-6, (mode, dist, table)      # (the reference's own expectation)
        out["b_%s_angle" % mode], out["b_%s_dist" % mode], out["b_base_yaw"] = angles, dist, np.array(base)
    return out


def domino_cases(rng_seed=7):
    utils = exec_source(REF + "/common/utils.py", functions=("rotate_bounding_box",), ns={"np": np, "quat2mat": rotation.quat2mat, "Tuple": tuple})
    PlacementArea = __import__("collections").namedtuple("PlacementArea", ["offset", "size"])
    ns = exec_source(REF + "/goals/dominos.py", assigns=("MAX_RETRY",),
                     classes={"DominoStateGoal": ("_adjust_and_check_fit", "_create_new_domino_position_and_rotation", "_sample_next_goal_positions", "_set_target_quat")},
                     ns={"np": np, "rotation": rotation, "PlacementArea": PlacementArea})
    from robogym_amd.envs.rearrange.xml import domino_half_sizes

    table_pos, table_size = np.array([1.32, 0.75, 0.4]), np.array([0.4575, 0.6, 0.05324])      # (a stub table, near the blocks world's)

    class Sim:
        def __init__(self, N, ecc, mul, portion):
            self.num_objects, self.used_table_portion = N, portion
            self.simulation_params = types.SimpleNamespace(object_size=0.0254, domino_distance_mul=mul)
            self.half = domino_half_sizes(0.0254, ecc)
            self.target_quat = np.tile([1.0, 0, 0, 0], (N, 1))

        def set_target_quat(self, q):
            self.target_quat = np.array(q)

        def forward(self):
            pass

        def get_target_bounding_boxes(self):      # get_block_bounding_box: the geom's box turned by the body's orientation
            return np.array([utils["rotate_bounding_box"]((np.zeros(3), self.half), rotation.quat_conjugate(q.copy())) for q in self.target_quat])

        def get_table_dimensions(self):
            return table_pos, table_size, table_pos[2] + table_size[2]

        def get_placement_area(self):      # simulation/base.py:980-1010
            tsx, tsy = table_size[:2] * 2
            p = np.clip(self.used_table_portion, self.num_objects * 0.1, 1.0)
            w, h = 0.5 * tsx * p, 0.38 * tsy * p
            return PlacementArea(offset=(0.5 * tsx - w / 2.0, 0.44 * tsy - h / 2.0, 2 * table_size[2]), size=(w, h, 0.26))

    out = dict(c_table_pos=table_pos, c_table_size=table_size)
    setups = [(1, 1.5, 4.0, 1.0), (2, 1.5, 4.0, 1.0), (5, 1.5, 4.0, 1.0), (5, 2.5, 4.0, 1.0), (5, 1.5, 4.5, 1.0), (2, 1.5, 16.0, 1.0), (5, 1.5, 30.0, 1.0)]      # (N, eccentricity, distance_mul, portion); the last never fits
    out["c_setups"] = np.array(setups)
    for si, (N, ecc, mul, portion) in enumerate(setups):
        sim = Sim(N, ecc, mul, portion)
        goal = ns["DominoStateGoal"].__new__(ns["DominoStateGoal"])
        goal.mujoco_simulation = sim
        area = sim.get_placement_area()
        logs, poss, yaws, valid = [], [], [], []
        for call in range(8 if mul < 20 else 1):
            rs = LoggedRandom(rng_seed + 100 * si + call)
            pos, ok = goal._sample_next_goal_positions(rs)
            q = sim.target_quat
            logs.append(np.array(rs.log)); poss.append(pos); yaws.append(2 * np.arctan2(q[:, 3], q[:, 0])); valid.append(ok)
        out["c%d_ndraw" % si] = np.array([len(l) for l in logs])
        out["c%d_draws" % si] = np.concatenate(logs)
        out["c%d_pos" % si], out["c%d_yaw" % si], out["c%d_valid" % si] = np.array(poss), np.array(yaws), np.array(valid)
        out["c%d_half" % si], out["c%d_area" % si] = sim.half, np.array([area.offset[:2], area.size[:2]])
    assert any((out["c%d_ndraw" % si] > 4).any() for si in range(len(setups))), "no setup shows retries"
    return out


def yaw_cases(osns, rng):
    T, N = 16, 5
    draws, q_in, q_out = [], [], []
    for t in range(T):
        tq = rotation.quat_from_angle_and_axis(rng.uniform(-np.pi, np.pi, N), np.array([[0, 0, 1.0]] * N))
        sim = types.SimpleNamespace(num_objects=N, get_target_quat=lambda pad=False, tq=tq: tq.copy())
        rs = LoggedRandom(1000 + t)
        q_out.append(osns["randomize_quaternion_along_z"](sim, rs)); draws.append(np.array(rs.log)); q_in.append(tq)
    return dict(d_draws=np.array(draws), d_quat_in=np.array(q_in), d_quat_out=np.array(q_out))


def main():
    osns = exec_source(REF + "/goals/object_state.py",
                       functions=("euler_angle_difference_single_pair", "euler_angle_difference", "full_euler_angle_difference", "_random_quat_along_z", "randomize_quaternion_along_z"),
                       assigns=("PARALLEL_QUATS", "PARALLEL_QUATS_180"), classes={"ObjectStateGoal": ("relative_goal", "goal_distance")},
                       ns={"np": np, "rotation": rotation, "dict": dict, "List": list})
    rng = np.random.RandomState(23)
    out = dict(parallel_quats=np.array(osns["PARALLEL_QUATS"]), parallel_quats_180=np.array(osns["PARALLEL_QUATS_180"]),
               pos_threshold=np.array(THRESHOLD["obj_pos"]), rot_threshold=np.array(THRESHOLD["obj_rot"]))
    for mode in ("mod90", "mod180"):
        out.update({"a_%s_%s" % (mode, k): v for k, v in cases_a(osns, mode, rng).items()})
        out.update({"a_tie_%s_%s" % (mode, k): v for k, v in cases_tie(osns, mode, rng).items()})
    out.update(tables_b(osns))
    out.update(domino_cases())
    out.update(yaw_cases(osns, rng))
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_dominos.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; retries per setup:", [out["c%d_ndraw" % si].tolist() for si in range(len(out["c_setups"]))])
    # ---- the MJCF build of the domino world
    from gen_golden_blocks_worlds import describe
    from robogym_amd.envs.rearrange.xml import build_dominos_xml

    worlds = {"%d_%g" % (n, e): describe(build_dominos_xml(n, domino_eccentricity=e).build()) for e in (1.5, 2.5) for n in (1, 2, 5)}
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_dominos_worlds.json")
    with open(path, "w") as f:
        json.dump(worlds, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
