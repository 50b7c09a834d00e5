"""Golden vectors for the rearrange block tasks (tests/golden/rearrange_tasks.npz, tests/golden/rearrange_task_keys.json): the REAL goal code of
/root/reference/robogym/envs/rearrange/goals/pickandplace.py (`move_one_object_to_the_air`), goals/object_stack_goal.py (`ObjectStackGoal._sample_next_goal_positions /
relative_goal / goal_distance`), goals/object_reach_goal.py (`ObjectReachGoal` / `DeterministicReachGoal._sample_next_goal_positions / current_state`) and
blocks_reach.py (`BlocksReachEnv._calculate_goal_distance_reward`), their source executed as it stands on a stub simulation and a recording random state.
The placement itself (`place_objects_in_grid` / `place_objects_with_no_constraint`) is stubbed with recorded positions: the repository's placement is
distribution-equivalent, not draw-for-draw, so the golden pins what each task does GIVEN the placement and its own draws.  Needs /root/reference; the fixtures travel.

    python tools/gen_golden_rearrange_tasks.py
"""
import ast
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/robogym/envs/rearrange"
np.float = float      # (the reference's rotation module predates numpy 1.24)
sys.path.insert(0, "/root/reference")
from robogym.utils import rotation  # noqa: E402


def load(path, funcs=(), classes=None, ns=None):
    """The named module-level functions and classes (with the named methods only) of a reference file, executed on their own in `ns`."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in funcs]
    for cname, (bases, meths) in (classes or {}).items():
        cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cname][0]
        keep = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in meths]
        assert len(keep) == len(meths), (cname, meths)
        for n in keep:
            n.returns = None
            for arg in n.args.args:
                arg.annotation = None
        body.append(ast.ClassDef(name=cname, bases=[ast.Name(id=b, ctx=ast.Load()) for b in bases], keywords=[], body=keep, decorator_list=[]))
    for n in body:
        if isinstance(n, ast.FunctionDef):
            n.returns = None
            for arg in n.args.args:
                arg.annotation = None
    m = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(m)
    exec(compile(m, path, "exec"), ns)
    return ns


class Recorder:
    """A numpy RandomState that records every draw the goal code takes: (method, result)."""

    def __init__(self, seed):
        self.rs, self.log = np.random.RandomState(seed), []

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self.rs.uniform(low, high, size); self.log.append(("uniform", v)); return v

    def randint(self, *a, **k):
        v = self.rs.randint(*a, **k); self.log.append(("randint", v)); return v

    def shuffle(self, x):
        self.rs.shuffle(x); self.log.append(("shuffle", list(x)))


def main():
    rng = np.random.RandomState(7)
    # ObjectStateGoal's rotation distance and base methods the task classes inherit (relative_goal / goal_distance of object_state.py)
    base = load(os.path.join(REF, "goals/object_state.py"), funcs=("full_euler_angle_difference",),
                classes={"ObjectStateGoal": ([], ("relative_goal", "goal_distance", "current_state"))}, ns={"np": np, "rotation": rotation, "dict": dict, "deepcopy": None, "ICP": None})
    T = 32
    out = {}
    # ---- pick-and-place: move_one_object_to_the_air on placements of 1 and 5 objects
    pnp = load(os.path.join(REF, "goals/pickandplace.py"), funcs=("move_one_object_to_the_air",), ns={"np": np})
    for N in (1, 5):
        pl, res, h, i = rng.uniform(1.0, 1.6, (T, N, 3)), [], [], []
        for t in range(T):
            rs = Recorder(100 + t)
            res.append(pnp["move_one_object_to_the_air"](pl[t].copy(), (0.05, 0.25), rs))
            assert [k for k, _ in rs.log] == ["uniform", "randint"]
            h.append(float(rs.log[0][1])); i.append(int(rs.log[1][1]))
        out.update({"pnp%d_placement" % N: pl, "pnp%d_height" % N: np.array(h), "pnp%d_index" % N: np.array(i), "pnp%d_goal" % N: np.array(res)})
    # ---- stack: _sample_next_goal_positions (placement stubbed with a recorded bottom position), relative_goal / goal_distance
    stack_ns = load(os.path.join(REF, "goals/object_stack_goal.py"), classes={"ObjectStackGoal": (["ObjectStateGoal"], ("_sample_next_goal_positions", "relative_goal", "goal_distance"))},
                    ns={"np": np, "rotation": rotation, "ObjectStateGoal": base["ObjectStateGoal"]})
    for N, fixed in ((2, False), (5, False), (5, True)):
        bottoms, perms, goals = rng.uniform(1.0, 1.6, (T, 1, 3)), [], []
        for t in range(T):
            bb = bottoms[t].copy()
            sim = types.SimpleNamespace(num_objects=N, simulation_params=types.SimpleNamespace(object_size=0.0254), get_object_bounding_boxes=lambda: np.zeros((N, 2, 3)),
                                        get_table_dimensions=lambda: None, get_placement_area=lambda: None, max_placement_retry=100, max_placement_retry_per_object=10)
            stack_ns["place_objects_with_no_constraint"] = lambda *a, **k: (bb.copy(), True)
            g = stack_ns["ObjectStackGoal"].__new__(stack_ns["ObjectStackGoal"])
            g.mujoco_simulation, g.fixed_order = sim, fixed
            rs = Recorder(200 + t)
            pos, ok = g._sample_next_goal_positions(rs)
            assert ok and [k for k, _ in rs.log] == ([] if fixed else ["shuffle"])
            perms.append(rs.log[0][1] if rs.log else list(range(N))); goals.append(pos)
        tag = "stack%d%s" % (N, "_fixed" if fixed else "")
        out.update({tag + "_bottom": bottoms, tag + "_order": np.array(perms), tag + "_goal": np.array(goals)})
    N = 2
    g = stack_ns["ObjectStackGoal"].__new__(stack_ns["ObjectStackGoal"])
    g.mujoco_simulation = types.SimpleNamespace(num_objects=N, num_groups=N, max_num_objects=N, goal_pos_offset=0.0, goal_rot_weight=1.0)
    g.args, g.rot_dist_func = types.SimpleNamespace(rot_dist_type="full"), base["full_euler_angle_difference"]
    cur_pos, goal_pos, grip = rng.uniform(1.0, 1.6, (T, N, 3)), rng.uniform(1.0, 1.6, (T, N, 3)), rng.uniform(1.0, 1.6, (T, 1, 3))
    cur_rot, goal_rot = rng.uniform(-np.pi, np.pi, (T, N, 3)), rng.uniform(-np.pi, np.pi, (T, N, 3))
    contact = (rng.rand(T, N, 2) < 0.3).astype(np.float64)
    keys, dist = None, {k: [] for k in ("obj_pos", "obj_rot", "gripper_pos", "grasped", "rel_obj_pos", "rel_obj_rot", "rel_gripper_pos")}
    for t in range(T):
        grasped = np.array([x[0] + x[1] for x in contact[t]])      # is_object_grasped
        d = g.goal_distance({"obj_pos": goal_pos[t], "obj_rot": goal_rot[t]}, {"obj_pos": cur_pos[t], "obj_rot": cur_rot[t], "gripper_pos": grip[t], "grasped": grasped})
        keys = (sorted(k for k in d if k != "relative_goal"), sorted(d["relative_goal"]))
        for k in ("obj_pos", "obj_rot", "gripper_pos", "grasped"):
            dist[k].append(d[k])
        for k in ("obj_pos", "obj_rot", "gripper_pos"):
            dist["rel_" + k].append(d["relative_goal"][k])
    out.update({"stackd_cur_pos": cur_pos, "stackd_cur_rot": cur_rot, "stackd_goal_pos": goal_pos, "stackd_goal_rot": goal_rot, "stackd_grip": grip, "stackd_contact": contact})
    out.update({"stackd_" + k: np.array(v) for k, v in dist.items()})
    task_keys = {"blocks_stack": {"goal_dist": keys[0], "relative_goal": keys[1]}}
    # ---- reach: ObjectReachGoal / DeterministicReachGoal._sample_next_goal_positions (set_object_pos recorded), current_state; the reach reward
    reach_ns = load(os.path.join(REF, "goals/object_reach_goal.py"), classes={"ObjectReachGoal": (["ObjectStateGoal"], ("_sample_next_goal_positions", "current_state")),
                                                                            "DeterministicReachGoal": (["ObjectReachGoal"], ("__init__", "_sample_next_goal_positions"))},
                    ns={"np": np, "ObjectStateGoal": base["ObjectStateGoal"], "GoalArgs": lambda: None})
    placed, moved, rgoal = rng.uniform(1.0, 1.6, (T, 1, 3)), [], []
    for t in range(T):
        pp = placed[t].copy()
        reach_ns["place_objects_with_no_constraint"] = lambda *a, **k: (pp.copy(), True)
        rec = []
        sim = types.SimpleNamespace(simulation_params=types.SimpleNamespace(target_height=0.1), set_object_pos=lambda p: rec.append(np.array(p, copy=True)), get_object_bounding_boxes=lambda: None,
                                    get_table_dimensions=lambda: None, get_placement_area=lambda: None, max_placement_retry=100, max_placement_retry_per_object=10)
        g = reach_ns["ObjectReachGoal"].__new__(reach_ns["ObjectReachGoal"]); g.mujoco_simulation = sim
        pos, ok = g._sample_next_goal_positions(Recorder(300 + t))
        assert ok and len(rec) == 1
        moved.append(rec[0]); rgoal.append(pos)
    out.update({"reach_placement": placed, "reach_moved": np.array(moved), "reach_goal": np.array(rgoal)})
    rec = []
    sim = types.SimpleNamespace(simulation_params=types.SimpleNamespace(target_height=0.1), set_object_pos=lambda p: rec.append(np.array(p, copy=True)))
    D = reach_ns["DeterministicReachGoal"]
    dg = D.__new__(D)
    reach_ns["ObjectReachGoal"].__init__ = lambda self, mujoco_simulation, args=None: setattr(self, "mujoco_simulation", mujoco_simulation)
    D.__init__(dg, sim)
    det = [dg._sample_next_goal_positions(None)[0] for _ in range(5)]
    out.update({"det_goal": np.array(det), "det_moved": np.array(rec)})
    site = rng.uniform(1.0, 1.6, (T, 3))
    cs = []
    for t in range(T):
        st = site[t]
        g = reach_ns["ObjectReachGoal"].__new__(reach_ns["ObjectReachGoal"])
        g.mujoco_simulation = types.SimpleNamespace(mj_sim=types.SimpleNamespace(data=types.SimpleNamespace(get_site_xpos=lambda name, st=st: st.copy() if name == "robot0:grip" else None)))
        c = g.current_state()
        cs.append(np.concatenate([c["obj_pos"], c["obj_rot"]], -1))
        task_keys.setdefault("blocks_reach", {"current_state": sorted(c)})
    out.update({"reach_site": site, "reach_current_state": np.array(cs)})
    env_ns = load(os.path.join(REF, "blocks_reach.py"), classes={"BlocksReachEnv": ([], ("_calculate_goal_distance_reward",))}, ns={"np": np})
    prev, cur = rng.uniform(0, 0.5, (T, 1)), rng.uniform(0, 0.5, (T, 1))
    rew = [env_ns["BlocksReachEnv"]._calculate_goal_distance_reward(None, {"obj_pos": prev[t], "obj_rot": np.ones(1)}, {"obj_pos": cur[t], "obj_rot": np.zeros(1)}) for t in range(T)]
    out.update({"reach_prev_dist": prev, "reach_cur_dist": cur, "reach_reward": np.array(rew)})
    # ---- per env: observation keys (RearrangeEnv._observe_simple: the same 24 for every task, tests/golden/rearrange_obs_keys.json) and goal_dist keys of info
    obs_keys = [k for k, _ in json.load(open(os.path.join(HERE, "..", "tests", "golden", "rearrange_obs_keys.json")))]
    for env in ("blocks_pickandplace", "blocks_stack", "blocks_reach", "ycb_pickandplace"):
        e = task_keys.setdefault(env, {})
        e["obs"] = obs_keys
        e.setdefault("goal_dist", ["obj_pos", "obj_rot"])
    np.savez_compressed(os.path.join(HERE, "..", "tests", "golden", "rearrange_tasks.npz"), **out)
    with open(os.path.join(HERE, "..", "tests", "golden", "rearrange_task_keys.json"), "w") as f:
        json.dump(task_keys, f, indent=1, sort_keys=True)
    print("wrote", len(out), "arrays; keys", json.dumps({k: v.get("goal_dist") for k, v in task_keys.items()}))


if __name__ == "__main__":
    main()
