"""Golden vectors for duplicated-object groups (tests/golden/rearrange_groups.npz): the REAL `ObjectStateGoal.relative_goal / goal_distance`
(/root/reference/robogym/envs/rearrange/goals/object_state.py:492-599, rot_dist_type "full") with `object_groups` that hold duplicates, `RearrangeEnv.
_calculate_num_success` (common/base.py:824-836) and `sample_group_counts` (common/utils.py:47-73), and the train goal's `place_targets_with_goal_distance_ratio` (+ `_place_objects`) and
`move_one_object_to_the_air_with_restrictions` (goals/train_state.py), their source executed as it stands on stubs, the way
tools/gen_golden_rearrange_goal.py does.  Needs /root/reference; only the arrays travel.

    python tools/gen_golden_rearrange_groups.py

Matching cases (positions in world coordinates, above the table): N in {2, 5, 8}; layouts [N], [2, 1, 2], [1, 4], [3, 3, 2] and all singletons; random poses, poses
with some objects NEAR a goal of their group that is not their own, the swapped pair, and four exact ties on a 1/8 grid.  The generator asserts in double that in
every greedy round of every case but the ties the runner-up distance exceeds the minimum by 1e-4 m, so an fp32 implementation has to make the same picks."""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
np.float = float      # (the reference's rotation module predates numpy 1.24)
sys.path.insert(0, "/root/reference")
from robogym.utils import rotation  # noqa: E402

REF = "/root/reference/robogym/envs/rearrange"
NMAX, MARGIN = 8, 1.0e-4
OFFSET = np.array([1.45, 0.77, 0.9])      # somewhere above the table: nothing touches


def _functions(path, names, cls=None):
    """the named top-level functions (or methods of `cls`) of a reference file, compiled from its own source"""
    tree = ast.parse(open(path).read())
    scope = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == cls][0].body if cls else tree.body
    got = [n for n in scope if isinstance(n, ast.FunctionDef) and n.name in names]
    assert len(got) == len(names), (path, names)
    for n in got:
        n.returns = None
        for a in n.args.args:
            a.annotation = None
    body = [ast.ClassDef(name=cls, bases=[], keywords=[], body=got, decorator_list=[])] if cls else got
    module = ast.Module(body=body, type_ignores=[])
    ast.fix_missing_locations(module)
    ns = {"np": np, "rotation": rotation, "dict": dict}
    exec(compile(module, path, "exec"), ns)
    return ns


GOAL = _functions(REF + "/goals/object_state.py", {"relative_goal", "goal_distance"}, cls="ObjectStateGoal")["ObjectStateGoal"]
FULL = _functions(REF + "/goals/object_state.py", {"full_euler_angle_difference"})["full_euler_angle_difference"]
ENV = _functions(REF + "/common/base.py", {"_calculate_num_success"}, cls="RearrangeEnv")["RearrangeEnv"]
SAMPLE = _functions(REF + "/common/utils.py", {"sample_group_counts"})["sample_group_counts"]


def reference_case(counts, cur_pos, cur_rot, goal_pos, goal_rot):
    n = len(cur_pos)
    ids = np.split(np.arange(n), np.cumsum(counts)[:-1])
    sim = types.SimpleNamespace(num_objects=n, num_groups=len(counts), max_num_objects=n, goal_pos_offset=0.0, goal_rot_weight=1.0,
                                object_groups=[types.SimpleNamespace(object_ids=list(map(int, g))) for g in ids])
    g = GOAL.__new__(GOAL)
    g.mujoco_simulation, g.args, g.rot_dist_func = sim, types.SimpleNamespace(rot_dist_type="full"), FULL
    out = g.goal_distance({"obj_pos": goal_pos, "obj_rot": goal_rot}, {"obj_pos": cur_pos, "obj_rot": cur_rot})
    env = types.SimpleNamespace(constants=types.SimpleNamespace(success_threshold={"obj_pos": 0.04, "obj_rot": 0.2}, goal_reward_per_object=1.0))
    nsucc = ENV._calculate_num_success(env, {"obj_pos": out["obj_pos"], "obj_rot": out["obj_rot"]})
    # the match itself: the goal of the object's group whose position gives the object's relative position
    match = np.zeros(n, dtype=np.int64)
    for grp in ids:
        for i in grp:
            hit = [j for j in grp if np.array_equal(goal_pos[j] - cur_pos[i], out["relative_goal"]["obj_pos"][i])]
            assert len(hit) == 1, (counts, i, hit)
            match[i] = hit[0]
    assert sorted(match) == list(range(n))
    return match, out["relative_goal"]["obj_pos"], out["relative_goal"]["obj_rot"], out["obj_pos"], out["obj_rot"], int(nsucc)


def min_margin(counts, cur_pos, goal_pos):
    """the smallest gap between the minimum and the runner-up over the greedy rounds of every group (double)"""
    n = len(cur_pos)
    gap = np.inf
    for grp in np.split(np.arange(n), np.cumsum(counts)[:-1]):
        dist = np.linalg.norm(cur_pos[grp][:, None] - goal_pos[grp][None], axis=-1)
        for _ in range(len(grp)):
            flat = np.sort(dist[np.isfinite(dist)])
            if len(flat) > 1:
                gap = min(gap, flat[1] - flat[0])
            i, j = np.unravel_index(np.argmin(dist), dist.shape)
            dist[i, :] = np.inf; dist[:, j] = np.inf
    return gap


def train_cases():
    """TrainStateGoal._sample_next_goal_positions' two steps (goals/train_state.py:87-113): `place_targets_with_goal_distance_ratio` with `_place_objects`,
    `_place_objects_trial`, `_is_valid_proposal` (common/utils.py) and `move_one_object_to_the_air_with_restrictions`, their source on a seeded RandomState; the
    `collision` package's boxes stand in as axis-aligned rectangles (what Poly.from_box makes).  Five yawed blocks on a table, ratio x (pickup, stack) probabilities."""
    import logging

    class Vector:
        def __init__(self, x, y):
            self.x, self.y = x, y

    class Poly:
        def __init__(self, c, w, h):
            self.c, self.w, self.h = c, w, h

        @staticmethod
        def from_box(c, w, h):
            return Poly(c, w, h)

    def collide(a, b):
        return abs(a.c.x - b.c.x) < 0.5 * (a.w + b.w) and abs(a.c.y - b.c.y) < 0.5 * (a.h + b.h)

    U = _functions(REF + "/common/utils.py", {"place_targets_with_goal_distance_ratio", "_place_objects", "_place_objects_trial", "_is_valid_proposal"})
    U.update(Poly=Poly, Vector=Vector, collide=collide)
    T = _functions(REF + "/goals/train_state.py", {"move_one_object_to_the_air_with_restrictions"})
    T["logger"] = logging.getLogger("gen")
    N = 5
    table_pos, table_size = np.array([1.3, 0.75, 0.2]), np.array([0.6, 0.6, 0.2])
    area = types.SimpleNamespace(offset=(0.3, 0.3, 0.4), size=(0.6, 0.45, 0.26))
    rows = []
    for ratio in (1.0, 0.5, 0.0):
        for pp, sp in ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0)):
            for rep in range(4):
                seed = len(rows) + 100
                rs = np.random.RandomState(seed)
                np.random.seed(seed)
                setup = np.random.RandomState(seed + 5000)
                yaw = setup.uniform(0, 2 * np.pi, N)
                half = np.stack([(np.abs(np.cos(yaw)) + np.abs(np.sin(yaw))) * 0.0254] * 2 + [np.full(N, 0.0254)], -1)
                centre = setup.uniform(-0.002, 0.002, (N, 3))
                bb = np.stack([centre, half], 1)
                shift = np.array([area.offset[0], area.offset[1], 0.0]) - table_size + table_pos
                obj = np.concatenate([setup.uniform(0.06, 0.4, (N, 2)) * [1.0, 0.9], np.full((N, 1), 0.4254)], -1) + shift
                before, valid = U["place_targets_with_goal_distance_ratio"](bb, (table_pos, table_size, 0.4), area, obj, ratio, 0.06, 100, 20, rs)
                assert valid
                after = T["move_one_object_to_the_air_with_restrictions"](before.copy(), (0.05, 0.25), 0.0254, rs, pickup_proba=pp, stacking_proba=sp, goal_distance_ratio=ratio)
                rows.append(dict(seed=seed, ratio=ratio, pickup=pp, stack=sp, centre=centre, half=half, obj=obj, before=before, after=after, next_draw=rs.uniform()))
    out = {"train_" + k: np.array([r[k] for r in rows]) for k in rows[0]}
    out.update(train_table_pos=table_pos, train_table_size=table_size, train_area_offset=np.array(area.offset), train_area_size=np.array(area.size))
    return out


def main():
    rng = np.random.RandomState(23)
    cases = []      # (kind, counts, cur_pos, cur_rot, goal_pos, goal_rot)
    layouts = {2: [[2], [1, 1]], 5: [[5], [2, 1, 2], [1, 4], [1] * 5], 8: [[8], [3, 3, 2], [1] * 8]}
    per_layout = {2: 8, 5: 10, 8: 10}
    for n, lays in layouts.items():
        for counts in lays:
            made = 0
            while made < per_layout[n]:
                cur_pos, goal_pos = rng.uniform(-0.3, 0.3, (n, 3)) + OFFSET, rng.uniform(-0.3, 0.3, (n, 3)) + OFFSET
                cur_rot, goal_rot = rng.uniform(-np.pi, np.pi, (n, 3)), rng.uniform(-np.pi, np.pi, (n, 3))
                if made % 5 == 0:       # pure yaw (objects flat on the table)
                    cur_rot[:, :2] = 0; goal_rot[:, :2] = 0
                if made % 2 == 1:       # some objects near a goal of their own group, in a shuffled assignment: the success count depends on the match
                    for grp in np.split(np.arange(n), np.cumsum(counts)[:-1]):
                        perm = rng.permutation(grp)
                        near = rng.rand(len(grp)) < 0.7
                        for i, j in zip(grp[near], perm[near]):
                            cur_pos[i] = goal_pos[j] + rng.uniform(-0.01, 0.01, 3)
                            cur_rot[i] = goal_rot[j] + rng.uniform(-0.03, 0.03, 3)
                if min_margin(counts, cur_pos, goal_pos) < MARGIN:
                    continue
                cases.append(("random", counts, cur_pos, cur_rot, goal_pos, goal_rot))
                made += 1
    # the swapped pair: each object exactly on the other's goal -- achieved with one group of two, not achieved with two groups of one
    gp = np.array([[1.25, 0.625, 0.875], [1.5, 0.875, 0.875]]); gr = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, -1.0]])
    for counts in ([2], [1, 1]):      # (both distances are exactly zero, on grid coordinates: a tie like those below, and either pick gives the same matching)
        cases.append(("swapped", counts, gp[::-1].copy(), gr[::-1].copy(), gp, gr))
    # exact ties: coordinates on a 1/8 grid, so equal distances are equal bit for bit in fp32 and fp64 alike; np.argmin takes the lowest flat index
    G = lambda *rows: np.array(rows, dtype=np.float64) / 8.0
    z = np.zeros((8, 3))
    ties = [
        # object 0 midway between the two goals, closer to both than object 1 -> (0, 0), which leaves goal 1 to object 1 (the highest index would swap them)
        ([2], G([10, 6, 7], [14, 6, 7]), G([10, 5, 7], [10, 7, 7])),
        # objects 1 and 2 equally far from goal 0 and closer than anything else -> (1, 0) before (2, 0)
        ([5], G([13, 8, 7], [10, 6, 7], [10, 4, 7], [14, 2, 8], [8, 9, 8]), G([10, 5, 7], [13, 5, 7], [12, 9, 8], [15, 3, 8], [9, 7, 8])),
        # object 3 equally far from goals 3 and 4 of its group [1, 4] -> goal 3
        ([1, 4], G([9, 4, 7], [11, 8, 7], [14, 3, 7], [12, 5, 7], [9, 9, 8]), G([9, 5, 7], [15, 8, 8], [14, 1, 8], [12, 6, 7], [12, 4, 7])),
        # the same distance in two different groups of [2, 1, 2]: (0, 1) and (3, 4) tie -> the order of the picks differs, the matching does not
        ([2, 1, 2], G([10, 4, 7], [14, 8, 7], [12, 6, 8], [9, 8, 7], [13, 2, 7]), G([13, 8, 8], [10, 5, 7], [12, 5, 8], [14, 3, 8], [9, 7, 7])),
    ]
    for counts, cp, gpos in ties:
        n = len(cp)
        cases.append(("tie", counts, cp, z[:n].copy(), gpos, z[:n].copy()))
    assert all(min_margin(*ties[q]) == 0.0 for q in (0, 1, 2))
    T = len(cases)
    A = dict(n=np.zeros(T, dtype=np.int32), kind=np.array([c[0] for c in cases]), groups=np.zeros((T, NMAX), dtype=np.int32), match=np.zeros((T, NMAX), dtype=np.int32),
             num_success=np.zeros(T, dtype=np.int32), **{k: np.zeros((T, NMAX, 3)) for k in ("cur_pos", "cur_rot", "goal_pos", "goal_rot", "rel_pos", "rel_rot")},
             dist_pos=np.zeros((T, NMAX)), dist_rot=np.zeros((T, NMAX)))
    for t, (kind, counts, cur_pos, cur_rot, goal_pos, goal_rot) in enumerate(cases):
        n = len(cur_pos)
        match, rel_pos, rel_rot, d_pos, d_rot, nsucc = reference_case(counts, cur_pos, cur_rot, goal_pos, goal_rot)
        A["n"][t] = n; A["groups"][t, :n] = np.repeat(np.arange(len(counts)), counts); A["match"][t, :n] = match; A["num_success"][t] = nsucc
        for k, v in (("cur_pos", cur_pos), ("cur_rot", cur_rot), ("goal_pos", goal_pos), ("goal_rot", goal_rot), ("rel_pos", rel_pos), ("rel_rot", rel_rot)):
            A[k][t, :n] = v
        A["dist_pos"][t, :n] = d_pos; A["dist_rot"][t, :n] = d_rot
    sw = [t for t in range(T) if A["kind"][t] == "swapped"]
    assert [int(A["num_success"][t]) for t in sw] == [2, 0] and list(A["match"][sw[0], :2]) == [1, 0]
    moved = sum(int((A["match"][t, :A["n"][t]] != np.arange(A["n"][t])).any()) for t in range(T))
    # sample_group_counts: 256 seeds, the counts and the generator's next draw (the replay has to consume the same draws)
    S = 256
    counts5, after5 = np.zeros((S, 5), dtype=np.int32), np.zeros(S)
    for seed in range(S):
        rs = np.random.RandomState(seed)
        c = SAMPLE(rs, 5, 1.0, 8.0)
        counts5[seed, :len(c)] = c; after5[seed] = rs.uniform()
    out = os.path.join(HERE, "..", "tests", "golden", "rearrange_groups.npz")
    np.savez_compressed(out, sample_counts=counts5, sample_next_draw=after5, **train_cases(), **A)
    print("wrote %s: %d matching cases (%d with a match that is not the identity; success counts %s), %d sampled count lists" % (
        out, T, moved, np.bincount(A["num_success"]).tolist(), S))


if __name__ == "__main__":
    main()
