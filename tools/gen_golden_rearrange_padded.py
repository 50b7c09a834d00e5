"""Golden vectors for per-env object counts (tests/golden/rearrange_padded.npz): the REAL `ObjectStateGoal.relative_goal / goal_distance`
(/root/reference/robogym/envs/rearrange/goals/object_state.py:492-599, rot_dist_type "full"), `RearrangeEnv._calculate_num_success` (common/base.py:824-848) and
`RobotEnv._is_successful` (robot_env.py:569-575) with `max_num_objects` > `num_objects`, their source executed as it stands on stubs, the way
tools/gen_golden_rearrange_goal.py does.  Needs /root/reference; only the arrays travel.

    python tools/gen_golden_rearrange_padded.py

The states are what the reference's observation hands those methods: `obj_pos` / `obj_rot` of goal and current state padded with zeros to max_num_objects
(simulation/base.py:1015-1024).  M in {3, 5, 8}, n in 1..M; layouts: every object its own group (the `goal_pos - obj_pos` path, which sees the padded rows) and, for
n >= 2, one group of all n objects (the matching path, which pads its output).  Per object one of four kinds -- inside both thresholds, position outside, rotation
outside, both outside -- so every case set has states on both sides of both thresholds; the generator asserts that every distance keeps 1e-3 from its threshold and that
every greedy round's runner-up exceeds the minimum by 1e-4 m, so an fp32 implementation has to decide the same way."""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_golden_rearrange_groups import ENV, FULL, GOAL, OFFSET, _functions, min_margin  # noqa: E402  (the reference's methods, compiled from their own source)

ROBOT = _functions("/root/reference/robogym/robot_env.py", {"_is_successful"}, cls="RobotEnv")["RobotEnv"]
MMAX, THR, KEEP, MARGIN = 8, {"obj_pos": 0.04, "obj_rot": 0.2}, 1.0e-3, 1.0e-4


def reference_case(M, counts, cur_pos, cur_rot, goal_pos, goal_rot):
    """the padded [M, ...] states through the reference's goal layer -> (rel_pos, rel_rot, dist_pos, dist_rot [M], num_success, is_successful)"""
    n = int(sum(counts))
    ids = np.split(np.arange(n), np.cumsum(counts)[:-1])
    sim = types.SimpleNamespace(num_objects=n, num_groups=len(counts), max_num_objects=M, goal_pos_offset=0.0, goal_rot_weight=1.0,
                                object_groups=[types.SimpleNamespace(object_ids=list(map(int, g))) for g in ids])
    g = GOAL.__new__(GOAL)
    g.mujoco_simulation, g.args, g.rot_dist_func = sim, types.SimpleNamespace(rot_dist_type="full"), FULL
    out = g.goal_distance({"obj_pos": goal_pos, "obj_rot": goal_rot}, {"obj_pos": cur_pos, "obj_rot": cur_rot})
    env = types.SimpleNamespace(constants=types.SimpleNamespace(success_threshold=dict(THR), goal_reward_per_object=1.0))
    dist = {"obj_pos": out["obj_pos"], "obj_rot": out["obj_rot"]}
    assert out["obj_pos"].shape == (M,) and out["relative_goal"]["obj_pos"].shape == (M, 3)
    return (out["relative_goal"]["obj_pos"], out["relative_goal"]["obj_rot"], out["obj_pos"], out["obj_rot"], float(ENV._calculate_num_success(env, dist)),
            bool(ROBOT._is_successful(env, dist)))


def main():
    rng = np.random.RandomState(41)
    rows = []
    for M in (3, 5, 8):
        for n in range(1, M + 1):
            for counts in ([1] * n,) + (([n],) if n >= 2 else ()):
                made = 0
                while made < 4:
                    goal_pos, goal_rot = np.zeros((M, 3)), np.zeros((M, 3))
                    goal_pos[:n] = rng.uniform(-0.3, 0.3, (n, 3)) + OFFSET
                    goal_rot[:n] = rng.uniform(-np.pi, np.pi, (n, 3))
                    if made % 2 == 0:      # pure yaw (objects flat on the table)
                        goal_rot[:, :2] = 0
                    # case 0 of a set: every active object inside both thresholds (the goal is achieved); the others: a random kind per object
                    kind = np.zeros(n, dtype=int) if made == 0 else rng.randint(0, 4, n)
                    cur_pos, cur_rot = goal_pos.copy(), goal_rot.copy()
                    step = rng.normal(size=(n, 3)); step /= np.linalg.norm(step, axis=-1, keepdims=True)
                    far_p = (kind & 1).astype(bool)
                    cur_pos[:n] += step * np.where(far_p, rng.uniform(0.06, 0.12, n), rng.uniform(0.0, 0.03, n))[:, None]
                    far_r = (kind & 2).astype(bool)
                    cur_rot[:n, 2] += np.where(far_r, rng.uniform(0.3, 1.2, n), rng.uniform(0.0, 0.15, n)) * rng.choice([-1.0, 1.0], n)
                    if len(counts) == 1 and n >= 2 and made % 2 == 1:      # duplicates: the objects sit at a shuffled assignment of the goals
                        perm = rng.permutation(n)
                        cur_pos[:n], cur_rot[:n] = cur_pos[perm], cur_rot[perm]
                    if min_margin(counts, cur_pos[:n], goal_pos[:n]) < MARGIN:
                        continue
                    rel_pos, rel_rot, d_pos, d_rot, nsucc, ok = reference_case(M, counts, cur_pos, cur_rot, goal_pos, goal_rot)
                    if min(np.abs(d_pos[:n] - THR["obj_pos"]).min(), np.abs(d_rot[:n] - THR["obj_rot"]).min()) < KEEP:
                        continue
                    assert not d_pos[n:].any() and not d_rot[n:].any() and not rel_pos[n:].any() and not rel_rot[n:].any()      # the padded slots read zero
                    rows.append(dict(M=M, n=n, single=int(len(counts) == 1 and n >= 2), cur_pos=cur_pos, cur_rot=cur_rot, goal_pos=goal_pos, goal_rot=goal_rot, rel_pos=rel_pos,
                                     rel_rot=rel_rot, dist_pos=d_pos, dist_rot=d_rot, num_success=nsucc, achieved=ok))
                    made += 1
    T = len(rows)
    A = dict(M=np.array([r["M"] for r in rows], dtype=np.int32), n=np.array([r["n"] for r in rows], dtype=np.int32), single=np.array([r["single"] for r in rows], dtype=np.int32),
             num_success=np.array([r["num_success"] for r in rows]), achieved=np.array([r["achieved"] for r in rows]),
             **{k: np.zeros((T, MMAX, 3)) for k in ("cur_pos", "cur_rot", "goal_pos", "goal_rot", "rel_pos", "rel_rot")}, dist_pos=np.zeros((T, MMAX)), dist_rot=np.zeros((T, MMAX)))
    for t, r in enumerate(rows):
        for k in ("cur_pos", "cur_rot", "goal_pos", "goal_rot", "rel_pos", "rel_rot", "dist_pos", "dist_rot"):
            A[k][t, :r["M"]] = r[k]
    # both sides of both thresholds among the active objects, achieved and not achieved, and the padded slots counted as within (the NOTE of _calculate_num_success)
    act = np.arange(MMAX)[None, :] < A["n"][:, None]
    for k, thr in (("dist_pos", THR["obj_pos"]), ("dist_rot", THR["obj_rot"])):
        assert (A[k][act] < thr).any() and (A[k][act] > thr).any()
    within = ((A["dist_pos"] < THR["obj_pos"]) & (A["dist_rot"] < THR["obj_rot"]) & act).sum(1)
    assert np.array_equal(A["num_success"], within + (A["M"] - A["n"])) and np.array_equal(A["achieved"], within == A["n"]) and A["achieved"].any() and not A["achieved"].all()
    out = os.path.join(HERE, "..", "tests", "golden", "rearrange_padded.npz")
    np.savez_compressed(out, pos_threshold=THR["obj_pos"], rot_threshold=THR["obj_rot"], **A)
    print("wrote %s: %d cases (%d achieved, %d with one group of duplicates)" % (out, T, int(A["achieved"].sum()), int(A["single"].sum())))


if __name__ == "__main__":
    main()
