"""Golden vectors for rot_dist_type "icp" (tests/golden/rearrange_icp.npz, rearrange_icp_spread.json): the REAL `ICP` of /root/reference/robogym/utils/icp.py, imported
as it stands (sklearn's NearestNeighbors; a stub stands in for `trimesh`, which robogym/utils/mesh.py imports and the functions used here never call), run on OUR point
clouds (robogym_amd/envs/rearrange/icp.py) of four objects of the shipped ycb set 4 and of one block.  Needs /root/reference and sklearn; the fixtures travel.

    python tools/gen_golden_rearrange_icp.py

Clouds (float32 in the file, as the device holds them): the source as `object_point_clouds` makes it, the target thinned to at most 1024 points by a fixed stride.
Cases per cloud: generic ones -- a random goal orientation, the object turned away from it by 0.05 .. 0.3 rad about a random axis -- and, for the four objects, the
z-rotation table of the reference's tests/test_object_rotation.py:213-362 (goal = z(angle) x init for 0, pi/4, pi/2, 3 pi/4, pi).  Stored per case: the reference's
result matrix (or the refused flag) and its last max_error over the threshold.
A case is KEPT when the reference and our float64 restatement (`icp_rotation`) agree to 1e-9 on the matrix and exactly on the flag, the threshold margin
|max_error / threshold - 1| is at least 0.1, and the float32 and float64 runs of the restatement agree on the flag.  The tool fails unless at least 90 % of the generic
candidates and every z-table row are kept.  The spread -- the largest Euler-angle difference between the float32 and the float64 run of the restatement over the kept,
accepted cases -- goes into the json with the counts and the smallest margin; tests/test_rearrange_icp.py takes its kernel tolerance from it.
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
np.float = float      # (the reference's rotation module predates numpy 1.24)
sys.modules.setdefault("trimesh", types.ModuleType("trimesh"))
sys.path.insert(0, "/root/reference")
from robogym.utils import icp as REF  # noqa: E402

from robogym_amd.envs.rearrange import icp as OURS  # noqa: E402
from robogym_amd.envs.rearrange.xml import load_blocks_model, load_ycb_model  # noqa: E402

OBJECTS = ("057_racquetball", "003_cracker_box", "073-b_lego_duplo", "011_banana")
Z_ANGLES = (0.0, np.pi / 4, np.pi / 2, 3 * np.pi / 4, np.pi)
#: which z rotations count as "at the goal" (rotation distance < 0.2) per object: the reference's table for a ball, a box with 180 degree symmetry, one with 90 degree
#: symmetry and an asymmetric object
Z_AT_GOAL = {"057_racquetball": (1, 1, 1, 1, 1), "003_cracker_box": (1, 0, 0, 0, 1), "073-b_lego_duplo": (1, 0, 1, 0, 1), "011_banana": (1, 0, 0, 0, 0)}
ERROR_THRESHOLD, MAX_TARGET, N_GENERIC = 0.15, 1024, 10


def qmul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3], p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] + p[2] * q[0] + p[3] * q[1] - p[1] * q[3], p[0] * q[3] + p[3] * q[0] + p[1] * q[2] - p[2] * q[1]])


def axis_angle(axis, angle):
    axis = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def reference_case(src_w, tgt_w):
    """ICP.compute's result (matrix or None) and the last max_error over the threshold, from the reference's own functions"""
    obj = REF.ICP(tgt_w, error_threshold=ERROR_THRESHOLD)
    mat = obj.compute(src_w)
    _, max_error = REF.icp(src_w, tgt_w, obj.knn, max_iterations=5, tolerance=1e-6)
    return mat, float(max_error) / float(obj.error_threshold)


def wrap(a):
    return (a + np.pi) % (2 * np.pi) - np.pi


def main():
    rng = np.random.RandomState(23)
    ycb = load_ycb_model(8, set_index=4)
    names = list(ycb.names["object_mesh"])
    clouds = []
    for name in OBJECTS:
        src, tgt, _ = OURS.object_clouds_of_body(ycb, ycb.name2id("body", "object%d" % names.index(name)), ERROR_THRESHOLD, 500)
        stride = -(-len(tgt) // MAX_TARGET)
        clouds.append((name, src.astype(np.float32), tgt[::stride].astype(np.float32)))
    blocks = load_blocks_model(2)
    src, tgt, _ = OURS.object_clouds_of_body(blocks, blocks.name2id("body", "object0"), ERROR_THRESHOLD, 500)
    clouds.append(("block", src.astype(np.float32), tgt.astype(np.float32)))

    cases = []      # (cloud, obj_quat, goal_quat, is_ztable, z_index)
    for c, (name, _, _) in enumerate(clouds):
        for _ in range(N_GENERIC):
            goal = rng.randn(4); goal /= np.linalg.norm(goal)
            cases.append((c, qmul(axis_angle(rng.randn(3), rng.uniform(0.05, 0.3)), goal), goal, False, -1))
        if name in Z_AT_GOAL:
            init = axis_angle([0, 0, 1], 0.3)      # (an initial yaw: the table holds for z x init)
            for k, ang in enumerate(Z_ANGLES):
                cases.append((c, init, qmul(axis_angle([0, 0, 1], ang), init), True, k))

    keep, rows, spread, margin_min, dropped = [], [], 0.0, np.inf, []
    for c, oq, gq, is_z, k in cases:
        name, src, tgt = clouds[c]
        src_w = src.astype(np.float64) @ OURS._quat2mat(oq).T
        tgt_w = tgt.astype(np.float64) @ OURS._quat2mat(gq).T
        ref_mat, ref_ratio = reference_case(src_w, tgt_w)
        m64, r64 = OURS.icp_rotation(src_w, tgt_w, ERROR_THRESHOLD, return_error=True)
        m32, _ = OURS.icp_rotation(src_w, tgt_w, ERROR_THRESHOLD, dtype=np.float32, return_error=True)
        same = (ref_mat is None) == (m64 is None) and (ref_mat is None or np.abs(ref_mat - m64).max() <= 1e-9)
        margin = abs(ref_ratio - 1.0)
        ok = bool(same and margin >= 0.1 and (m32 is None) == (m64 is None))
        if is_z:
            at_goal = ref_mat is not None and 2 * np.arccos(min(1.0, abs(0.5 * np.sqrt(max(0.0, 1 + np.trace(ref_mat)))))) < 0.2
            assert at_goal == bool(Z_AT_GOAL[name][k]), "z table: %s at %.3f is %s in the reference" % (name, Z_ANGLES[k], "at the goal" if at_goal else "away")
        if not ok:
            dropped.append((name, is_z, k, same, margin))
            continue
        if m64 is not None:
            spread = max(spread, float(np.abs(wrap(OURS.mat2euler(m32.astype(np.float64)) - OURS.mat2euler(m64))).max()))
        margin_min = min(margin_min, margin)
        keep.append((c, oq, gq, is_z, k))
        rows.append((np.zeros((3, 3)) if ref_mat is None else ref_mat, ref_mat is None, ref_ratio))
    n_generic, kept_generic = sum(not x[3] for x in cases), sum(not x[3] for x in keep)
    n_z, kept_z = sum(x[3] for x in cases), sum(x[3] for x in keep)
    print("generic kept %d / %d, z table kept %d / %d, spread %.3g, smallest margin %.3g, dropped %s" % (kept_generic, n_generic, kept_z, n_z, spread, margin_min, dropped))
    assert kept_generic >= 0.9 * n_generic and kept_z == n_z, "the keeping rule drops too much: swap the object, do not loosen the rule"

    out = {"names": np.array([c[0] for c in clouds]), "z_angles": np.array(Z_ANGLES), "error_threshold": np.float64(ERROR_THRESHOLD),
           "case_cloud": np.array([x[0] for x in keep], dtype=np.int32), "case_obj_quat": np.array([x[1] for x in keep]), "case_goal_quat": np.array([x[2] for x in keep]),
           "case_z_index": np.array([x[4] for x in keep], dtype=np.int32), "ref_mat": np.array([r[0] for r in rows]), "ref_refused": np.array([r[1] for r in rows]),
           "ref_error_ratio": np.array([r[2] for r in rows]), "z_at_goal": np.array([Z_AT_GOAL[n] for n in OBJECTS], dtype=np.int32)}
    for c, (_, src, tgt) in enumerate(clouds):
        out["src_%d" % c], out["tgt_%d" % c] = src, tgt
    gold = os.path.join(HERE, "..", "tests", "golden")
    np.savez_compressed(os.path.join(gold, "rearrange_icp.npz"), **out)
    with open(os.path.join(gold, "rearrange_icp_spread.json"), "w") as f:
        json.dump({"spread": spread, "what": "largest Euler-angle difference [rad] between the float32 and the float64 run of icp_rotation over the kept, accepted cases",
                   "generic_candidates": n_generic, "generic_kept": kept_generic, "z_table_rows": n_z, "z_table_kept": kept_z, "smallest_margin": margin_min,
                   "error_threshold": ERROR_THRESHOLD}, f, indent=1)
        f.write("\n")
    print("wrote", gold)


if __name__ == "__main__":
    main()
