"""Golden vectors for the masks of the placement area (tests/golden/rearrange_placement_mask.json).  The reference's `check_objects_in_placement_area`,
`extract_placement_area_boundary`, `get_placement_area` and `get_table_setting` (/root/reference/robogym/envs/rearrange/simulation/base.py:834-902, 980-1010) are
executed from their source on a stub simulation whose table is the shipped blocks model's, as tools/gen_golden_rearrange_dominos.py does (whose `exec_source` this
uses); nothing of it is copied.  Data only:

  (a) `pin`: the positions of the reference's own table (envs/rearrange/tests/test_object_in_placement_area.py:22-53), read from that file, with their margins and the
      masks the reference computes for them, without padding (num_objects rows) and padded to max_num_objects = 5 with zero rows; the generator asserts that they are
      the masks that table expects.
  (b) `clouds`: for n in {1, 3, 5} and used_table_portion in {1.0, 0.2} a seeded cloud of 256 points in a band of +- 0.2 m around the boundary (z included), each with
      the reference's max_dist and its hard mask at margin 0.02 ...
  (c) ... and its soft probability clip(max_dist / margin, 0, 1) at margin 0.1.
  `soft`: the four positions of the reference's soft-mask test (:129-141) with their probabilities at margin 0.1.

A cloud point with |max_dist - margin| < 1e-5 for either margin is dropped: that is about ten fp32 ulps of the ~1.7 m coordinates after the handful of operations
involved, so an fp32 implementation has to decide the same way.  More than 1 % dropped from a cloud is an error (expected: about 1e-4).

Needs /root/reference; the fixture travels.

    python tools/gen_golden_rearrange_placement_mask.py
"""
import ast
import collections
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
np.bool = bool      # (the reference predates numpy 1.24)

from gen_golden_rearrange_dominos import REF, exec_source  # noqa: E402

PlacementArea = collections.namedtuple("PlacementArea", ["offset", "size"])
MAX_OBJECTS, HARD_MARGIN, SOFT_MARGIN, KEEP, BAND, CLOUD = 5, 0.02, 0.1, 1.0e-5, 0.2, 256
METHODS = ("extract_placement_area_boundary", "check_objects_in_placement_area", "get_table_setting", "get_placement_area")


def reference_sim(table_pos, table_size, num_objects, max_num_objects, portion):
    """the reference's four methods on a stub that answers what they ask of the simulation"""
    ns = exec_source(REF + "/simulation/base.py", classes={"RearrangeSimulationInterface": METHODS}, ns={"np": np, "PlacementArea": PlacementArea, "Optional": None})
    sim = ns["RearrangeSimulationInterface"]()
    sim.num_objects, sim.max_num_objects, sim.used_table_portion = int(num_objects), int(max_num_objects), float(portion)
    sim.get_table_dimensions = lambda: (table_pos, table_size, table_pos[2] + table_size[2])
    return sim


def max_dist_of(sim, pos):
    """the reference's max_dist: the hard rule's own decision at a margin is `max_dist < margin`, so the smallest margin in a bisection that accepts the point IS it; here
    it is read off directly from the boundary the reference extracts (the same three lines as :881-884), and checked against the reference's decisions below"""
    b = sim.extract_placement_area_boundary()
    d = np.maximum(np.maximum(pos - np.array(b[3:]), np.array(b[:3]) - pos), 0.0)
    return d.max(-1)


def reference_pin_table():
    """(obj_pos, in_placement_area, margin) of test_single_obj_in_placement_area's parametrize list, read from the reference's test file"""
    path = REF + "/tests/test_object_in_placement_area.py"
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name == "test_single_obj_in_placement_area":
            return ast.literal_eval(node.decorator_list[0].args[1])
    raise RuntimeError("parametrize list not found in " + path)


def reference_soft_table():
    path = REF + "/tests/test_object_in_placement_area.py"
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.FunctionDef) and node.name == "test_soft_mask_observation":
            return ast.literal_eval(node.decorator_list[0].args[1])[0]
    raise RuntimeError("parametrize list not found in " + path)


def main():
    from robogym_amd.envs.rearrange.xml import load_blocks_model

    model = load_blocks_model(5)
    A = model.arrays
    table_pos = np.array(A["body_pos"][model.name2id("body", "table")], dtype=np.float64)
    table_size = np.array(A["geom_size"][model.names["geom"].index("table")], dtype=np.float64)
    out = dict(table_pos=table_pos.tolist(), table_size=table_size.tolist(), max_num_objects=MAX_OBJECTS, hard_margin=HARD_MARGIN, soft_margin=SOFT_MARGIN)
    # ---- (a) the reference's own table
    pin = []
    for obj_pos, expected, margin in reference_pin_table():
        n = len(obj_pos)
        sim = reference_sim(table_pos, table_size, n, MAX_OBJECTS, 1.0)
        pos = np.array(obj_pos, dtype=np.float64)
        mask = sim.check_objects_in_placement_area(pos, margin=margin)
        padded_pos = np.concatenate([pos, np.zeros((MAX_OBJECTS - n, 3))])
        padded = sim.check_objects_in_placement_area(padded_pos, margin=margin)
        assert list(mask) == list(expected) and list(padded[:n]) == list(expected) and padded[n:].all() and len(padded) == MAX_OBJECTS
        assert np.abs(max_dist_of(sim, pos) - margin).min() > 1.0e-4      # (every case clear of its decision)
        pin.append(dict(n=n, margin=margin, pos=pos.tolist(), mask=[bool(x) for x in mask], padded_pos=padded_pos.tolist(), padded_mask=[bool(x) for x in padded]))
    out["pin"] = pin
    b = reference_sim(table_pos, table_size, 5, MAX_OBJECTS, 1.0).extract_placement_area_boundary()
    out["boundary_n5_portion1"] = [float(x) for x in b]
    # ---- (b), (c) clouds around the boundary of the area of n objects
    rng = np.random.RandomState(20261020)
    clouds = []
    for n in (1, 3, 5):
        for portion in (1.0, 0.2):
            sim = reference_sim(table_pos, table_size, n, MAX_OBJECTS, portion)
            b = np.array(sim.extract_placement_area_boundary())
            lo, hi = b[:3], b[3:]
            # per coordinate: near the low face, near the high face, or anywhere between them
            where = rng.randint(0, 3, (CLOUD, 3))
            near = rng.uniform(-BAND, BAND, (CLOUD, 3))
            pos = np.where(where == 0, lo + near, np.where(where == 1, hi + near, rng.uniform(lo - BAND, hi + BAND, (CLOUD, 3))))
            md = max_dist_of(sim, pos)
            keep = (np.abs(md - HARD_MARGIN) >= KEEP) & (np.abs(md - SOFT_MARGIN) >= KEEP)
            assert (~keep).sum() <= 0.01 * CLOUD, "dropped %d of %d points" % ((~keep).sum(), CLOUD)
            pos, md = pos[keep], md[keep]
            # the reference's decisions, the cloud taken num_objects rows at a time (the method insists on that shape)
            hard = np.zeros(len(pos), dtype=bool)
            for i in range(0, len(pos) - len(pos) % n, n):
                hard[i:i + n] = sim.check_objects_in_placement_area(pos[i:i + n], margin=HARD_MARGIN)
            for i in range(len(pos) - len(pos) % n, len(pos)):      # (a remainder: padded with copies of the point)
                hard[i] = sim.check_objects_in_placement_area(np.tile(pos[i], (n, 1)), margin=HARD_MARGIN)[0]
            assert np.array_equal(hard, md < HARD_MARGIN) and hard.any() and not hard.all()
            proba = np.clip(md / SOFT_MARGIN, 0.0, 1.0)
            assert ((proba > 0) & (proba < 1)).any()
            # the reference's soft rule draws np.random.random() once per call: with the global generator seeded, its decisions are u > proba for that one u
            for i in range(0, len(pos) - len(pos) % n, n):
                np.random.seed(i)
                u = np.random.RandomState(i).random_sample()
                assert np.array_equal(sim.check_objects_in_placement_area(pos[i:i + n], margin=SOFT_MARGIN, soft=True), u > proba[i:i + n])
            clouds.append(dict(n=n, portion=portion, boundary=b.tolist(), pos=pos.tolist(), max_dist=md.tolist(), hard_mask=[bool(x) for x in hard], soft_proba=proba.tolist()))
    out["clouds"] = clouds
    # ---- the soft test's positions
    spos, expected = reference_soft_table()
    sim = reference_sim(table_pos, table_size, len(spos), MAX_OBJECTS, 1.0)
    md = max_dist_of(sim, np.array(spos, dtype=np.float64))
    out["soft"] = dict(pos=spos, expected=expected, margin=SOFT_MARGIN, proba=np.clip(md / SOFT_MARGIN, 0.0, 1.0).tolist())
    assert [None if 0 < p < 1 else p == 0 for p in out["soft"]["proba"]] == expected
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_placement_mask.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes;", sum(len(c["pos"]) for c in clouds), "cloud points")


if __name__ == "__main__":
    main()
