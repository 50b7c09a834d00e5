"""Golden vectors for rearrange/blocks_attached and the fixed goal placement (tests/golden/rearrange_attached.npz, rearrange_attached_worlds.json).  The reference's
source is executed as it stands on a stub simulation, as tools/gen_golden_rearrange_dominos.py does (whose `exec_source` this uses); nothing of it is copied.

  (a) `AttachedBlockStateGoal._sample_next_goal_positions` (/root/reference/robogym/envs/rearrange/goals/attached_block_state.py) for several seeds: the seed, the log of
      its draws (the permutation as the row order it produced, then the two uniforms) and the goal positions.
  (f) `place_targets_with_fixed_position` (common/utils.py:884-919, through _place_objects / _place_objects_trial) on a handful of placement tables, N in {1, 3, 8},
      boxes with non-zero bounding-box centres and unequal half sizes included.
  worlds: the MJCF build of the blocks world with 6, 7 and 8 blocks per array, as tools/gen_golden_blocks_worlds.py records the smaller ones.

Needs /root/reference; the fixtures travel.

    python tools/gen_golden_rearrange_attached.py
"""
import collections
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))

from gen_golden_rearrange_dominos import REF, exec_source  # noqa: E402

PlacementArea = collections.namedtuple("PlacementArea", ["offset", "size"])
TABLE_POS, TABLE_SIZE = np.array([1.32, 0.75, 0.4]), np.array([0.4575, 0.6, 0.05324])      # (a stub table, near the blocks world's)


class LoggedRandom:
    """np.random.RandomState whose draws are recorded: a permutation as the order of rows it produced, uniforms as their values"""

    def __init__(self, seed):
        self.rs, self.perm, self.log = np.random.RandomState(seed), None, []

    def permutation(self, x):
        twin = np.random.RandomState()
        twin.set_state(self.rs.get_state())
        order = twin.permutation(len(x))
        v = self.rs.permutation(x)
        assert np.array_equal(v, np.asarray(x)[order])      # (rows of an array are shuffled by the draws that shuffle their indices)
        self.perm = order
        return v

    def uniform(self, low=0.0, high=1.0, size=None):
        v = self.rs.uniform(low=low, high=high, size=size); self.log.extend(np.atleast_1d(v).tolist()); return v


class Sim:
    """what the two goal generators ask of the simulation"""

    def __init__(self, centre, half, portion=1.0, object_size=0.0254):
        self.boxes = np.stack([centre, half], 1)
        self.num_objects, self.used_table_portion = len(centre), portion
        self.simulation_params = types.SimpleNamespace(object_size=object_size)
        self.target_quat = None

    def set_target_quat(self, q):
        self.target_quat = np.array(q)

    def forward(self):
        pass

    def get_object_bounding_boxes(self):
        return self.boxes.copy()

    def get_table_dimensions(self):
        return TABLE_POS, TABLE_SIZE, TABLE_POS[2] + TABLE_SIZE[2]

    def get_placement_area(self):      # simulation/base.py:980-1010
        tsx, tsy = TABLE_SIZE[:2] * 2
        p = np.clip(self.used_table_portion, self.num_objects * 0.1, 1.0)
        w, h = 0.5 * tsx * p, 0.38 * tsy * p
        return PlacementArea(offset=(0.5 * tsx - w / 2.0, 0.44 * tsy - h / 2.0, 2 * TABLE_SIZE[2]), size=(w, h, 0.26))


def main():
    utils = exec_source(REF + "/common/utils.py", functions=("_place_objects", "_place_objects_trial", "place_targets_with_fixed_position"),
                        ns={"np": np, "PlacementArea": PlacementArea})
    ns = exec_source(REF + "/goals/attached_block_state.py", classes={"AttachedBlockStateGoal": ("_sample_next_goal_positions",)},
                     ns={"np": np, "place_targets_with_fixed_position": utils["place_targets_with_fixed_position"]})
    out = dict(table_pos=TABLE_POS, table_size=TABLE_SIZE)
    # ---- (a) the attached goal
    sim = Sim(np.zeros((8, 3)), np.full((8, 3), 0.0254))
    goal = ns["AttachedBlockStateGoal"].__new__(ns["AttachedBlockStateGoal"])
    goal.mujoco_simulation = sim
    seeds = np.arange(100, 112)
    perms, draws, poss = [], [], []
    for seed in seeds:
        rs = LoggedRandom(int(seed))
        pos, ok = goal._sample_next_goal_positions(rs)
        assert ok and np.array_equal(sim.target_quat, np.tile([1, 0, 0, 0], (8, 1))) and len(rs.log) == 2
        perms.append(rs.perm); draws.append(rs.log); poss.append(pos)
    area = sim.get_placement_area()
    out.update(a_seeds=seeds, a_perm=np.array(perms), a_draws=np.array(draws), a_pos=np.array(poss), a_object_size=np.array(0.0254),
               a_area=np.array([area.offset[:2], area.size[:2]]))
    assert len({tuple(p) for p in perms}) == len(seeds)
    # ---- (f) fixed placements
    rng = np.random.RandomState(41)
    cases = [(1, 1.0), (3, 1.0), (3, 0.5), (8, 1.0), (8, 0.9)]
    out["f_cases"] = np.array(cases)
    for ci, (N, portion) in enumerate(cases):
        centre, half = rng.uniform(-0.02, 0.02, (N, 3)), rng.uniform(0.01, 0.05, (N, 3))
        if ci == 0:
            centre[:] = 0.0
        rel = rng.uniform(0.0, 1.0, (N, 2))
        if ci == 1:
            rel[0], rel[1] = (0.0, 0.0), (1.0, 1.0)      # (the area's corners)
        s_ = Sim(centre, half, portion)
        a_ = s_.get_placement_area()
        pos, ok = utils["place_targets_with_fixed_position"](s_.get_object_bounding_boxes(), s_.get_table_dimensions(), a_, rel)
        assert ok
        out.update({"f%d_centre" % ci: centre, "f%d_half" % ci: half, "f%d_rel" % ci: rel, "f%d_pos" % ci: pos, "f%d_area" % ci: np.array([a_.offset[:2], a_.size[:2]])})
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_attached.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    # ---- the MJCF build of the 6-, 7- and 8-block worlds
    from gen_golden_blocks_worlds import describe
    from robogym_amd.envs.rearrange.xml import build_blocks_xml

    worlds = {str(n): describe(build_blocks_xml(n).build()) for n in (6, 7, 8)}
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_attached_worlds.json")
    with open(path, "w") as f:
        json.dump(worlds, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
