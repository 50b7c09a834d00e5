"""tests/golden/rearrange_blocks_worlds.json: the blocks worlds with 1 and 2 blocks as compile_mjcf builds them from the reference's MJCF + assets -- per array its
shape, dtype and sha256 (the arrays copied from the larger world), the values of the arrays set_constants computes (compared with a tolerance: they go through a
matrix inverse), the name tables.  envs/rearrange/xml.py `blocks_world_subset` cuts these worlds out of the shipped 5-block one; tests/test_rearrange_tasks.py
checks the cut against this file.  Needs /root/reference; the fixture travels.

    python tools/gen_golden_blocks_worlds.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))

from robogym_amd.envs.rearrange.xml import build_blocks_xml  # noqa: E402

#: the arrays robogym_amd/mujoco/setconst.py `set_constants` writes
COMPUTED = ("body_subtreemass", "stat_meaninertia", "body_invweight0", "dof_invweight0", "tendon_length0", "tendon_invweight0", "tendon_lengthspring", "actuator_acc0")


def fingerprint(a):
    a = np.ascontiguousarray(a)
    return {"shape": list(a.shape), "dtype": a.dtype.str, "sha256": hashlib.sha256(a.tobytes()).hexdigest()}


def describe(model):
    A = model.arrays
    return {"arrays": {k: fingerprint(v) for k, v in sorted(A.items()) if k not in COMPUTED},
            "computed": {k: np.asarray(A[k], dtype=np.float64).ravel().tolist() for k in COMPUTED},
            "names": {k: list(v) for k, v in sorted(model.names.items())}}


def main():
    out = {str(n): describe(build_blocks_xml(n).build()) for n in (1, 2)}
    path = os.path.join(HERE, "..", "tests", "golden", "rearrange_blocks_worlds.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
