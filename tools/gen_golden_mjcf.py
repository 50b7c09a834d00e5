"""tests/golden/mjcf_locked.xml, mjcf_solver.xml, mjcf_meshes.npz: the merged MJCF documents of dactyl/locked and of the rearrange TCP solver world, as
`build_locked_xml()` / `build_solver_xml()` assemble them from the robogym asset tree, with `meshdir` replaced by the placeholder MESHDIR, and the convex hull
of every mesh file they name (vertices exactly as in the STL, outward-oriented faces).  tests/test_compile_mjcf.py writes the hulls as binary STL files and
feeds the documents through the C ABI, so it runs without the asset tree.  The hulls keep the vertices the compiler stores for collision; the inertial frames
of the mesh geoms are those of the hulls.  Needs the asset tree (ROBOGYM_ASSETS_DIR); the fixtures travel with the repository.

    ROBOGYM_ASSETS_DIR=/path/to/robogym/assets python tools/gen_golden_mjcf.py
"""
import os
import re
import sys

import numpy as np
from scipy.spatial import ConvexHull

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

from robogym_amd.envs.dactyl.locked import build_locked_xml  # noqa: E402
from robogym_amd.envs.rearrange.xml import build_solver_xml  # noqa: E402
from robogym_amd.mujoco.mjcf_compiler import load_stl  # noqa: E402
from robogym_amd.mujoco.mujoco_xml import assets_dir  # noqa: E402


def main():
    meshdir = os.path.join(assets_dir(), "stls")
    files = set()
    for name, build in (("locked", build_locked_xml), ("solver", build_solver_xml)):
        doc = build().xml_string()
        files |= {f for f in re.findall(r'file="([^"]+)"', doc) if f.lower().endswith(".stl")}
        doc = doc.replace('meshdir="%s"' % meshdir, 'meshdir="MESHDIR"')
        assert assets_dir() not in doc
        with open(os.path.join(OUT, "mjcf_%s.xml" % name), "w") as f:
            f.write(doc)
    arrays = {"names": np.array(sorted(files))}
    for i, fn in enumerate(sorted(files)):
        pts = np.unique(load_stl(os.path.join(meshdir, fn)).reshape(-1, 3), axis=0)
        hull = ConvexHull(pts)
        faces = hull.simplices.copy()
        a, b, c = (pts[faces[:, k]] for k in range(3))
        flip = np.einsum("ij,ij->i", np.cross(b - a, c - a), hull.equations[:, :3]) < 0
        faces[flip] = faces[flip][:, ::-1]
        used = np.unique(faces)
        arrays["v%d" % i] = pts[used].astype(np.float32)
        arrays["f%d" % i] = np.searchsorted(used, faces).astype(np.int32)
    np.savez_compressed(os.path.join(OUT, "mjcf_meshes.npz"), **arrays)
    print("%d meshes -> %s" % (len(files), os.path.join(OUT, "mjcf_meshes.npz")))


if __name__ == "__main__":
    main()
