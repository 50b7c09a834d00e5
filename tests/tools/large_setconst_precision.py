"""The row sets of tests/test_large_setconst.py and the float32 round-off of mj_setConst on them.

`rb_setconst_kernel` computes dof / body / tendon `_invweight0` in float32; it cannot be expected to beat the round-off of the same
algorithm evaluated in float32 on the host.  This tool evaluates robogym_amd/mujoco/setconst.py's definition twice per model and row set
-- in double (`setconst.set_constants`, the ground truth of the tests) and in float32 (`set_constants_f32`: the same numpy code with the
model arrays, the Jacobians, M and its inverse in float32) -- and writes the worst relative error of the float32 evaluation, E32, per
output to tests/golden/large_setconst_spread.json.  The tests hold the kernel to max(2e-5, 4 x E32) (the factor 4: a different
elimination order).  Nothing here looks at the kernel's output.

    python -m tests.tools.large_setconst_precision          # rewrites the json (ten evaluations of the full cube, seconds each)
"""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden", "large_setconst_spread.json")
ROW_FIELDS = ("body_pos", "body_mass", "body_inertia", "dof_armature", "site_pos")     # the rows the kernel reads and the row sets below change
OUTPUTS = ("dof_invweight0", "body_invweight0", "tendon_invweight0")
CUBE_SCALE = 1.05


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def default_rows(model):
    A = model.arrays
    return {"body_pos": _f32(A["body_pos"]).reshape(-1, 3), "body_mass": _f32(A["body_mass"]).reshape(-1), "body_inertia": _f32(A["body_inertia"]).reshape(-1, 3),
            "dof_armature": _f32(A["dof_armature"]).reshape(-1), "site_pos": _f32(A["site_pos"]).reshape(-1, 3)}


def full_cube_site_shift(model):
    """tests/test_large_env_params.py::_site_shift: U(-3 mm, 3 mm) on the fingertip and reference sites (same generator, same ids)"""
    from robogym_amd.envs.dactyl.full_perpendicular import FINGERTIP_SITE_NAMES, REFERENCE_SITE_NAMES

    names = model.names["site"]
    ids = [names.index("robot0:" + n) for n in list(FINGERTIP_SITE_NAMES) + list(REFERENCE_SITE_NAMES)]      # FullPerpendicularSimulation.tip_sites + ref_sites
    shift = np.zeros((len(names), 3))
    shift[ids] = np.random.RandomState(11).uniform(-0.003, 0.003, (len(ids), 3))
    return shift.astype(np.float32)


def full_cube_row_sets(model, site_shift=None):
    """name -> rows (float32, as they sit in the env's parameter block): the four masked-in envs of the full-cube test, the combined env of the physics test and the env flag test's"""
    A, N = model.arrays, model.names
    nb = len(N["body"])
    cubelets = [b for b, n in enumerate(N["body"]) if n.startswith("cube:cubelet:")]
    cube_bodies = [b for b, n in enumerate(N["body"]) if n.startswith("cube:")]
    hand_dofs = [int(A["jnt_dofadr"][j]) for j, n in enumerate(N["joint"]) if n.startswith("robot0:")]
    shift = full_cube_site_shift(model) if site_shift is None else _f32(site_shift)
    sets = {"default": default_rows(model)}
    r = default_rows(model)
    r["body_inertia"] = r["body_inertia"] * np.random.RandomState(21).uniform(0.5, 1.5, (nb, 1)).astype(np.float32)      # RandomizedBodyInertiaWrapper: one factor per body
    sets["inertia"] = r
    r = default_rows(model)
    r["body_pos"][cubelets] = r["body_pos"][cubelets] * np.float32(CUBE_SCALE)       # set_cube_size_multiplier(1.05)
    r["site_pos"] = r["site_pos"] + shift
    sets["scale+sites"] = r
    r = default_rows(model)
    r["body_mass"][cube_bodies] = r["body_mass"][cube_bodies] * np.random.RandomState(22).uniform(0.7, 1.3, len(cube_bodies)).astype(np.float32)
    r["dof_armature"][hand_dofs] = r["dof_armature"][hand_dofs] * np.float32(2.0)
    sets["mass+armature"] = r
    r = {k: v.copy() for k, v in sets["scale+sites"].items()}
    r["body_inertia"] = sets["inertia"]["body_inertia"].copy()
    sets["inertia+scale+sites"] = r
    r = default_rows(model)
    r["body_pos"][cubelets] = r["body_pos"][cubelets] * np.float32(CUBE_SCALE)       # the env flag test: cube_size_multiplier alone
    sets["scale"] = r
    return sets


def rearrange_row_sets(model):
    """default and: body_mass x 1.5 on the object bodies (none in the solver world), dof_armature x 1.5, body_pos + 5 mm on two robot bodies"""
    A, N = model.arrays, model.names
    objects = [b for b, n in enumerate(N["body"]) if n.startswith("object")]
    two = [N["body"].index("Elbow"), N["body"].index("left_gripper")]        # an arm link and a gripper finger
    r = default_rows(model)
    r["body_mass"][objects] = r["body_mass"][objects] * np.float32(1.5)
    r["dof_armature"] = r["dof_armature"] * np.float32(1.5)
    r["body_pos"][two] = r["body_pos"][two] + np.float32(0.005)
    return {"default": default_rows(model), "changed": r}


def model_with_rows(model, rows):
    return model.copy_with(**{k: np.asarray(v, dtype=np.float64) for k, v in rows.items()})


def truth(model, rows):
    """`setconst.set_constants` in double on the model with the (float32-rounded) rows: the three outputs"""
    from robogym_amd.mujoco import setconst

    m = setconst.set_constants(model_with_rows(model, rows))
    return {k: np.asarray(m.arrays[k], dtype=np.float64).copy() for k in OUTPUTS}


def set_constants_f32(model, rows):
    """The definition of setconst.set_constants:234-263 with the model arrays, the Jacobians, M and its inverse in float32."""
    from robogym_amd.mujoco import mjcf_compiler as C
    from robogym_amd.mujoco import setconst as SC

    m = model_with_rows(model, rows)
    A = m.arrays
    for k, v in list(A.items()):
        if isinstance(v, np.ndarray) and v.dtype == np.float64:
            A[k] = v.astype(np.float32).astype(np.float64)          # every model array rounded to float32
    f = np.float32
    nbody, nv = len(A["body_parentid"]), len(A["dof_bodyid"])
    kin = SC.kinematics(m, A["qpos0"])
    kin = {k: v.astype(f) for k, v in kin.items()}
    M = np.diag(A["dof_armature"].astype(f))
    jacs = {}
    for b in range(1, nbody):
        jp, jr = SC.jac(m, kin, kin["xipos"][b], b)
        jacs[b] = (jp.astype(f), jr.astype(f))
        if A["body_mass"][b] <= 0 and not A["body_inertia"][b].any():
            continue
        jp, jr = jacs[b]
        Iw = kin["ximat"][b] @ np.diag(A["body_inertia"][b].astype(f)) @ kin["ximat"][b].T
        M = M + f(A["body_mass"][b]) * (jp.T @ jp) + jr.T @ Iw @ jr
    assert M.dtype == f
    Minv = np.linalg.inv(M) if nv else np.zeros((0, 0), dtype=f)
    assert Minv.dtype == f
    biw = np.zeros((nbody, 2), dtype=f)
    for b in range(1, nbody):
        if A["body_weldid"][b] == 0:
            continue
        jp, jr = jacs[b]
        biw[b, 0] = max(f(SC.MINVAL), np.trace(jp @ Minv @ jp.T) / f(3))
        biw[b, 1] = max(f(SC.MINVAL), np.trace(jr @ Minv @ jr.T) / f(3))
    diw = np.diag(Minv).copy()
    for j in range(len(A["jnt_type"])):
        da, t = A["jnt_dofadr"][j], A["jnt_type"][j]
        if t == C.JNT_BALL:
            diw[da:da + 3] = diw[da:da + 3].mean()
        elif t == C.JNT_FREE:
            diw[da:da + 3] = diw[da:da + 3].mean(); diw[da + 3:da + 6] = diw[da + 3:da + 6].mean()
    L, Jt = SC.tendon(m, kin, A["qpos0"])
    Jt = Jt.astype(f)
    tiw = np.array([max(f(SC.MINVAL), Jt[t] @ Minv @ Jt[t]) for t in range(len(L))], dtype=f)
    return {"dof_invweight0": diw.astype(np.float64), "body_invweight0": biw.astype(np.float64), "tendon_invweight0": tiw.astype(np.float64)}


def rel_err(got, want):
    """worst relative error over the non-zero entries of `want` (entries that are exactly 0 -- welded bodies -- must be 0 in `got`)"""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    if want.size == 0:
        return 0.0
    nz = want != 0
    assert not np.any(got[~nz] != 0)
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz]))) if nz.any() else 0.0


def models():
    from robogym_amd.envs.dactyl.full_perpendicular import load_full_perpendicular_model
    from robogym_amd.envs.rearrange.xml import load_blocks_model, load_solver_model
    from robogym_amd.mujoco import setconst
    from robogym_amd.mujoco.big_tables import derive_big_tables

    full = load_full_perpendicular_model()
    setconst.set_constants(full)
    derive_big_tables(full)
    return {"full_cube": (full, full_cube_row_sets(full)), "blocks5": (load_blocks_model(5), None), "solver_world": (load_solver_model(), None)}


def main():
    out = {"_comment": "E32: worst relative error of the float32 host evaluation of mj_setConst against the double one, per model, row set and output "
                       "(tests/tools/large_setconst_precision.py); the tests' bound is max(2e-5, 4 * E32)", "E32": {}}
    for name, (model, sets) in models().items():
        sets = sets if sets is not None else rearrange_row_sets(model)
        out["E32"][name] = {}
        for key, rows in sets.items():
            t, s = truth(model, rows), set_constants_f32(model, rows)
            out["E32"][name][key] = {k: rel_err(s[k], t[k]) for k in OUTPUTS}
            print(name, key, out["E32"][name][key])
    with open(GOLDEN, "w") as fjson:
        json.dump(out, fjson, indent=1, sort_keys=True)
        fjson.write("\n")


if __name__ == "__main__":
    main()
