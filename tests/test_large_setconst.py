"""Device-side mj_setConst on the large-model stepper: `rb_setconst_kernel` / `rb_batch_set_constants` / `LargeModelSimulation.set_constants(mask)` and
`BatchedFullPerpendicularEnv(set_constants_on_reset=True)`.

Ground truth everywhere: `setconst.set_constants` in double on `model.copy_with(<the env's rows, rounded to fp32>)`, computed once per distinct row set in the
module-scoped fixture `truths` (the row sets themselves: tests/tools/large_setconst_precision.py, which also produced tests/golden/large_setconst_spread.json).
Tolerance per output: max(2e-5, 4 x E32) relative, plus atol 1e-12 on body_invweight0 -- 2e-5 is the bound of the same three outputs on the hand stepper
(tests/test_env_params.py:93-95), E32 the worst relative error of a float32 HOST evaluation of the same definition against the double one (the golden file), the
factor 4 covers a different elimination order.  Nothing is derived from the kernel's own output."""
import json
import os

import numpy as np
import pytest
import torch

from robogym_amd import _native
from tests.test_large_env_params import _scaled_cube_model, _site_shift, _sync_row, blocks_models, full_model  # noqa: F401  (fixtures)
from tests.test_large_model import OracleFullCube
from tests.tools import large_setconst_precision as SP

OUT = SP.OUTPUTS
SENTINEL = 123.25
FULL_ENVS = ("default", "inertia", "scale+sites", "mass+armature")       # envs 0-3 of the full-cube test; env 4 is masked out


@pytest.fixture(scope="module")
def spread():
    with open(os.path.join(os.path.dirname(__file__), "golden", "large_setconst_spread.json")) as f:
        return json.load(f)["E32"]


@pytest.fixture(scope="module")
def truths(full_model, blocks_models):
    """(model name, row set) -> (rows, double values of the three outputs): one setconst.set_constants per distinct row set"""
    out = {}
    for key, rows in SP.full_cube_row_sets(full_model).items():
        out["full_cube", key] = (rows, SP.truth(full_model, rows))
    for name, model in (("blocks5", blocks_models[0]), ("solver_world", blocks_models[1])):
        for key, rows in SP.rearrange_row_sets(model).items():
            out[name, key] = (rows, SP.truth(model, rows))
    return out


def _tol(spread, name, key, k, factor=1.0):
    return factor * max(2e-5, 4.0 * spread[name][key][k])


def _write_rows(sim, e, rows):
    P = sim.params
    for k, v in rows.items():
        P[k][e] = torch.as_tensor(v, device=sim.device)


def _rows_of(sim, e):
    return {k: sim.params[k][e].cpu().numpy().copy() for k in SP.ROW_FIELDS}


def _outputs_of(sim, e):
    return {k: sim.params[k][e].cpu().numpy().astype(np.float64).reshape(-1) for k in OUT}


def _check(got, want, spread, name, key, label, factor=1.0):
    """every entry within the tolerance of the double value; bodies welded to the world (mocap bodies included) exactly 0"""
    for k in OUT:
        w, g = np.asarray(want[k], dtype=np.float64).reshape(-1), got[k]
        assert g.shape == w.shape, (label, k)
        if w.size == 0:
            continue
        tol = _tol(spread, name, key, k, factor)
        atol = 1e-12 if k == "body_invweight0" else 0.0
        err = np.abs(g - w)
        rel = float((err / np.maximum(np.abs(w), 1e-300))[w != 0].max())
        print("%s %s: worst relative error %.3e (bound %.3e)" % (label, k, rel, tol))
        assert np.all(np.isfinite(g)), (label, k)
        assert np.all(err <= tol * np.abs(w) + atol), (label, k, rel, tol)
        assert np.all(g[w == 0] == 0.0), (label, k)


def _sentinel(sim):
    for k in OUT:
        if sim.params[k].numel():
            sim.params[k][:] = SENTINEL


# ------------------------------------------------------------------------------------------------ the full cube (large configuration)
def _full_cube_batch(full_model, lib, device):
    """B = 5: envs 0-3 carry FULL_ENVS' rows, env 4 (masked out) the inertia rows; all five start with the three output rows overwritten by a sentinel"""
    from robogym_amd.envs.dactyl.full_perpendicular import FullPerpendicularSimulation

    kw = dict(lib=lib) if lib is not None else dict(device=device)
    sim = FullPerpendicularSimulation(full_model, 5, n_substeps=2, env_params=True, **kw)
    assert sim.info["threads"] == 256
    sets = SP.full_cube_row_sets(full_model, _site_shift(full_model, sim))
    for e, key in enumerate(FULL_ENVS):
        if key == "scale+sites":      # through the product's own writer, then checked against the row set bit for bit
            mask = torch.zeros(5, dtype=torch.bool, device=sim.device); mask[e] = True
            sim.set_cube_size_multiplier(torch.full((5,), SP.CUBE_SCALE, device=sim.device), mask)
            sim.params["site_pos"][e] += torch.as_tensor(_site_shift(full_model, sim).astype(np.float32), device=sim.device)
        else:
            _write_rows(sim, e, sets[key])
    _write_rows(sim, 4, sets["inertia"])
    _sentinel(sim)
    return sim, sets


def _run_full_cube(full_model, truths, spread, lib, device):
    sim, sets = _full_cube_batch(full_model, lib, device)
    for e, key in enumerate(FULL_ENVS):
        for k, v in _rows_of(sim, e).items():
            assert np.array_equal(v, truths["full_cube", key][0][k]), (key, k)       # the env's rows ARE the row set the double values were computed from
    before4 = sim.params.block[4].cpu().numpy().copy()
    mask = torch.tensor([1, 1, 1, 1, 0], dtype=torch.bool, device=sim.device)
    sim.set_constants(mask)
    sim.sync()
    assert int(sim.status.max()) == 0
    A = full_model.arrays
    own = {k: np.asarray(A[k], dtype=np.float64).reshape(-1) for k in OUT}
    got = [_outputs_of(sim, e) for e in range(4)]
    for e, key in enumerate(FULL_ENVS):
        _check(got[e], truths["full_cube", key][1], spread, "full_cube", key, "env %d (%s)" % (e, key))
    _check(got[0], own, spread, "full_cube", "default", "env 0 against the model's arrays")
    assert np.array_equal(sim.params.block[4].cpu().numpy(), before4)                 # the masked env: bit-identical, sentinel included
    assert float(sim.params["dof_invweight0"][4, 0]) == SENTINEL
    for e, key in list(enumerate(FULL_ENVS))[1:]:                                     # stale rows would not pass: the new values are far from the model's
        for k in ("dof_invweight0", "body_invweight0"):
            nz = own[k] != 0
            far = np.abs(got[e][k] - own[k])[nz] / np.abs(own[k][nz])
            assert far.max() > 100 * _tol(spread, "full_cube", key, k), (key, k, far.max())
    return sim, got


def test_full_cube_set_constants_emul(full_model, truths, spread, emul_lib):
    """Full cube, B = 5, mask 0-3: default rows | body_inertia x U(0.5, 1.5) per body | cube scale 1.05 + site shift | body_mass x U(0.7, 1.3) on the cube bodies and
    dof_armature x 2 on the hand dofs; env 4 masked out."""
    _run_full_cube(full_model, truths, spread, emul_lib, "cpu")


def test_refresh_constants_on_large_simulation_emul(full_model, truths, spread, emul_lib):
    """`randomization.sim.refresh_constants(sim, rows)` works unchanged on a FullPerpendicularSimulation"""
    from robogym_amd.randomization.sim import refresh_constants

    sim, sets = _full_cube_batch(full_model, emul_lib, "cpu")
    refresh_constants(sim, [1])
    _check(_outputs_of(sim, 1), truths["full_cube", "inertia"][1], spread, "full_cube", "inertia", "refresh_constants row 1")
    for e in (0, 2, 3, 4):
        assert float(sim.params["dof_invweight0"][e, 0]) == SENTINEL


# ------------------------------------------------------------------------------------------------ the rearrange worlds (one-wave configurations)
def _run_rearrange(blocks_models, truths, spread, lib, device):
    from robogym_amd.mujoco.large_simulation import LargeModelSimulation

    for name, model in (("blocks5", blocks_models[0]), ("solver_world", blocks_models[1])):
        sim = LargeModelSimulation(model, 2, device=device, lib=lib, hand=False, env_params=True)
        assert sim.info["threads"] == 64
        _write_rows(sim, 1, truths[name, "changed"][0])
        _sentinel(sim)
        sim.set_constants()
        sim.sync()
        assert int(sim.status.max()) == 0
        A = model.arrays
        own = {k: np.asarray(A[k], dtype=np.float64).reshape(-1) for k in OUT}
        got = [_outputs_of(sim, e) for e in range(2)]
        assert got[0]["tendon_invweight0"].size == 0 and sim.params["tendon_invweight0"].shape == (2, 0)
        for e, key in enumerate(("default", "changed")):
            _check(got[e], truths[name, key][1], spread, name, key, "%s env %d (%s)" % (name, e, key))
        _check(got[0], own, spread, name, "default", name + " env 0 against the model's arrays")
        welded = np.flatnonzero(np.asarray(A["body_weldid"]) == 0)
        mocap = np.flatnonzero(np.asarray(A["body_mocapid"]) >= 0)
        assert len(mocap) >= 1 and set(mocap) <= set(welded) and len(welded) == (14 if name == "blocks5" else 9)
        for e in range(2):
            assert np.all(got[e]["body_invweight0"].reshape(-1, 2)[welded] == 0.0)
        for k in ("dof_invweight0", "body_invweight0"):
            nz = own[k] != 0
            far = np.abs(got[1][k] - own[k])[nz] / np.abs(own[k][nz])
            assert far.max() > 100 * _tol(spread, name, "changed", k), (name, k, far.max())


def test_rearrange_worlds_set_constants_emul(blocks_models, truths, spread, emul_lib):
    """blocks5 main world (small configuration: equalities, a mocap body, no tendon) and the solver world, B = 2 each: body_mass x 1.5 on the object bodies,
    dof_armature x 1.5, body_pos + 5 mm on two robot bodies."""
    _run_rearrange(blocks_models, truths, spread, emul_lib, "cpu")


# ------------------------------------------------------------------------------------------------ C ABI
def test_setconst_header_library_and_binding_agree():
    """include/rgstep_setconst.h (included by include/rgstep.h) under the rule tests/test_boundary.py applies to rgstep.h itself: the gfx950 build of the library
    exports every function the header declares, and the binding's list for it names exactly those."""
    import ctypes
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "rgstep_setconst.h")).read()
    declared = sorted(set(re.findall(r"\b(r[gba]_[a-z_0-9]+)\s*\(", text)))
    assert declared == ["rb_batch_set_constants"] and set(_native.EXPORTS_SETCONST) == set(declared)
    assert '#include "rgstep_setconst.h"' in open(os.path.join(root, "include", "rgstep.h")).read()
    path = os.path.join(root, "robogym_amd", "csrc", "librgstep.so")
    assert os.path.exists(path), "build it: python -c 'import __graft_entry__ as g; g.build()'"
    L = ctypes.CDLL(path)
    for name in declared:
        assert hasattr(L, name), name


# ------------------------------------------------------------------------------------------------ error paths
def test_set_constants_error_paths_emul(blocks_models, emul_lib):
    from robogym_amd.mujoco.large_simulation import LargeModelSimulation

    plain = LargeModelSimulation(blocks_models[1], 2, device="cpu", lib=emul_lib, hand=False)
    assert plain.set_constants() is None                           # the hand stepper's rule: without rows there is nothing to refresh
    rc = emul_lib.rb_batch_set_constants(plain._bh, None, None)    # the C entry point itself refuses, in rg_batch_set_constants' words
    msg = emul_lib.rg_last_error().decode()
    assert rc != 0 and "has no per-env parameter rows" in msg and "the model's own constants are already consistent" in msg
    sim = LargeModelSimulation(blocks_models[1], 2, device="cpu", lib=emul_lib, hand=False, env_params=True)
    with pytest.raises(AssertionError):
        sim.set_constants(torch.ones(3, dtype=torch.int32))
    assert emul_lib.rb_multi_begin() == 0                          # not recordable, like the other entry points that are no physics launch
    rc = emul_lib.rb_batch_set_constants(sim._bh, None, None)
    msg = emul_lib.rg_last_error().decode()
    assert emul_lib.rb_multi_launch(None) == 0
    assert rc != 0 and "not recordable" in msg
    sim.set_constants(torch.tensor([True, False]))                 # a bool mask is accepted
    assert int(sim.status.max()) == 0


# ------------------------------------------------------------------------------------------------ consequence in the physics
def _physics_after_set_constants(full_model, truths, lib, device, synchronise):
    """One env with the inertia AND the scale + site rows: set_constants(), then 2 env.steps of 2 substeps against OracleFullCube of the copied model WITH
    setconst.set_constants applied (protocol of test_large_env_params._full_mj_launches: state re-synchronised from the oracle before each launch)."""
    from robogym_amd.envs.dactyl.full_perpendicular import FullPerpendicularSimulation
    from robogym_amd.mujoco import setconst
    from robogym_amd.mujoco.big_tables import derive_big_tables

    kw = dict(lib=lib) if lib is not None else dict(device=device)
    sim = FullPerpendicularSimulation(full_model, 1, n_substeps=2, env_params=True, **kw)
    shift = _site_shift(full_model, sim)
    rows = truths["full_cube", "inertia+scale+sites"][0]
    model = _scaled_cube_model(full_model, SP.CUBE_SCALE, shift).copy_with(**{k: np.asarray(v, dtype=np.float64) for k, v in rows.items()})
    stale = {k: np.asarray(model.arrays[k], dtype=np.float64).copy() for k in OUT}
    setconst.set_constants(model)
    derive_big_tables(model)
    assert max(np.abs(model.arrays[k] - stale[k]).max() / np.abs(stale[k]).max() for k in OUT) > 1e-2      # the oracle's constants did change
    o = OracleFullCube(model, sim.pos_to_ctrl, sim.qpos_idxs["hand_angle"])
    o.hold_pose()
    for _ in range(60):
        o.sim.step()
    states = []
    for _ in range(2):
        states.append((o.state_f32(), float(o.sim.time)))
        o.sim.sim_step(2); o.sim.forward()
    # ---- the device side: row writes, set_constants and the launches in stream order
    sim.params["body_inertia"][0] = torch.as_tensor(rows["body_inertia"], device=sim.device)
    sim.set_cube_size_multiplier(SP.CUBE_SCALE)
    sim.params["site_pos"][0] += torch.as_tensor(shift.astype(np.float32), device=sim.device)
    sim.set_constants()
    errs = []
    ref = [None, None]
    for k, (st, t) in enumerate(states):
        for name, view in (("qpos", sim.qpos), ("qvel", sim.qvel), ("pid", sim.pid), ("warm", sim.qacc_warmstart), ("ctrl", sim.ctrl)):
            view[0] = torch.as_tensor(st[name], device=sim.device)
        sim.view(_native.RG_F_TIME)[0, 0] = t
        sim.env_step(nsubsteps=2, nforward_ticks=1)
        if synchronise:
            sim.sync()
            ref[k] = (sim.qpos[0].cpu().numpy().copy(), sim.qvel[0].cpu().numpy().copy())
    final = (sim.qpos[0].cpu().numpy().astype(np.float64), sim.qvel[0].cpu().numpy().astype(np.float64), int(sim.status.max()))
    for k in SP.ROW_FIELDS:
        assert np.array_equal(sim.params[k][0].cpu().numpy(), rows[k]), k
    return sim, o, final, ref, states


def test_full_cube_physics_after_set_constants_emul(full_model, truths, spread, emul_lib, oracle_lib):
    """bounds of test_full_cube_rows_match_per_env_oracles_emul for its `scale+sites` row: qpos < 5e-4, qvel < 5e-2, status 0"""
    oracle_lib.set_kernel_variant(False)
    sim, o, final, ref, states = _physics_after_set_constants(full_model, truths, emul_lib, "cpu", True)
    # after launch k the oracle stood at states[k + 1] (launch 0) / its final state (launch 1)
    e0 = (np.abs(ref[0][0] - states[1][0]["qpos"]).max(), np.abs(ref[0][1] - states[1][0]["qvel"]).max())
    e1 = (np.abs(final[0] - o.sim.qpos).max(), np.abs(final[1] - o.sim.qvel).max())
    print("physics after set_constants: qpos err %.2e / %.2e, qvel err %.2e / %.2e" % (e0[0], e1[0], e0[1], e1[1]))
    assert final[2] == 0
    assert max(e0[0], e1[0]) < 5e-4 and max(e0[1], e1[1]) < 5e-2
    _check(_outputs_of(sim, 0), truths["full_cube", "inertia+scale+sites"][1], spread, "full_cube", "inertia+scale+sites", "combined env")


# ------------------------------------------------------------------------------------------------ env flag
def test_env_set_constants_on_reset_emul(full_model, truths, spread, emul_lib):
    from robogym_amd.envs.dactyl.full_perpendicular import make_simple_env

    small = dict(mujoco_substeps=1, reset_initial_steps=1, n_random_initial_steps=1, max_pose_resets=1, num_scramble_steps=4)
    kw = dict(parameters={"cube_size_multiplier": SP.CUBE_SCALE}, constants=small, starting_seed=1, batch_size=2, model=full_model, lib=emul_lib, per_env_parameters=True)
    env = make_simple_env(set_constants_on_reset=True, **kw)
    env.reset()
    sim = env.mujoco_simulation
    assert int(sim.status.max()) == 0
    for k, v in _rows_of(sim, 0).items():
        assert np.array_equal(v, truths["full_cube", "scale"][0][k]), k
    for e in range(2):
        _check(_outputs_of(sim, e), truths["full_cube", "scale"][1], spread, "full_cube", "scale", "flag on, env %d" % e)
    off = make_simple_env(**kw)
    off.reset()
    A = full_model.arrays
    for k in OUT:                                                    # flag off: the unscaled model's values, bit for bit
        want = np.asarray(A[k], dtype=np.float32).reshape(-1)
        for e in range(2):
            assert np.array_equal(off.mujoco_simulation.params[k][e].cpu().numpy().reshape(-1), want), k
    with pytest.raises(ValueError, match="set_constants_on_reset"):
        make_simple_env(set_constants_on_reset=True, pipelined_reset=True, **kw)


# ------------------------------------------------------------------------------------------------ MI355X
@pytest.mark.gpu
def test_full_cube_set_constants_gpu(full_model, truths, spread):
    """The full-cube test on the GPU at B = 5 (the large configuration's kernel can go wrong at any B >= 1, the mask needs >= 2 envs)."""
    _run_full_cube(full_model, truths, spread, None, "cuda:0")


@pytest.mark.gpu
def test_full_cube_set_constants_gpu_against_emulation_gpu(full_model, truths, spread, emul_lib):
    """The GPU's three rows against the emulation harness's, same batch: within 2 x the tolerance."""
    sim, got = _run_full_cube(full_model, truths, spread, None, "cuda:0")
    esim, egot = _run_full_cube(full_model, truths, spread, emul_lib, "cpu")
    for e, key in enumerate(FULL_ENVS):
        _check(got[e], egot[e], spread, "full_cube", key, "GPU against emulation, env %d" % e, factor=2.0)


@pytest.mark.gpu
def test_rearrange_worlds_set_constants_gpu(blocks_models, truths, spread):
    _run_rearrange(blocks_models, truths, spread, None, "cuda:0")


@pytest.mark.gpu
def test_full_cube_physics_after_set_constants_stream_order_gpu(full_model, truths, spread, oracle_lib):
    """Row writes, set_constants() and the two env_steps without any synchronisation in between; the only readback is at the end.  Same bounds as on the harness."""
    oracle_lib.set_kernel_variant(False)
    sim, o, final, ref, states = _physics_after_set_constants(full_model, truths, None, "cuda:0", False)
    e1 = (np.abs(final[0] - o.sim.qpos).max(), np.abs(final[1] - o.sim.qvel).max())
    print("physics after set_constants (GPU, stream order): qpos err %.2e, qvel err %.2e" % e1)
    assert final[2] == 0 and e1[0] < 5e-4 and e1[1] < 5e-2
    _check(_outputs_of(sim, 0), truths["full_cube", "inertia+scale+sites"][1], spread, "full_cube", "inertia+scale+sites", "combined env (GPU)")
