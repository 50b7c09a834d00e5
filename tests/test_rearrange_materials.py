"""Per-object materials of the rearrange envs (`material_names`): stage RA_ROWS_MATERIAL of ra_param_rows_kernel draws or takes a material per
slot where an episode ended and writes its rows on top of the restored parameter block.  The table against the fixture made from the reference's files, the rows in
closed form and against the host mj_setConst, the default list as the identity, the physics on the rows against per-env oracle worlds, the draws against a host
restatement of the generator, the damping rule through the recipe, the randomizers on top, parking, the refusals.  Every check of the kernel runs twice: on the
emulation harness (CPU, the same kernel source) and, `-m gpu`, on the MI355X through the C ABI."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from robogym_amd import _native
from robogym_amd.envs.rearrange import blocks, holdout, materials, ycb
from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv
from robogym_amd.envs.rearrange.xml import load_blocks_model, load_solver_model, load_ycb_model
from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv, GroupedYcbRearrangeEnv
from robogym_amd.mujoco import setconst

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = materials.MATERIAL_NAMES
ALL = list(NAMES)
IDX = {n: i for i, n in enumerate(NAMES)}
H = 0.0254      # the blocks' half edge
RESTORE, MATERIAL, PARK = _native.RA_ROWS_RESTORE, _native.RA_ROWS_MATERIAL, _native.RA_ROWS_PARK


def _kw(lib, **more):
    """the recipe stages the neighbouring tests use: the shortest on the emulator, a short real recipe on the GPU"""
    if lib is not None:
        kw = dict(device="cpu", lib=lib, n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
    else:
        kw = dict(device="cuda:0", n_substeps=40, stabilize_steps=10, n_random_initial_steps=1, settle_steps=5)
    kw.update(more)
    return kw


def _ok(*envs):
    for env in envs:
        env.sync()
        assert int(env.sim.status.max()) == 0
        if env.solver_sim is not None:
            assert int(env.solver_sim.status.max()) == 0


def _launch(env, stages, ended=0, stabilised=0, started=0, step=None):
    """one direct launch of ra_env_param_rows on masks written here"""
    for row, v in ((env.ended, ended), (env.stabilised, stabilised), (env.episode_started, started)):
        row.copy_(torch.as_tensor(np.broadcast_to(np.asarray(v), (env.B,)).astype(bool).copy(), device=env.device))
    if step is not None:
        env.recipe.step = int(step)
    env._param_rows_launch(stages)
    env.sync()


def _np(t):
    return t.detach().cpu().numpy()


def _object_geoms(env, i):
    a = env.param_rows
    return np.arange(a.obj_geomadr[i], a.obj_geomadr[i] + a.obj_geomnum[i])


def _f32(v):
    return np.asarray(v, dtype=np.float32)


# ------------------------------------------------------------------------------------------------ 1. the table
def test_package_table_is_the_fixture():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "rearrange_materials.json")))
    assert golden == materials.MATERIALS and sorted(golden) == NAMES == ["chess", "default", "painted_wood", "rubber-ball", "tangram"]
    T = materials.material_table()
    assert T.shape == (5, _native.RA_MAT_WORDS) and T.dtype == np.float32 and not T[IDX["default"]].any()
    every = _native.RA_MAT_MASS | _native.RA_MAT_FRICTION | _native.RA_MAT_SOLREF | _native.RA_MAT_JOINT
    for n in NAMES:
        if n != "default":
            assert int(T[IDX[n], 0]) == every | (_native.RA_MAT_SOLIMP if n == "chess" else 0), n
            assert T[IDX[n], 1] == np.float32(golden[n]["density"] / 1000.0) and list(T[IDX[n], 10:]) == [0.0, 0.0]
    # the compiled worlds carry `default`: its joint entry is the model's, its geoms have the model density
    m = load_blocks_model(2)
    dof = int(m.arrays["jnt_dofadr"][m.names["joint"].index("object0:joint")])
    assert np.all(m.arrays["dof_damping"][dof:dof + 6] == golden["default"]["joint_damping"]) and np.all(m.arrays["dof_armature"][dof:dof + 6] == golden["default"]["joint_armature"])
    assert np.isclose(m.arrays["body_mass"][m.name2id("body", "object0")], materials.MODEL_DENSITY * (2 * H) ** 3, rtol=1e-9)
    assert materials.material_list(None) == NAMES and materials.material_list([]) == NAMES and materials.material_list(["tangram", "tangram"]) == ["tangram", "tangram"]


# ------------------------------------------------------------------------------------------------ 2. the rows, in closed form
def _expected_model(env, e, mats):
    """env e's own world on the host: `copy_with` of the table's values for the materials `mats` (per slot) and the host mj_setConst"""
    A, a = env.model.arrays, env.param_rows
    over = {k: np.array(A[k], dtype=np.float64) for k in ("geom_friction", "geom_solref", "geom_solimp", "body_mass", "body_inertia", "dof_armature", "dof_damping")}
    for i, name in enumerate(mats):
        m = materials.MATERIALS[name]
        if name == "default":
            continue
        w = i if env.object_perm is None else int(env.object_perm[e, i])
        g, b, d = _object_geoms(env, w), int(a.obj_body[w]), int(a.obj_dofadr[w])
        over["geom_friction"][g] = _f32(m["friction"]).astype(np.float64)
        over["geom_solref"][g] = _f32(m["solref"]).astype(np.float64)
        if m["solimp"] is not None:
            over["geom_solimp"][g, :3] = _f32(m["solimp"]).astype(np.float64)
        over["body_mass"][b] *= m["density"] / materials.MODEL_DENSITY
        over["body_inertia"][b] *= m["density"] / materials.MODEL_DENSITY
        over["dof_armature"][d:d + 6] = m["joint_armature"]
        over["dof_damping"][d:d + 6] = m["joint_damping"]
    return setconst.set_constants(env.model.copy_with(**over))


def _rows_closed_form(env, pins, blocks_world):
    B, N = env.B, env.N
    env.set_object_material_next(pins)
    default = _np(env._param_block_default).copy()
    _launch(env, RESTORE | MATERIAL, ended=1)
    P, a, A = env.sim.params, env.param_rows, env.model.arrays
    assert np.array_equal(_np(env.object_material), pins)
    rows = _np(env.sim.view(_native.RG_F_DEBUG))
    lo = (P.block.data_ptr() - env.sim.view(_native.RG_F_DEBUG).data_ptr()) // 4
    off = {k: (P[k].data_ptr() - env.sim.view(_native.RG_F_DEBUG).data_ptr()) // 4 - lo for k in P.keys()}
    block = rows[:, lo:lo + default.size]
    for e in range(B):
        mats = [NAMES[k] for k in pins[e]]
        want = _expected_model(env, e, mats).arrays
        touched = np.zeros(default.size, dtype=bool)
        for i, name in enumerate(mats):
            m = materials.MATERIALS[name]
            g, b, d = _object_geoms(env, i), int(a.obj_body[i]), int(a.obj_dofadr[i])
            touched[off["dof_damping"] + d:off["dof_damping"] + d + 6] = True      # (stabilize_damping, the restore stage's)
            assert np.all(_np(P["dof_damping"][e, d:d + 6]) == np.float32(env.stabilize_object_damping))
            if name == "default":
                continue
            for key, width in (("geom_friction", 3), ("geom_solref", 2), ("geom_solimp", 5)):
                for gg in g:
                    touched[off[key] + width * gg:off[key] + width * gg + (3 if key == "geom_solimp" else width)] = True
            touched[off["body_mass"] + b] = True
            touched[off["body_inertia"] + 3 * b:off["body_inertia"] + 3 * b + 3] = True
            touched[off["body_invweight0"] + 2 * b:off["body_invweight0"] + 2 * b + 2] = True
            for key in ("dof_armature", "dof_invweight0"):
                touched[off[key] + d:off[key] + d + 6] = True
            # the float32 of the table's value, exactly
            assert np.array_equal(_np(P["geom_friction"][e, g]), np.tile(_f32(m["friction"]), (len(g), 1))), (e, i, name)
            assert np.array_equal(_np(P["geom_solref"][e, g]), np.tile(_f32(m["solref"]), (len(g), 1))), (e, i, name)
            solimp = _f32(A["geom_solimp"][g]).copy()
            if m["solimp"] is not None:
                solimp[:, :3] = _f32(m["solimp"])
            assert np.array_equal(_np(P["geom_solimp"][e, g]), solimp), (e, i, name)
            assert np.all(_np(P["dof_armature"][e, d:d + 6]) == np.float32(m["joint_armature"]))
            # density acts through mass: three fp32 roundings (the model's row, the ratio, their product) at 6e-8 each
            k = m["density"] / materials.MODEL_DENSITY
            mass, inertia = float(P["body_mass"][e, b]), _np(P["body_inertia"][e, b]).astype(np.float64)
            if blocks_world:
                assert np.isclose(mass, m["density"] * (2 * H) ** 3, rtol=1e-6, atol=0) and np.allclose(inertia, m["density"] * (2 * H) ** 3 * (2 * H) ** 2 / 6, rtol=1e-6, atol=0), (e, i, name)
            assert np.isclose(mass / A["body_mass"][b], k, rtol=1e-6, atol=0) and np.allclose(inertia / A["body_inertia"][b], k, rtol=1e-6, atol=0), (e, i, name)
            # both _invweight0 rows: the host mj_setConst on this env's own world
            assert np.allclose(_np(P["dof_invweight0"][e, d:d + 6]), want["dof_invweight0"][d:d + 6], rtol=1e-5, atol=0), (e, i, name, _np(P["dof_invweight0"][e, d:d + 6]), want["dof_invweight0"][d:d + 6])
            assert np.allclose(_np(P["body_invweight0"][e, b]), want["body_invweight0"][b], rtol=1e-5, atol=0), (e, i, name, _np(P["body_invweight0"][e, b]), want["body_invweight0"][b])
        # every other word of the block: block_default's bits
        assert np.array_equal(block[e][~touched].view(np.uint32), default[~touched].view(np.uint32)), e
    _ok(env)


def _rows_blocks(lib):
    env = BatchedBlockRearrangeEnv(4, num_objects=2, device_reset=True, material_names=ALL, **_kw(lib))
    pins = np.array([[IDX["chess"], IDX["default"]], [IDX["painted_wood"], IDX["rubber-ball"]], [IDX["tangram"], IDX["chess"]], [IDX["default"], IDX["tangram"]]], dtype=np.int32)
    assert set(pins.ravel()) == set(range(5))
    _rows_closed_form(env, pins, blocks_world=True)


def _rows_ycb(lib):
    """ycb set 5, B = 2: the ratio of mass and inertia to the model is density / 1000, every convex part of an object carries its material's rows, and the centre of
    mass of a mesh object lies off its free joint (obj_lever2)"""
    env = BatchedYcbRearrangeEnv(2, device_reset=True, material_names=ALL, main_model=load_ycb_model(8, set_index=5), **_kw(lib))
    assert max(env.param_rows.obj_geomnum[i] for i in range(8)) > 1 and max(env.param_rows.obj_lever2[i][k] for i in range(8) for k in range(3)) > 0
    pins = np.array([[0, 1, 2, 3, 4, 0, 2, 4], [4, 3, 2, 1, 0, 3, 3, 1]], dtype=np.int32)
    _rows_closed_form(env, pins, blocks_world=False)


def test_rows_closed_form_blocks_emul(emul_lib):
    _rows_blocks(emul_lib)


def test_rows_closed_form_ycb_emul(emul_lib):
    _rows_ycb(emul_lib)


@pytest.mark.gpu
def test_rows_closed_form_blocks_gpu():
    _rows_blocks(None)


@pytest.mark.gpu
def test_rows_closed_form_ycb_gpu():
    _rows_ycb(None)


# ------------------------------------------------------------------------------------------------ 3. default is the identity
def _default_is_identity(lib):
    kw = _kw(lib, starting_seed=5, device_reset=True, num_objects=2)
    plain, named, pinned = BatchedBlockRearrangeEnv(2, **kw), BatchedBlockRearrangeEnv(2, material_names=["default"], **kw), BatchedBlockRearrangeEnv(2, material_names=ALL, **kw)
    for env in (plain, named):      # nothing new is requested: no field, no stage bit, no allocation
        a = env.param_rows
        assert not env.materials_on and env.object_material is None and env.object_material_next is None and env.material_names == ["default"]
        assert not a.mat_table and not a.obj_material and not a.obj_material_next and a.num_materials == 0 and a.num_choice == 0 and env._row_stages() == RESTORE | PARK
    assert pinned.materials_on and pinned._row_stages() == RESTORE | MATERIAL | PARK and pinned.material_names == NAMES
    pinned.set_object_material_next("default")
    rng = np.random.RandomState(2)
    for env in (plain, named, pinned):
        env.reset()
    for k in range(3):
        if k:
            a = torch.tensor(rng.uniform(-1, 1, plain.action_shape).astype(np.float32), device=plain.device)
            obs = [env.step(a)[0] for env in (plain, named, pinned)]
        for name in ("packed", "goal", "yaw", "static_obs"):
            assert torch.equal(getattr(plain, name), getattr(named, name)) and torch.equal(getattr(plain, name), getattr(pinned, name)), (k, name)
        assert torch.equal(plain.sim.qpos, named.sim.qpos) and torch.equal(plain.sim.qpos, pinned.sim.qpos), k
        assert torch.equal(plain.sim.params.block.view(torch.int32), named.sim.params.block.view(torch.int32)), k
        assert torch.equal(plain.sim.params.block.view(torch.int32), pinned.sim.params.block.view(torch.int32)), k
    assert bool((pinned.object_material == IDX["default"]).all())
    _ok(plain, named, pinned)


def test_default_is_identity_emul(emul_lib):
    _default_is_identity(emul_lib)


@pytest.mark.gpu
def test_default_is_identity_gpu():
    _default_is_identity(None)


# ------------------------------------------------------------------------------------------------ 4. the physics reads the rows
PHYSICS_MATERIALS = ("rubber-ball", "tangram", "chess")


def _physics(lib, n_substeps, nsteps):
    """tests/test_rearrange_env_params.py `_run`, its protocol unchanged (5-block world, three envs, `_oracle_env(settle=30)`: the blocks rest on the table, so their
    contacts mix the material's direct, negative solref with the table's positive one), the rows produced by the stage: every block of env e has PHYSICS_MATERIALS[e],
    and each env is compared with ITS OWN oracle world, `copy_with` of the same values plus the host mj_setConst."""
    from tests.test_rearrange_kernel import _oracle_env, sync_from_oracle

    main, solver = load_blocks_model(5), load_solver_model()
    kw = _kw(lib, n_substeps=n_substeps)
    env = BatchedBlockRearrangeEnv(3, num_objects=5, device_reset=True, material_names=ALL, main_model=main, **kw)
    env.set_object_material_next(np.array([[IDX[n]] * 5 for n in PHYSICS_MATERIALS]))
    _launch(env, RESTORE | MATERIAL, ended=1)
    _launch(env, RESTORE | MATERIAL, stabilised=1)      # (stabilize_objects' end: the material's damping, 0)
    sim = env.sim
    assert np.all(_np(sim.params["dof_damping"][:, env.obj_dofs]) == 0)
    oras = [_oracle_env((_expected_model(env, e, [n] * 5), solver), n_substeps, settle=30, seed=2).main for e, n in enumerate(PHYSICS_MATERIALS)]
    rng = np.random.RandomState(1)
    errs = []
    for step in range(nsteps):
        for e, o in enumerate(oras):
            o.sim.ctrl[:6] += 0.02 * rng.randn(6)
            sync_from_oracle(sim, o.sim, row=e)
        sim.env_step(nforward_ticks=1)
        sim.sync()
        row = []
        for e, o in enumerate(oras):
            o.step()
            row.append((float(np.abs(sim.qpos[e].cpu().numpy() - o.sim.qpos).max()), float(np.abs(sim.qvel[e].cpu().numpy() - o.sim.qvel).max())))
        errs.append(row)
        assert int(sim.status.max()) == 0
    return np.array(errs), oras


def _report(errs):
    for e, n in enumerate(PHYSICS_MATERIALS):
        print("env %d (%s): qpos median %.2e max %.2e | qvel median %.2e max %.2e" % (e, n, np.median(errs[:, e, 0]), errs[:, e, 0].max(), np.median(errs[:, e, 1]), errs[:, e, 1].max()))


def test_physics_reads_the_material_rows_emul(emul_lib, oracle_lib):
    errs, oras = _physics(emul_lib, n_substeps=2, nsteps=2)
    _report(errs)
    assert errs[:, :, 0].max() < 2e-6 and errs[:, :, 1].max() < 5e-4, errs
    q = [o.sim.qpos.copy() for o in oras]
    assert np.abs(q[0] - q[1]).max() > 1e-5 and np.abs(q[0] - q[2]).max() > 1e-5 and np.abs(q[1] - q[2]).max() > 1e-5


@pytest.mark.gpu
def test_physics_reads_the_material_rows_gpu(oracle_lib):
    errs, oras = _physics(None, n_substeps=40, nsteps=4)
    _report(errs)
    assert np.median(errs[:, :, 0]) < 5e-6 and errs[:, :, 0].max() < 5e-3 and np.median(errs[:, :, 1]) < 5e-4, errs
    q = [o.sim.qpos.copy() for o in oras]
    assert np.abs(q[0] - q[1]).max() > 1e-5 and np.abs(q[0] - q[2]).max() > 1e-5 and np.abs(q[1] - q[2]).max() > 1e-5


# ------------------------------------------------------------------------------------------------ 5. the draws
M32 = 0xFFFFFFFF


def _env_hash(a, b, c, d):
    """env_hash of csrc/rg_env_common.h, restated on Python integers"""
    h = ((a * 0x9E3779B1) & M32) ^ (((b + 0x7F4A7C15) & M32) * 0x85EBCA77 & M32)
    h ^= h >> 15; h = h * 0xC2B2AE3D & M32; h ^= ((c + 0x165667B1) & M32) * 0x27D4EB2F & M32; h ^= h >> 13; h = h * 0x9E3779B1 & M32
    h ^= ((d + 0xD6E8FEB8) & M32) * 0x85EBCA77 & M32; h ^= h >> 16; h = h * 0xC2B2AE3D & M32; h ^= h >> 15; h = h * 0x27D4EB2F & M32; h ^= h >> 13
    return h


def _host_draws(seed, step, B, N, choice, pins=None, groups=None):
    """the stage's choice of materials on the host: env_u01 on the stream 0x165667B1 from draw 4000 + slot, a pin where one is given, a group's lowest slot for its members"""
    out = np.zeros((B, N), dtype=np.int32)
    for e in range(B):
        for s in range(N):
            u = np.float32(_env_hash(seed ^ 0x165667B1, step, e, 4000 + s) >> 8) * np.float32(1.0 / 16777216.0)
            c = min(int(np.float32(u * np.float32(len(choice)))), len(choice) - 1)
            out[e, s] = choice[c] if pins is None or pins[e, s] < 0 else pins[e, s]
        if groups is not None:
            out[e] = [out[e, min(j for j in range(N) if groups[e][j] == groups[e][s])] for s in range(N)]
    return out


def _draws(lib):
    names = ["painted_wood", "tangram", "tangram"]
    choice = [IDX[n] for n in names]
    kw = _kw(lib, num_objects=4, device_reset=True, material_names=names, starting_seed=11)
    env = BatchedBlockRearrangeEnv(32, **kw)
    seed = int(env.recipe.seed)
    assert env.param_rows.mat_seed == seed and [env.param_rows.mat_choice[k] for k in range(3)] == choice and env.param_rows.num_choice == 3
    _launch(env, RESTORE | MATERIAL, ended=1, step=7)
    first = _np(env.object_material).copy()
    assert set(first.ravel()) <= set(choice)
    tangram = int((first == IDX["tangram"]).sum())
    print("tangram %d of 128 draws" % tangram)
    assert abs(tangram - 85) <= 21      # 4 sigma of Binomial(128, 2 / 3)
    assert np.array_equal(first, _host_draws(seed, 7, 32, 4, choice))      # both tiers: the generator restated on the host
    _launch(env, RESTORE | MATERIAL, ended=1, step=8)
    second = _np(env.object_material).copy()
    assert not np.array_equal(first, second) and np.array_equal(second, _host_draws(seed, 8, 32, 4, choice))
    # an env whose episode did not end keeps its row
    ended = np.arange(32) % 2 == 0
    _launch(env, RESTORE | MATERIAL, ended=ended, stabilised=~ended, step=9)
    third = _np(env.object_material)
    assert np.array_equal(third[~ended], second[~ended]) and np.array_equal(third[ended], _host_draws(seed, 9, 32, 4, choice)[ended])
    # a pinned slot keeps its pin while its neighbours draw (the pin may name any material of the table, and stays)
    pins = np.full((32, 4), -1, dtype=np.int32); pins[:, 2] = IDX["chess"]; pins[5, 0] = IDX["default"]
    env.set_object_material_next(pins)
    for step in (10, 11):
        _launch(env, RESTORE | MATERIAL, ended=1, step=step)
        got = _np(env.object_material)
        assert np.all(got[:, 2] == IDX["chess"]) and got[5, 0] == IDX["default"] and np.array_equal(got, _host_draws(seed, step, 32, 4, choice, pins=pins))
    assert len(set(got[:, 1])) == 2 and np.array_equal(_np(env.object_material_next), pins)
    # groups: members take the material of their group's lowest slot
    grouped = BatchedBlockRearrangeEnv(32, object_groups=[2, 2], **kw)
    assert _np(grouped.obj_group[0]).tolist() == [0, 0, 1, 1] and grouped.param_rows.obj_group
    _launch(grouped, RESTORE | MATERIAL, ended=1, step=7)
    got = _np(grouped.object_material)
    assert np.array_equal(got[:, 0], got[:, 1]) and np.array_equal(got[:, 2], got[:, 3]) and np.array_equal(got[:, [0, 2]], first[:, [0, 2]])
    assert np.array_equal(got, _host_draws(seed, 7, 32, 4, choice, groups=_np(grouped.obj_group))) and not np.array_equal(got[:, 0], got[:, 2])
    _ok(env, grouped)


def test_draws_emul(emul_lib):
    _draws(emul_lib)


@pytest.mark.gpu
def test_draws_gpu():
    _draws(None)


# ------------------------------------------------------------------------------------------------ 6. damping through the recipe
def _damping(lib):
    env = BatchedBlockRearrangeEnv(2, num_objects=2, device_reset=True, material_names=ALL, starting_seed=1, **_kw(lib))
    env.set_object_material_next(["tangram", "default"])
    damping = lambda: _np(env.sim.params["dof_damping"][:, env.obj_dofs]).reshape(2, 2, 6)
    model = _f32(env.model.arrays["dof_damping"][_np(env.obj_dofs)]).reshape(2, 6)
    assert np.all(model == np.float32(0.01))
    _launch(env, RESTORE | MATERIAL | PARK, ended=1)
    assert np.all(damping() == np.float32(env.stabilize_object_damping))
    _launch(env, RESTORE | MATERIAL | PARK, stabilised=1)
    assert np.all(damping()[:, 0] == 0) and np.array_equal(damping()[:, 1], np.tile(model[1], (2, 1)))
    env.reset()
    assert np.all(damping()[:, 0] == 0) and np.array_equal(damping()[:, 1], np.tile(model[1], (2, 1)))
    assert _np(env.object_material).tolist() == [[IDX["tangram"], IDX["default"]]] * 2
    _ok(env)


def test_damping_through_the_recipe_emul(emul_lib):
    _damping(emul_lib)


@pytest.mark.gpu
def test_damping_through_the_recipe_gpu():
    _damping(None)


# ------------------------------------------------------------------------------------------------ 7. the randomizers on top
def _randomizers(lib):
    """The randomizers start from the rows as they stand at the episode's start, block + material.  (chess is left out: GeomSolimpRandomizer clips dmax into
    [0.5, 0.99] at parameter 0 too, as the reference's does, and chess's 0.999 lies outside.)"""
    kw = _kw(lib, num_objects=2, device_reset=True, material_names=ALL, starting_seed=1)
    pins = ["tangram", "rubber-ball"]
    same = BatchedBlockRearrangeEnv(2, randomizer_params={"geom_friction": (0.0, 0.0), "body_mass": (0.0, 0.0)}, **kw)
    twice = BatchedBlockRearrangeEnv(2, randomizer_params={"geom_friction": (float(np.log(2.0)), 0.0)}, **kw)
    for env in (same, twice):
        env.set_object_material_next(pins)
        env.reset()
    A = same.model.arrays
    for i, name in enumerate(pins):
        m, a = materials.MATERIALS[name], same.param_rows
        g, b = _object_geoms(same, i), int(a.obj_body[i])
        k = np.float32(m["density"] / materials.MODEL_DENSITY)
        for e in range(2):
            P = same.sim.params
            assert np.array_equal(_np(P["geom_friction"][e, g]), np.tile(_f32(m["friction"]), (len(g), 1)))
            assert np.array_equal(_np(P["geom_solref"][e, g]), np.tile(_f32(m["solref"]), (len(g), 1)))
            assert np.array_equal(_np(P["geom_solimp"][e, g]), _f32(A["geom_solimp"][g]))
            assert float(P["body_mass"][e, b]) == np.float32(A["body_mass"][b]) * k and np.array_equal(_np(P["body_inertia"][e, b]), _f32(A["body_inertia"][b]) * k)
            got = _np(twice.sim.params["geom_friction"][e, g])
            print("friction x exp(log 2):", got[0], "material", _f32(m["friction"]))
            assert np.array_equal(got, np.tile(np.float32(2.0) * _f32(m["friction"]), (len(g), 1)))
    # a geom that is no object's keeps the model's friction, doubled
    table = same.model.names["geom"].index("table")
    assert np.array_equal(_np(twice.sim.params["geom_friction"][0, table]), np.float32(2.0) * _f32(A["geom_friction"][table]))
    _ok(same, twice)


def test_randomizers_on_top_emul(emul_lib):
    _randomizers(emul_lib)


@pytest.mark.gpu
def test_randomizers_on_top_gpu():
    _randomizers(None)


# ------------------------------------------------------------------------------------------------ 8. parking
def _parking(lib):
    env = BatchedBlockRearrangeEnv(2, num_objects=2, max_num_objects=3, device_reset=True, material_names=ALL, starting_seed=2, **_kw(lib))
    env.set_object_material_next([-1, -1, IDX["rubber-ball"]])
    env.reset()
    assert env.num_active.tolist() == [2, 2] and bool((env.object_material[:, 2] == IDX["rubber-ball"]).all())
    P, b = env.sim.params, int(env.param_rows.obj_body[2])
    mass = np.float32(env.model.arrays["body_mass"][b]) * np.float32(1100.0 / 1000.0)
    for e in range(2):
        assert float(P["body_mass"][e, b]) == mass
        assert np.array_equal(_np(P["xfrc_applied"][e, b, :3]), -mass * _np(P["gravity"][e])) and not _np(P["xfrc_applied"][e, b, 3:]).any()
        assert np.all(_np(P["dof_damping"][e, env.obj_v[2]:env.obj_v[2] + 6]) == np.float32(blocks.PARK_DAMPING))
    _ok(env)


def test_parking_cancels_the_materials_weight_emul(emul_lib):
    _parking(emul_lib)


@pytest.mark.gpu
def test_parking_cancels_the_materials_weight_gpu():
    _parking(None)


# ------------------------------------------------------------------------------------------------ 9. refusals and the ABI
def _refusals(lib):
    kw = _kw(lib, num_objects=2)
    with pytest.raises(ValueError, match="unknown material 'granite'.*chess, default, painted_wood, rubber-ball, tangram"):
        BatchedBlockRearrangeEnv(2, device_reset=True, material_names=["default", "granite"], **kw)
    with pytest.raises(NotImplementedError, match="material_names"):      # the host route
        BatchedBlockRearrangeEnv(2, material_names=["tangram"], **kw)
    with pytest.raises(ValueError, match="material_names.*per_env_parameters=True"):
        BatchedBlockRearrangeEnv(2, device_reset=True, per_env_parameters=False, material_names=["tangram"], **kw)
    with pytest.raises(NotImplementedError, match="material_names.*grouped ycb env"):
        GroupedYcbRearrangeEnv(4, object_sets=(0, 1), device_reset=True, material_names=["tangram"], **_kw(lib))
    with pytest.raises(NotImplementedError, match="material_names"):
        holdout.make_env(batch_size=2, parameters={"material_names": ["tangram"]}, **kw)
    with pytest.raises(NotImplementedError, match="per-group material_args"):      # per-group material_args stay refused
        blocks.make_env(batch_size=2, parameters={"simulation_params": {"num_objects": 2, "object_groups": [{"count": 2, "material_args": {"geom": {"density": "720.0"}}}]}, "material_names": ["tangram"]},
                        device_reset=True, **_kw(lib))
    env = blocks.make_env(batch_size=2, parameters={"simulation_params": {"num_objects": 2}, "material_names": None}, device_reset=True, **_kw(lib))
    assert env.material_names == NAMES and env.materials_on and env.object_material.shape == (2, 2) and env.object_material.dtype == torch.int32
    e2 = ycb.make_env(batch_size=2, parameters={"simulation_params": {"num_objects": 8}, "material_names": ["chess", "default"]}, device_reset=True, **_kw(lib))
    assert e2.material_names == ["chess", "default"] and e2.param_rows.num_choice == 2
    for call in (lambda: env.reset(on_device=False), lambda: env.reset_goals(on_device=False)):
        with pytest.raises(NotImplementedError, match="material_names"):
            call()
    for bad in (["granite", "default"], [5, 0], [-2, 0], [0, 1, 2], 0.5):
        with pytest.raises(ValueError, match="object_material_next"):
            env.set_object_material_next(bad)
    env.set_object_material_next([IDX["chess"], -1], rows=[1])
    assert _np(env.object_material_next).tolist() == [[-1, -1], [IDX["chess"], -1]]
    plain = BatchedBlockRearrangeEnv(2, device_reset=True, **kw)
    with pytest.raises(ValueError, match="set_object_material_next"):
        plain.set_object_material_next("tangram")
    # the launch: every refusal a named error
    L, a = env._L, env.param_rows
    launch = lambda args=a, e=env: L.ra_env_param_rows(e.sim._bh, ctypes.byref(args), None)

    def refused(field, value, message, index=None):
        target = a if index is None else getattr(a, field)
        had = getattr(a, field) if index is None else target[index]
        try:
            if index is None:
                setattr(a, field, value)
            else:
                target[index] = value
            assert launch() != 0 and message in L.rg_last_error(), (field, L.rg_last_error())
        finally:
            if index is None:
                setattr(a, field, had)
            else:
                target[index] = had

    a.stages = RESTORE | MATERIAL
    assert launch() == 0
    refused("stages", 8, b"stages")
    refused("stages", 0, b"stages")
    refused("mat_table", None, b"RA_ROWS_MATERIAL needs mat_table")
    refused("mat_choice", 5, b"material index out of range", index=0)
    refused("mat_choice", -1, b"material index out of range", index=1)
    refused("num_choice", _native.RA_MAT_MAXCHOICE + 1, b"num_choice")
    refused("num_materials", 0, b"num_materials")
    refused("obj_material", None, b"obj_material")
    refused("obj_geomnum", 100000, b"geom range", index=1)
    refused("obj_geomadr", -1, b"geom range", index=0)
    refused("mat_off", int(a.mat_off[3]) + 1, b"mat_off", index=3)
    plain.param_rows.stages = RESTORE | MATERIAL      # MATERIAL without a table
    assert launch(plain.param_rows, plain) != 0 and b"RA_ROWS_MATERIAL needs mat_table" in L.rg_last_error()
    a.stages = RESTORE | MATERIAL | PARK
    assert launch() == 0      # stages up to 7
    assert L.ra_param_rows_args_size() == ctypes.sizeof(_native.RaParamRowsArgs)
    fields = [f[0] for f in _native.RaParamRowsArgs._fields_]
    assert fields.index("stages") < fields.index("mat_table") < fields.index("mat_off") < fields.index("obj_perm") and _native.RA_ROWS_MATERIAL == 4
    _ok(env, e2, plain)


def test_refusals_emul(emul_lib):
    _refusals(emul_lib)


@pytest.mark.gpu
def test_refusals_gpu():
    _refusals(None)
