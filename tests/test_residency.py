"""Residency of the hand stepper's rollout configurations, checked instead of computed by hand: the LDS image in granules and the host's grid arithmetic on the CPU,
registers and resident workgroups per CU from the runtime on the GPU (rg_kernel_resources).  Today: 10 granules of 1280 B and 168 VGPRs = 3 waves per SIMD, 12 envs
per CU (14 per CU at 128 VGPRs and 9 granules was measured and not kept, profiles/four_waves.txt).  And the path that any smaller contact capacity leans on: an
env.step that exceeds the rollout capacities and is handed to the large configuration in the middle, and the reuse of a workgroup's LDS image across work items."""
import ctypes

import numpy as np
import pytest
import torch

from robogym_amd import _native

GRANULE, LDS_GRANULES_PER_CU = 1280, 128     # 160 KiB of LDS per CU, allocated in granules of 1280 B
ROLLOUT_GRANULES, WAVES_PER_SIMD = 10, 3      # what the rollout configurations are built for


def test_rollout_image_granules_and_large_image_bytes(emul_lib):
    assert emul_lib.rg_lds_bytes_cfg(_native.RG_CFG_ROLLOUT) <= ROLLOUT_GRANULES * GRANULE
    assert emul_lib.rg_lds_bytes() == emul_lib.rg_lds_bytes_cfg(_native.RG_CFG_ROLLOUT)
    assert emul_lib.rg_lds_bytes_cfg(_native.RG_CFG_LARGE) == 20480


def test_persistent_grid_per_cu_follows_granules_and_register_budget(emul_lib):
    granules = -(-emul_lib.rg_lds_bytes_cfg(_native.RG_CFG_ROLLOUT) // GRANULE)
    assert emul_lib.rg_items_per_cu() == min(LDS_GRANULES_PER_CU // granules, 4 * WAVES_PER_SIMD) == 12


def _resources(L, config):
    out = (ctypes.c_int * 4)()
    _native.check(L, L.rg_kernel_resources(config, out), "rg_kernel_resources")
    return [int(v) for v in out]


@pytest.mark.gpu
def test_kernel_resources_gpu(locked_model):
    """What the runtime says about the compiled kernels: registers per lane and resident workgroups per CU at the launch's dynamic LDS size."""
    L = _native.lib()
    for name, config in (("rollout", _native.RG_CFG_ROLLOUT), ("items", _native.RG_CFG_ITEMS)):
        regs, static_lds, dyn_lds, blocks = _resources(L, config)
        print("%s: numRegs %d, static LDS %d B, dynamic LDS %d B, %d workgroups per CU" % (name, regs, static_lds, dyn_lds, blocks))
        assert regs <= 512 // WAVES_PER_SIMD // 8 * 8 and static_lds == 0 and dyn_lds == L.rg_lds_bytes_cfg(_native.RG_CFG_ROLLOUT)     # (registers are allocated in eights)
        assert blocks == L.rg_items_per_cu() == 12
    regs, static_lds, dyn_lds, blocks = _resources(L, _native.RG_CFG_LARGE)
    print("large: numRegs %d, static LDS %d B, dynamic LDS %d B, %d workgroups per CU" % (regs, static_lds, dyn_lds, blocks))
    assert dyn_lds == 20480 and blocks == 8
    sim_slots, queues = ctypes.c_int(0), ctypes.c_int(0)
    from robogym_amd.envs.dactyl.locked import LockedSimulation

    probe = LockedSimulation(locked_model, 4, device="cuda:0")
    L.rg_batch_items_info(probe._bh, ctypes.byref(sim_slots), ctypes.byref(queues))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    print("persistent grid: %d workgroups on %d CUs" % (sim_slots.value, cus))
    assert sim_slots.value == cus * L.rg_items_per_cu()


def _overfull_qpos(B):
    """Cube and target pushed under the floor plane (4 box-plane contacts each) and a randomly bent hand with many finger-finger contacts: more contacts
    than the rollout configuration holds (the pose of test_contact_cap_in_plane_pairs_stays_convergent, one draw per env).  Odd envs keep the model's
    start pose, which fits: the launch mixes envs that are handed over with envs that are not."""
    rows = []
    for e in range(B):
        q = np.random.RandomState(5 + e).randn(38) * 0.1
        q[:14] = 0; q[3] = 1; q[10] = 1; q[0:3] = -2; q[7:10] = -2
        rows.append(q)
    return np.asarray(rows, dtype=np.float32)


def _overflow_step(make_sim, B, capacity, items):
    from robogym_amd.mujoco import simulation_interface as si

    before, plane_before = si.SUBSTEP_ITEMS, si.MPR_PLANE_DEPTH
    si.SUBSTEP_ITEMS, si.MPR_PLANE_DEPTH = items, False     # (product default depth: there the two configurations agree to the bit)
    try:
        sim = make_sim()
        q = sim.qpos.clone()
        over = torch.as_tensor(_overfull_qpos(B), device=sim.device)
        q[0::2] = over[0::2]
        sim.view(_native.RG_F_QPOS)[:] = q
        sim.touch_qpos()
        gen = torch.Generator(device=sim.device); gen.manual_seed(11)
        action = torch.rand((B, 20), generator=gen, device=sim.device) * 2 - 1
        obs = torch.zeros((B, sim.obs_dim), device=sim.device)
        goal = torch.zeros((B, 4), device=sim.device); goal[:, 0] = 1
        gd = torch.zeros(B, device=sim.device)
        sim.env_step(action=action, goal_quat=goal, obs=obs, goal_dist=gd, nforward_ticks=3, capacity=capacity)
        sim.sync()
        redone = 0 if sim._redo is None or capacity != "auto" else int((sim._redo != 0).sum())
        rows = [sim.get_field(f).clone() for f in (_native.RG_F_QPOS, _native.RG_F_QVEL, _native.RG_F_CTRL, _native.RG_F_PID, _native.RG_F_WARMSTART, _native.RG_F_TIME)]
        return rows + [obs, gd, sim.status.clone()], redone
    finally:
        si.SUBSTEP_ITEMS, si.MPR_PLANE_DEPTH = before, plane_before


def _check_overflow(make_sim, B):
    got, redone = _overflow_step(make_sim, B, "auto", True)        # items path, the hand-over happens inside the env.step
    ref, _ = _overflow_step(make_sim, B, "large", False)           # the large configuration alone
    print("env.steps handed to the large configuration: %d of %d" % (redone, B))
    assert redone >= 1 and redone < B
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert int((got[-1] & (_native.RG_STATUS_CON_FULL | _native.RG_STATUS_CAND_FULL)).max()) == 0


def test_overflow_at_rollout_capacity_is_handed_over_emul(locked_model, emul_lib):
    from robogym_amd.envs.dactyl.locked import LockedSimulation

    _check_overflow(lambda: LockedSimulation(locked_model, 4, device="cpu", lib=emul_lib, n_substeps=2), 4)


@pytest.mark.gpu
def test_overflow_at_rollout_capacity_is_handed_over_gpu(locked_model):
    from robogym_amd.envs.dactyl.locked import LockedSimulation

    _check_overflow(lambda: LockedSimulation(locked_model, 64, device="cuda:0", n_substeps=2), 64)


@pytest.mark.gpu
def test_lds_overlays_are_safe_across_work_items_gpu(locked_model):
    """One env.step of 10 substeps at B = 256 (more than one persistent workgroup per XCD queue, so a workgroup's LDS image is reused by items of other
    envs): twice through rg_step_items_kernel, once through rg_step_kernel of the rollout configuration.  An array that an overlay clobbers while it is
    still alive shows as a difference between the dispatches or between the runs."""
    from robogym_amd.envs.dactyl.locked import LockedSimulation
    from robogym_amd.mujoco import simulation_interface as si

    B = 256
    before, plane_before = si.SUBSTEP_ITEMS, si.MPR_PLANE_DEPTH
    si.MPR_PLANE_DEPTH = False
    outs = []
    try:
        for items in (True, True, False):
            si.SUBSTEP_ITEMS = items
            sim = LockedSimulation(locked_model, B, device="cuda:0", n_substeps=10)
            gen = torch.Generator(device="cuda:0"); gen.manual_seed(23)
            hand = sim.get_qpos("hand_angle")
            sim.set_qpos("hand_angle", hand + 0.05 * torch.randn(hand.shape, generator=gen, device="cuda:0"))
            action = torch.rand((B, 20), generator=gen, device="cuda:0") * 2 - 1
            obs = torch.zeros((B, sim.obs_dim), device="cuda:0")
            sim.env_step(action=action, obs=obs, nforward_ticks=3)
            sim.sync()
            outs.append([sim.get_field(f).clone() for f in (_native.RG_F_QPOS, _native.RG_F_QVEL, _native.RG_F_CTRL, _native.RG_F_PID, _native.RG_F_WARMSTART,
                                                            _native.RG_F_STATS)] + [obs, sim.status.clone()])
    finally:
        si.SUBSTEP_ITEMS, si.MPR_PLANE_DEPTH = before, plane_before
    for a, b, c in zip(*outs):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert int(outs[0][-1].max()) == 0 and float(outs[0][5][:, 3].min()) == 10.0
