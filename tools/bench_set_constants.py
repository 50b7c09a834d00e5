"""Time of `set_constants()` (rb_setconst_kernel: mj_setConst on the device, every env of the batch) on the large-model stepper, next to one `env_step` of the
same batch: the full cube (large configuration), rearrange/blocks with 5 objects and the TCP solver world (one-wave configurations).  Every env carries its own
randomised body_mass / body_inertia / dof_armature rows.  HIP events around each call, warm-up first, median and spread over the repeats.  No bar is fixed: the
yardstick is the only alternative before this kernel, robogym_amd/mujoco/setconst.py on the host, seconds per distinct row for the full cube.
    python tools/bench_set_constants.py [batch] [repeats] [warmup] > profiles/setconst_large.txt"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robogym_amd.envs.dactyl.full_perpendicular import FullPerpendicularSimulation, load_full_perpendicular_model  # noqa: E402
from robogym_amd.envs.rearrange.xml import load_blocks_model, load_solver_model  # noqa: E402
from robogym_amd.mujoco.large_simulation import LargeModelSimulation  # noqa: E402

B, repeats, warmup = (int(sys.argv[k]) if len(sys.argv) > k else d for k, d in ((1, 4096), (2, 20), (3, 3)))
assert repeats >= 20, "at least 20 repeats"
dev = "cuda:0"


def timed(fn):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms = np.array(ms)
    return float(np.median(ms)), float(ms.min()), float(ms.max())


def randomise(sim, gen):
    P = sim.params
    for k in ("body_mass", "body_inertia", "dof_armature"):
        shape = P[k].shape[:2] + (1,) * (P[k].dim() - 2)
        P[k].mul_(0.7 + 0.6 * torch.rand(shape, generator=gen, device=dev))


print("set_constants() against env_step, batch %d, %d repeats after %d warm-up calls, HIP events; ms: median (min .. max)" % (B, repeats, warmup), flush=True)
gen = torch.Generator(device=dev); gen.manual_seed(3)
for name, make in (("full cube (nv 168, 256 threads per env)", lambda: FullPerpendicularSimulation(load_full_perpendicular_model(), B, device=dev, env_params=True)),
                   ("rearrange/blocks5 main world", lambda: LargeModelSimulation(load_blocks_model(5), B, device=dev, hand=False, n_substeps=40, env_params=True)),
                   ("TCP solver world", lambda: LargeModelSimulation(load_solver_model(), B, device=dev, hand=False, n_substeps=40, env_params=True))):
    sim = make()
    randomise(sim, gen)
    sc = timed(sim.set_constants)
    finite = all(bool(torch.isfinite(sim.params[k]).all()) for k in ("dof_invweight0", "body_invweight0", "tendon_invweight0"))
    st = timed(lambda: sim.env_step(nforward_ticks=1))
    print("%-42s threads %3d  nv %3d  set_constants %9.3f (%9.3f .. %9.3f)   env_step of %2d substeps %9.3f (%9.3f .. %9.3f)   ratio %.2f   status bits %d, outputs finite %s" % (
        name, sim.info["threads"], sim.nv, sc[0], sc[1], sc[2], sim.n_substeps, st[0], st[1], st[2], sc[0] / st[0], int(sim.status.max()), finite), flush=True)
    del sim
