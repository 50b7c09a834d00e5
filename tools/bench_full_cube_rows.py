"""dactyl/full_perpendicular env-steps/s with the per-env parameter rows ON and every new row randomised (timestep in [0.75, 1.2] x nominal, cube scale in
[0.95, 1.05], a random wrench on the cube of half the envs: the rows of tests/test_large_env_params.py::test_full_cube_randomised_rows_full_batch_gpu), next to the
same batch with rows ON and untouched.  No bar: the cost the randomization wrappers inherit.
    python tools/bench_full_cube_rows.py [batch] [steps] [warmup]"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from robogym_amd.envs.dactyl.full_perpendicular import BatchedFullPerpendicularEnv  # noqa: E402

B, steps, warmup = (int(sys.argv[k]) if len(sys.argv) > k else d for k, d in ((1, 4096), (2, 20), (3, 5)))
for randomise in (False, True):
    env = BatchedFullPerpendicularEnv(B, device="cuda:0", starting_seed=7, per_env_parameters=True)
    env.reset()
    sim = env.mujoco_simulation
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(5)
    if randomise:
        P = sim.params
        P["timestep"].mul_(0.75 + 0.45 * torch.rand(B, 1, generator=gen, device="cuda:0"))
        sim.set_cube_size_multiplier(0.95 + 0.1 * torch.rand(B, generator=gen, device="cuda:0"))
        w = torch.randn(B, 6, generator=gen, device="cuda:0") * torch.tensor([0.5, 0.5, 0.5, 0.005, 0.005, 0.005], device="cuda:0")
        w[B // 2:] = 0
        P["xfrc_applied"][:, env.model.name2id("body", "cube:middle")] = w
    for k in range(warmup + steps):
        if k == warmup:
            torch.cuda.synchronize(); t0 = time.perf_counter()
        env.step(torch.rand(B, env.num_actions, generator=gen, device="cuda:0") * 2 - 1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print("full cube, batch %d, rows ON, %s: %.0f env-steps/s (%.2f ms per step, status bits %d)" % (
        B, "every new row randomised" if randomise else "no row touched", B * steps / dt, 1e3 * dt / steps, int(sim.status.max())), flush=True)
