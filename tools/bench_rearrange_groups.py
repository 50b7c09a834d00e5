"""Cost of the greedy group matching inside ra_post_step_kernel: env-steps/s of rearrange/blocks (5 blocks) with `object_groups` "distinct" (no group rows: the
kernel's path without matching), "single" (one group of five: five rounds over 25 pairs) and "sample", same seed, same actions; a shortened reset recipe, `--warmup`
untimed steps then `--steps` timed ones (one synchronisation at each end).  One JSON line per mode.  Under `rocprofv3 --kernel-trace --stats` the kernel's own
time per launch can be read off per mode with `--modes`.

    python tools/bench_rearrange_groups.py [--batch 4096] [--steps 40] [--warmup 5] [--modes distinct,single,sample]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange import blocks  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--modes", default="distinct,single,sample")
    args = ap.parse_args()
    for mode in args.modes.split(","):
        env = blocks.make_simple_env(batch_size=args.batch, device="cuda:0", parameters={"simulation_params": {"object_groups": mode}}, stabilize_steps=20,
                                     n_random_initial_steps=2, settle_steps=20, starting_seed=1)
        env.reset()
        g = torch.Generator(device="cuda:0"); g.manual_seed(0)
        acts = [torch.rand(env.action_shape, device="cuda:0", generator=g) * 2 - 1 for _ in range(args.warmup + args.steps)]
        for a in acts[:args.warmup]:
            env.step(a)
        env.sync()
        t0 = time.perf_counter()
        for a in acts[args.warmup:]:
            env.step(a)
        env.sync()
        dt = time.perf_counter() - t0
        print(json.dumps({"object_groups": mode, "batch": args.batch, "steps": args.steps, "env_steps_per_s": round(args.batch * args.steps / dt, 1),
                          "ms_per_step": round(1e3 * dt / args.steps, 3), "status_bits": int(env.sim.status.max())}), flush=True)
        del env


if __name__ == "__main__":
    main()
