"""env-steps/s of rearrange/blocks with per-env object counts (`simulation_params.max_num_objects`), tools/bench_rearrange_tasks.py's protocol: `make_env` (wrapper
stack, MultiDiscrete actions) at B = 4096 with pipelined device resets, random bin actions, `--warmup` untimed steps then `--steps` timed ones (one synchronisation at
each end).  One JSON line per case: the plain 5-block env, M = 5 with every object in use, M = 5 with counts uniform over 1..5, M = 5 with one object per env -- what a
parked object still costs on rb_step_kernel, which steps it like any other body.

    python tools/bench_rearrange_num_objects.py [--batch 4096] [--steps 200] [--warmup 30] [--only "plain,M=5 uniform"] [--out profiles/<file>.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange import blocks  # noqa: E402

CASES = [("plain blocks (5)", None, None), ("M=5 all five in use", 5, "all"), ("M=5 uniform counts 1..5", 5, "uniform"), ("M=5 one object per env", 5, "one")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the case names to run (default: all)")
    args = ap.parse_args()
    lines = []
    for name, M, counts in CASES:
        if args.only and not any(name.startswith(p) for p in args.only.split(",")):
            continue
        sp = {} if M is None else {"num_objects": 1 if counts == "one" else 5, "max_num_objects": M}
        env = blocks.make_env(batch_size=args.batch, device="cuda:0", parameters={"simulation_params": sp}, pipelined_reset=True, device_reset=True, starting_seed=1)
        if counts == "uniform":
            env.set_num_objects_next(1 + torch.arange(args.batch).numpy() % 5)
        env.reset()
        g = torch.Generator(device="cuda:0"); g.manual_seed(0)
        acts = [torch.randint(0, 11, env.action_shape, device="cuda:0", generator=g, dtype=torch.int32) for _ in range(8)]
        for k in range(args.warmup):
            env.step(acts[k % 8])
        env.sync()
        t0 = time.perf_counter()
        for k in range(args.steps):
            env.step(acts[k % 8])
        env.sync()
        dt = time.perf_counter() - t0
        status = int(env.sim.status.max()) | int(env.solver_sim.status.max())
        rec = {"env": name, "B": args.batch, "steps": args.steps, "warmup": args.warmup, "env_steps_per_s": round(args.batch * args.steps / dt), "status": status}
        if M is not None:
            rec["mean_num_active"] = round(float(env.num_active.float().mean()), 3)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
