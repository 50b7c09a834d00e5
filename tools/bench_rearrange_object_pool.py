"""env-steps/s of rearrange/ycb with per-env object subsets (`object_pool`), tools/bench_rearrange_num_objects.py's protocol: `make_env` (wrapper stack, MultiDiscrete
actions) at B = 4096 on ycb set 0 with pipelined device resets, random bin actions, `--warmup` untimed steps then `--steps` timed ones (one synchronisation at each
end).  One JSON line per case: the plain 8-object env, and the pool with n = 8, 4 and 2 of the eight in use -- what the parked mesh objects still cost on
rb_step_kernel, which steps them like any other body.

    python tools/bench_rearrange_object_pool.py [--batch 4096] [--steps 100] [--warmup 20] [--only "plain,pool n=2"] [--out profiles/<file>.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange import ycb  # noqa: E402

CASES = [("plain ycb (8)", None), ("pool n=8 of 8", 8), ("pool n=4 of 8", 4), ("pool n=2 of 8", 2)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the case names to run (default: all)")
    args = ap.parse_args()
    lines = []
    for name, n in CASES:
        if args.only and not any(name.startswith(p) for p in args.only.split(",")):
            continue
        kw = {} if n is None else dict(object_pool=True, parameters={"simulation_params": {"num_objects": n}})
        env = ycb.make_env(batch_size=args.batch, device="cuda:0", pipelined_reset=True, device_reset=True, starting_seed=1, **kw)
        env.reset(on_device=True)
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
        rec = {"env": name, "B": args.batch, "steps": args.steps, "warmup": args.warmup, "env_steps_per_s": round(args.batch * args.steps / dt), "status": status,
               "placement_failed": int(env.placement_failed.sum())}
        if n is not None:
            rec["distinct_object_sets"] = len({tuple(r) for r in env.object_set().tolist()})
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del env
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
