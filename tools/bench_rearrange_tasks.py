"""env-steps/s of the rearrange block tasks next to rearrange/blocks and rearrange/ycb: `make_env` (wrapper stack, MultiDiscrete actions) at B = 4096 with pipelined
device resets, random bin actions, `--warmup` untimed steps then `--steps` timed ones (one synchronisation at each end).  One JSON line per env.

    python tools/bench_rearrange_tasks.py [--batch 4096] [--steps 200] [--warmup 30] [--only "blocks (5),dominos"] [--out profiles/<file>.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange import blocks, blocks_attached, blocks_pickandplace, blocks_reach, blocks_stack, blocks_train, dominos, ycb, ycb_pickandplace  # noqa: E402

CASES = [("blocks (5)", blocks.make_env, {}), ("blocks_pickandplace (5)", blocks_pickandplace.make_env, {"num_objects": 5}),
         ("blocks_stack (5)", blocks_stack.make_env, {"num_objects": 5}), ("blocks_pickandplace (1, default)", blocks_pickandplace.make_env, {}),
         ("blocks_stack (2, default)", blocks_stack.make_env, {}), ("blocks_reach (1, state)", blocks_reach.make_env, {}),
         ("blocks_reach (1, det-state)", blocks_reach.make_env, {"goal_generation": "det-state"}), ("ycb (8)", ycb.make_env, {}),
         ("ycb_pickandplace (8)", ycb_pickandplace.make_env, {}), ("blocks_train (5)", blocks_train.make_env, {}), ("dominos (5, train goal)", dominos.make_env, {}),
         ("dominos (5, holdout: arc goal)", dominos.make_env, {"is_holdout": True}), ("attached (8)", blocks_attached.make_env, {})]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="comma-separated prefixes of the env names to run (default: all)")
    args = ap.parse_args()
    lines = []
    for name, make, opt in CASES:
        if args.only and not any(name.startswith(p) for p in args.only.split(",")):
            continue
        params, consts = {}, {}
        if "num_objects" in opt:
            params = {"simulation_params": {"num_objects": opt["num_objects"]}}
        if "goal_generation" in opt:
            consts = {"goal_generation": opt["goal_generation"]}
        if "is_holdout" in opt:
            consts = {"is_holdout": opt["is_holdout"]}
        env = make(batch_size=args.batch, device="cuda:0", parameters=params, constants=consts, pipelined_reset=True, device_reset=True, starting_seed=1)
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
        status = int(env.sim.status.max()) | (0 if env.solver_sim is None else int(env.solver_sim.status.max()))
        rec = {"env": name, "B": args.batch, "steps": args.steps, "warmup": args.warmup, "env_steps_per_s": round(args.batch * args.steps / dt), "status": status}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del env
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
