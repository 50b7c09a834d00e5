"""env-steps/s of rearrange/blocks with per-object materials (`material_names`), bench.bench_rearrange_steady's protocol restated with the constructor keyword: B = 4096,
5 blocks, pipelined device resets, iid U(-1, 1) actions, `--knock` live envs per step have one object put off the table (their episode ends on that step and the full
reset recipe runs inside the following steps), `--warmup` untimed steps (one recipe length) then `--steps` timed ones, one synchronisation at each end.  One JSON line
per case: the default list (the stage is not requested) and the five-name list (the stage runs on the envs whose episode ended, the object-damping phase reads
`object_material` where the objects finished stabilising, five randomizers start from the env's own rows).

    python tools/bench_rearrange_materials.py [--batch 4096] [--steps 30] [--warmup 215] [--knock 4] [--out profiles/<file>.jsonl]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv  # noqa: E402
from robogym_amd.envs.rearrange.materials import MATERIAL_NAMES  # noqa: E402

CASES = [("default", ("default",)), ("five materials", tuple(MATERIAL_NAMES))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=215)
    ap.add_argument("--knock", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, B, lines = torch.device("cuda", 0), args.batch, []
    for name, names in CASES:
        env = BatchedBlockRearrangeEnv(B, device=dev, starting_seed=20200906, pipelined_reset=True, device_reset=True, material_names=names)
        full = (env.stabilize_steps, env.n_random_initial_steps, env.settle_steps)      # (the first reset only places the objects; the recipes inside the steps are the full one)
        env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = 20, 2, 20
        env.reset(on_device=True)
        env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = full
        gen = torch.Generator(device=dev); gen.manual_seed(20200906)
        ended = torch.zeros((), device=dev)

        def step():
            rows = torch.multinomial((env.stage == 0).float() + 1.0e-9, args.knock, generator=gen)      # (live envs, drawn without a readback)
            env.sim.qpos[rows, env.obj_q[0]] = 3.0
            return env.step(torch.rand((B, 6), generator=gen, device=dev) * 2 - 1)

        for _ in range(args.warmup):
            step()
        env.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            ended += step()[2].sum()
        env.sync()
        dt = time.perf_counter() - t0
        rec = {"material_names": name, "B": B, "steps": args.steps, "warmup": args.warmup, "env_steps_per_s": round(B * args.steps / dt), "ms_per_step": round(1e3 * dt / args.steps, 3),
               "episodes_ended_in_window": int(ended), "status": int(env.sim.status.max()) | int(env.solver_sim.status.max()), "placement_failed": int(env.placement_failed.sum())}
        if env.materials_on:
            rec["materials_in_use"] = torch.bincount(env.object_material.reshape(-1), minlength=len(MATERIAL_NAMES)).tolist()
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        del env
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "a") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
