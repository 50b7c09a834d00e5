"""Wall time of the synchronous `reset(mask)` of the rearrange envs, the device recipe against the host recipe: B = 4096, default recipe lengths (100 stabilising
steps, 10 of a random action, 100 settling), the 5-block world and one ycb object set; masks of 1, 64 and 4096 envs spread over the batch (env 0 and env B - 1 among
them from two envs on).  Each figure: one untimed call, then `--repeats` timed ones, each bracketed by `sync()`; median, minimum and maximum.

On a tree whose `reset` has the `on_device` keyword the env is built with `device_reset=True` and two kinds are timed on it: `kind=device` (`on_device=True`) and
`kind=host` (`on_device=False`).  On a tree without the keyword the tool times plain `reset(mask)` and calls it `kind=parent host` -- run it there to get the line the
host figures of this tree are compared with.

    python tools/bench_rearrange_sync_reset.py [--batch 4096] [--sizes 1,64,4096] [--repeats 5] [--envs blocks,ycb] [--out profiles/<file>.txt]
"""
import argparse
import inspect
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv  # noqa: E402
from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv  # noqa: E402

ENVS = {"blocks": BatchedBlockRearrangeEnv, "ycb": BatchedYcbRearrangeEnv}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--sizes", default="1,64,4096")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--envs", default="blocks,ycb")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    B = args.batch
    lines = []
    for name in args.envs.split(","):
        cls = ENVS[name]
        has_keyword = "on_device" in inspect.signature(cls.reset).parameters
        env = cls(B, device="cuda:0", starting_seed=1, **(dict(device_reset=True) if has_keyword else {}))
        env.reset(**(dict(on_device=False) if has_keyword else {}))
        kinds = [("device", dict(on_device=True)), ("host", dict(on_device=False))] if has_keyword else [("parent host", {})]
        for size in (min(int(s), B) for s in args.sizes.split(",")):
            rows = torch.linspace(0, B - 1, size).round().long() if size > 1 else torch.zeros(1, dtype=torch.long)
            mask = torch.zeros(B, dtype=torch.bool, device="cuda:0")
            mask[rows.to("cuda:0")] = True
            assert int(mask.sum()) == size
            for kind, kw in kinds:
                times = []
                for k in range(args.repeats + 1):
                    env.sync()
                    t0 = time.perf_counter()
                    env.reset(mask=mask, **kw)
                    env.sync()
                    times.append(1000.0 * (time.perf_counter() - t0))
                times = times[1:]      # (the first call is untimed)
                status = int(env.sim.status.max()) | int(env.solver_sim.status.max())
                line = "kind=%-11s env=%-6s B=%d mask=%-4d median_ms=%9.1f min_ms=%9.1f max_ms=%9.1f runs_ms=[%s] status=%d" % (
                    kind, name, B, size, statistics.median(times), min(times), max(times), ", ".join("%.1f" % t for t in times), status)
                print(line, flush=True)
                lines.append(line)
        del env
    if args.out:
        with open(args.out, "a") as f:
            for line in lines:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
