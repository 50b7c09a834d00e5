"""The headline rollout of bench.py (dactyl/locked, B = 8192, same seeds and actions) carried on over a long window, with what bench.py does not report:
the env.steps handed from the rollout to the large kernel configuration, and -- on an analysis build (-DRG_CAP_HIST) -- the histograms of contacts and
Jacobian pool words per substep.  RGSTEP_LIB selects the build.
usage: python tools/capacity_rollout.py [--pipelined-reset] [--warmup W] [--steps K] [--long-steps N]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from robogym_amd import _native
from robogym_amd.envs.dactyl.locked import make_simple_env

ap = argparse.ArgumentParser()
ap.add_argument("--pipelined-reset", action="store_true")
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--long-steps", type=int, default=300)
ap.add_argument("--batch", type=int, default=8192)
args = ap.parse_args()
B, dev = args.batch, torch.device("cuda", 0)
torch.cuda.set_device(0)
env = make_simple_env(batch_size=B, device=dev, starting_seed=20200901 + 1, pipelined_reset=args.pipelined_reset, sort_dispatch=True)
env.reset()
sim = env.mujoco_simulation
gen = torch.Generator(device=dev); gen.manual_seed(20200901 + 1)
handed = torch.zeros((), dtype=torch.int64, device=dev)


def window(n):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(n):
        env.step(torch.rand((B, 20), generator=gen, device=dev) * 2 - 1)
        if sim._redo is not None:
            handed.add_((sim._redo != 0).sum())
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0


window(args.warmup)
handed.zero_()
out = {"lib": os.path.basename(_native.LIB_PATH), "pipelined_reset": args.pipelined_reset, "lds_bytes": sim._L.rg_lds_bytes(), "per_cu": sim._L.rg_items_per_cu() if hasattr(sim._L, "rg_items_per_cu") else None}
for name, n in (("short", args.steps), ("long", args.long_steps)):
    if n <= 0:
        continue
    h0 = int(handed)
    t = window(n)
    out[name] = {"steps": n, "env_steps_per_s": round(B * n / t), "handed_over": int(handed) - h0, "of": B * n}
out["status_bits"] = int(sim.status.max().item())
print(json.dumps(out))
if hasattr(sim._L, "rg_cap_hist_read"):
    for cfg, cname in ((2, "substep-granular"), (0, "rollout, one workgroup per env.step"), (1, "large")):
        h = (ctypes.c_uint * 192)()
        assert sim._L.rg_cap_hist_read(cfg, h) == 0
        con, pool = list(h[:64]), list(h[64:])
        n = sum(con)
        if n == 0:
            continue
        print("capacity histogram, %s configuration: %d substeps (reset recipe and warm-up included)" % (cname, n))
        print("  contacts: " + " ".join("%d:%d" % (i, v) for i, v in enumerate(con) if v))
        print("  pool words (bins of 16, lower edge): " + " ".join("%d:%d" % (16 * i, v) for i, v in enumerate(pool) if v))
        tail = lambda xs, k: sum(xs[k:]) / n
        print("  P(contacts > k): " + " ".join("%d:%.2e" % (k, tail(con, k + 1)) for k in (8, 10, 12, 14, 16, 18, 20, 23)))
        print("  P(pool words >= w): " + " ".join("%d:%.2e" % (w, tail(pool, w // 16)) for w in (384, 448, 512, 528, 544, 576, 608, 640, 704, 768)))
