"""What rot_dist_type "icp" costs on rearrange/ycb (B = 4096, N = 8, shipped object set 0, pipelined device resets), and that "full" costs what it did:

    python tools/bench_rearrange_icp.py [--parent TREE] [--out profiles/rearrange_icp.txt]

One worker process per line -- `full` and `icp` of this tree and, with --parent, `full` of a built checkout of the parent commit (its own Python package and library) --
all alive on one GPU; the orchestrator hands out timed windows of at least --window seconds in turn (full, icp, parent, full, ...), so drift of the box hits every line
alike.  A window is env.step calls on random actions between two device synchronisations.  The icp worker also times its ra_env_icp launch alone.
Writes env-steps/s per window and their median per line, the run-to-run spread of the `full` windows, and the ICP launch's own time.
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))


def worker(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import ctypes

    import torch

    from robogym_amd import _native
    from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv

    dev = torch.device("cuda", 0)
    B = args.batch
    kw = {} if args.worker == "full" else {"rot_dist_type": args.worker}
    env = BatchedYcbRearrangeEnv(B, device=dev, starting_seed=20200901 + 5, pipelined_reset=True, device_reset=True, **kw)
    full = (env.stabilize_steps, env.n_random_initial_steps, env.settle_steps)
    env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = 20, 2, 20      # (the first reset only places the objects, as bench.py's steady-state line)
    env.reset()
    env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = full
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    step = lambda: env.step(torch.rand((B, 6), generator=gen, device=dev) * 2 - 1)
    for _ in range(5):
        step()
    torch.cuda.synchronize(dev)
    print(json.dumps({"ready": args.worker}), flush=True)
    for line in sys.stdin:
        cmd = line.strip()
        if cmd == "go":
            n, t0 = 0, time.perf_counter()
            while True:
                for _ in range(5):
                    step()
                n += 5
                torch.cuda.synchronize(dev)
                dt = time.perf_counter() - t0
                if dt >= args.window:
                    break
            print(json.dumps({"steps": n, "seconds": dt, "rate": B * n / dt}), flush=True)
        elif cmd == "icp":
            reps = 20
            env.icp.frozen = env.frozen.data_ptr()      # (the step's codes: the last launch of a step ran on the re-observation codes, which skip nearly every env)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(reps):
                _native.check(env._L, env._L.ra_env_icp(env.sim._bh, ctypes.byref(env.icp), env._stream()), "ra_env_icp")
            torch.cuda.synchronize(dev)
            print(json.dumps({"icp_launch_ms": 1e3 * (time.perf_counter() - t0) / reps, "status_bits": int(env.sim.status.max().item())}), flush=True)
        else:
            break


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, choices=["full", "icp"], help="(internal) run as the worker of this mode")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout the worker imports robogym_amd from")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its `full` line is measured next to this tree's")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--window", type=float, default=2.0, help="seconds per timed window, at least")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rearrange_icp.txt"))
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    lines = [("full", "full", ROOT), ("icp", "icp", ROOT)] + ([("parent full", "full", os.path.abspath(args.parent))] if args.parent else [])
    procs = {}
    for name, mode, tree in lines:      # one after the other: at most three processes hold the GPU
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", mode, "--tree", tree, "--batch", str(args.batch), "--window", str(args.window)],
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=tree)
        ready = p.stdout.readline()
        if not ready:
            raise SystemExit("worker %r did not start (exit code %r)" % (name, p.wait()))
        procs[name] = p

    def ask(name, cmd):
        p = procs[name]
        p.stdin.write(cmd + "\n"); p.stdin.flush()
        out = p.stdout.readline()
        if not out:
            raise SystemExit("worker %r ended (exit code %r)" % (name, p.wait()))
        return json.loads(out)

    rates = {name: [] for name, _, _ in lines}
    try:
        for _ in range(args.rounds):
            for name, _, _ in lines:
                rates[name].append(ask(name, "go")["rate"])
        icp = ask("icp", "icp")
    finally:
        for p in procs.values():
            try:
                p.stdin.write("quit\n"); p.stdin.flush()
            except OSError:
                pass
            p.wait()
    med = lambda v: sorted(v)[len(v) // 2] if len(v) % 2 else 0.5 * (sorted(v)[len(v) // 2 - 1] + sorted(v)[len(v) // 2])
    out = ["rearrange/ycb, B = %d, N = 8, object set 0, pipelined device resets; env-steps/s over interleaved windows of >= %.1f s (%d per line)" % (args.batch, args.window, args.rounds)]
    for name, _, _ in lines:
        out.append("%-12s median %10.0f   windows %s" % (name, med(rates[name]), " ".join("%.0f" % r for r in rates[name])))
    f = rates["full"]
    out.append("full: run-to-run spread of its windows (max - min) / median = %.2f %%" % (100.0 * (max(f) - min(f)) / med(f)))
    if args.parent:
        out.append("full against the parent's full: %+.2f %% (medians)" % (100.0 * (med(f) / med(rates["parent full"]) - 1.0)))
    step_full, step_icp = 1e3 * args.batch / med(f), 1e3 * args.batch / med(rates["icp"])
    out.append("ms per step: full %.2f, icp %.2f (+%.2f, %.1f %% of the icp step); the ra_env_icp launch alone (B x N = %d workgroups): %.2f ms" %
               (step_full, step_icp, step_icp - step_full, 100.0 * (step_icp - step_full) / step_icp, args.batch * 8, icp["icp_launch_ms"]))
    out.append("(an env.step issues the ICP launch in front of each of its env-kernel launches: two per step with device resets)")
    text = "\n".join(out) + "\n"
    print(text, end="")
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
