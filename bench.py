"""bench.py — env-steps/sec of the dactyl/locked env.step hot path on MI355X (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W          (single GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
    python bench.py --gpus N ...                           (no launcher: re-executes itself under torch.distributed.run with N ranks)

Workload: BASELINE.json configs[1] — dactyl/locked (Shadow hand + locked cube, nv=36), batch 8192 per
GPU (weak scaling), synthetic iid U(-1,1)^20 relative actions, 1 env-step = action map + 10 mj_step
substeps (dt 0.008) + the 3 state-less forward ticks + observation row + goal distance + reward /
tracker logic.  State is resident in HBM when the timed region starts (after `env.reset()`).
One JSON line on stdout (rank 0).  With N>1 every step starts the RCCL all-gather of its observation
rows over xGMI (the only exchange the path has); it overlaps with the next step and is awaited before the
following one is started, the last one inside the timed region.

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds everything else the line can
carry: the CPU baseline, the >= 2 s continuation of the headline rollout and the shortened runs of every other built
config under "secondary".  `--dump-outputs DIR` writes what the last timed env.step returned (observation dict,
reward, done, info) as DIR/<name>.npy in float32; the inputs are seeded, so two builds can be compared array by array.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md


def algorithmic_bytes_per_env_step(m, ncon, nefc, iters, nsub, obs_dim):
    """SURVEY.md §8(d) byte model: every stage-boundary array written once and read once, solver arrays
    read once per iteration, fp32."""
    d = m.dims
    nq, nv, nu, nb, nj, ng, ns, nt = (int(d[i]) for i in (0, 1, 2, 3, 4, 5, 6, 7))
    nM = int(m.k_dims[2]) if "k_dims" in m.arrays else 149
    nM = nM or 149
    S = 5 * nu
    staged = (2 * (nq + 2 * nv + S + nu) + 2 * (28 * nb + 12 * ng + 12 * ns + 6 * nj) + 2 * (13 * nb + 6 * nv)
              + 2 * (nt + nt * nv + nu + nu * nv) + 2 * (10 * nb + 2 * nM + nv) + 2 * 29 * ncon + 2 * (nefc * nv + 8 * nefc)
              + 2 * (6 * nb + 6 * nv + 3 * nv + nu + nefc + 2 * nv))
    solver = iters * (nefc * nv + 2 * nv * nv + 2 * nefc + 5 * nv)
    b_sub = 4.0 * (staged + solver)
    return nsub * b_sub + 4.0 * (nu + obs_dim), b_sub


def cpu_baseline(seconds=3.0):
    """The CPU oracle (double-precision C restatement, -O3 -march=native) stepping the same env, one env per C thread:
    1-thread rate, a ladder of thread counts up to the host's affinity, the best aggregate; kind 'port'.
    Also the oracle's own mean Newton iterations on the bench's action distribution.  oracle/cpu_baseline.py."""
    from oracle import cpu_baseline as cb

    out = cb.run(seconds)
    out["oracle_counters"] = cb.oracle_newton_iterations()
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(path, step_result, limit=DUMP_LIMIT_BYTES):
    """`--dump-outputs`: the (obs, reward, done, info) of one env.step as <path>/<name>.npy, float32, nested dict keys joined
    with '_' (obs_qpos, info_goal_dist_cube_quat, ...).  Past `limit` bytes in all, the same fixed, seeded subset of env rows
    is kept in every array."""
    flat = {}

    def walk(name, v):
        if isinstance(v, dict):
            for k, x in v.items():
                walk(name + "_" + k, x)
        elif torch.is_tensor(v):
            flat[name] = v.detach().to(torch.float32).cpu().numpy()

    for name, v in zip(("obs", "reward", "done", "info"), step_result):
        walk(name, v)
    total = sum(a.nbytes for a in flat.values())
    if total > limit:
        B = max(a.shape[0] for a in flat.values() if a.ndim)
        rows = np.sort(np.random.RandomState(0).choice(B, max(1, int(B * limit / total)), replace=False))
        flat = {k: (a[rows] if a.ndim and a.shape[0] == B else a) for k, a in flat.items()}
    os.makedirs(path, exist_ok=True)
    for k, a in flat.items():
        np.save(os.path.join(path, k + ".npy"), a)


def relaunch_with_ranks(n):
    """`python bench.py --gpus N` without a launcher (WORLD_SIZE unset): start N ranks of this very command under
    torch.distributed.run (one process per GPU, rendezvous on 127.0.0.1) and return its exit code."""
    import socket
    import subprocess

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd)


RG_KERNEL_SOURCES = ("rg_kernel.h", "rg_env_kernel.h", "rg_api.hip", "rg_types.h", "Makefile")                       # what rg_step_items_kernel / rg_step_kernel compile from
RB_KERNEL_SOURCES = RG_KERNEL_SOURCES + ("rb_kernel.h", "rb_env_kernel.h", "ra_env_kernel.h", "rb_types.h")           # rb_step_kernel shares the narrow-phase code of rg_kernel.h


def parity_measured():
    """The parity figures of profiles/parity.json (tests/tools/parity_json.py) if they were measured on THIS kernel build; else None -- never literals."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "parity.json")))
        if t.get("kernel_source_hash") != kernel_source_hash("rg"):
            return None
        return {k: v for k, v in t.items() if k.startswith("resync_") or k.startswith("free_running_") or k in ("round", "protocol")}
    except Exception:
        return None


def kernel_source_hash(which="rg"):
    """Identifies the kernel build a committed PMC figure belongs to (profiles/hbm_traffic.json carries one stamp for the hand's stepper, "rg", and one for the
    general stepper, "rb": an edit of rb_kernel.h leaves the rg kernels' machine code as it was -- tools/kernel_isa_hash.py shows that per kernel)."""
    import hashlib

    h = hashlib.sha256()
    for f in sorted(RG_KERNEL_SOURCES if which == "rg" else RB_KERNEL_SOURCES):
        h.update(f.encode()); h.update(open(os.path.join(ROOT, "robogym_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def rb_traffic_note(workload, B):
    """Why `traffic` is null, with the last measured figure, or where the figure comes from."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
        e = t["rb_step_kernel"][workload]
        gb = float(e["bytes_per_launch"]) / 1e9
        if rb_traffic(workload, B) is not None:
            return "PMC FETCH_SIZE x2 + WRITE_SIZE of the dominant launch, profiles/hbm_traffic.json (round %s)" % t.get("round")
        return "null: the committed figure (%.1f GB per launch at batch %d, round %s) was measured on another build of rb_step_kernel or batch size" % (gb, int(e["batch_per_gpu"]), t.get("round"))
    except (OSError, ValueError, KeyError):
        return "null: no PMC figure committed for this workload"


def rb_traffic(workload, B):
    """HBM GB per dominant rb_step_kernel launch from the round's PMC passes (profiles/hbm_traffic.json), if measured on this kernel build and batch; else None."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
        e = t.get("rb_step_kernel", {}).get(workload)
        if e and int(e["batch_per_gpu"]) == B and t.get("rb_source_hash") == kernel_source_hash("rb"):
            return float(e["bytes_per_launch"]) / 1e9
    except (OSError, ValueError, KeyError):
        pass
    return None


def algorithmic_bytes_sparse(m, nM, ncon, nefc, iters, nsub, obs_dim, jw=16):
    """The same stage-boundary model with the constraint Jacobian counted as it is stored by the large-model stepper: at most `jw` dofs per row
    (a contact touches two dof chains) instead of dense nefc x nv, and the solver's per-iteration traffic likewise (J once, the tree-sparse M
    instead of 2 nv^2).  Reported NEXT TO the SURVEY 8(d) dense figure for models with nv >> a row's support."""
    d = m.dims
    nq, nv, nu, nb, nj, ng, ns, nt = (int(d[i]) for i in (0, 1, 2, 3, 4, 5, 6, 7))
    S = 5 * nu
    w = min(jw, nv)
    staged = (2 * (nq + 2 * nv + S + nu) + 2 * (28 * nb + 12 * ng + 12 * ns + 6 * nj) + 2 * (13 * nb + 6 * nv) + 2 * (nt + nt * w + nu + nu * w)
              + 2 * (10 * nb + 2 * nM + nv) + 2 * 29 * ncon + 2 * (nefc * w + 8 * nefc) + 2 * (6 * nb + 6 * nv + 3 * nv + nu + nefc + 2 * nv))
    solver = iters * (nefc * w + 2 * nM + 2 * nefc + 5 * nv)
    b_sub = 4.0 * (staged + solver)
    return nsub * b_sub + 4.0 * (nu + obs_dim), b_sub


def bench_rearrange_blocks(args, emit=True, ycb=False, joint=False):
    """BASELINE.json configs[3]: rearrange/blocks, num_objects = 5 (UR16e + 2f-85 gripper, table contacts), batch 4096 on one MI355X; with `ycb`
    configs[4]: rearrange/ycb, num_objects = 8 (mesh objects), batch 4096 PER GPU (32768 on 8).
    `BatchedBlockRearrangeEnv.step` = rb_batch_step_tcp (TCP solver world: sync, forward, mocap target, 40 mj_step) + rb_batch_step_ex (main world:
    40 mj_step + 2 forwards, the last in full with sensors) + ra_env_post_step (observation row, reward, goals, tracker), after the reference's reset
    recipe (grid placement, 100 stabilisation steps, 10 random + 100 zero-action steps).  1 env-step = 80 mj_step of two models.
    N > 1 (`--gpus N`, one rank per GPU): the envs are sharded, every rank steps its own 4096, the packed observation rows (obs + reward + done) are
    all-gathered over RCCL behind the next step -- the path's only exchange, as for dactyl/locked.
    `joint`: robot_control_params.control_mode = "joint" (robot_interface.py:9-20): [B, 7] actions, no TCP solver world, two launches per step."""
    from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv
    from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_with_ranks(args.gpus))
    rank, local_rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("LOCAL_RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if emit and world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d ranks (WORLD_SIZE)" % (args.gpus, world))
    distributed = emit and (world > 1 or os.environ.get("RG_BENCH_FORCE_DIST") == "1")
    emul_path = os.environ.get("RG_BENCH_EMUL_LIB")      # TEST HOOK (tests/test_distributed.py): this code path on CPU, 2 ranks, gloo, kernel source on the emulation harness
    lib = None
    if emul_path:
        from robogym_amd import _native
        lib = _native.bind(emul_path)
        dev = torch.device("cpu")
    else:
        dev = torch.device("cuda", local_rank if emit else 0)
        torch.cuda.set_device(dev)
    if distributed:
        import torch.distributed as dist

        dist.init_process_group("gloo") if emul_path else dist.init_process_group("nccl", device_id=dev)
    B = args.batch if args.batch != 8192 else 4096
    quick = bool(getattr(args, "quick_reset", False))
    kw = dict(stabilize_steps=20, n_random_initial_steps=2, settle_steps=20) if quick else {}
    if emul_path:
        kw = dict(stabilize_steps=1, n_random_initial_steps=1, settle_steps=1, n_substeps=1, lib=lib)
    if getattr(args, "no_per_env_params", False):   # (A/B: the model's shared arrays instead of every env's own parameter block)
        kw["per_env_parameters"] = False
    if joint:
        kw["control_mode"] = "joint"
    env = (BatchedYcbRearrangeEnv if ycb else BatchedBlockRearrangeEnv)(B, device=dev, starting_seed=20200901 + 3 + rank, **kw)
    sync = (lambda: torch.cuda.synchronize(dev)) if not emul_path else (lambda: None)
    t_reset = time.perf_counter()
    env.reset()
    sync()
    t_reset = time.perf_counter() - t_reset
    gen = torch.Generator(device=dev); gen.manual_seed(20200901 + 3 + 1000 * rank)
    from robogym_amd.distributed import ShardedObservationGather

    gather = ShardedObservationGather(B, env.packed.shape[1], dev)

    def step():
        r = env.step(torch.rand((B, env.action_dim), generator=gen, device=dev) * 2 - 1)
        gather.start(env.packed)      # the packed row: observation + reward (3) + done
        return r

    for _ in range(args.warmup):
        step()
    env.sim.stats.zero_()
    if env.solver_sim is not None:
        env.solver_sim.stats.zero_()
    mk_event = (lambda: torch.cuda.Event(enable_timing=True)) if not emul_path else (lambda: None)
    ev = [[mk_event() for _ in range(3)] for _ in range(args.steps)]
    orig = env._physics

    def timed(actions, active=None, wrapped=False, solver_active=None, phase=None, _i=[0]):
        e = ev[_i[0] % len(ev)]; _i[0] += 1
        rec = lambda x: x.record() if x is not None else None
        if joint:
            rec(e[0]); rec(e[1]); env._keep_act = env._joint_action(actions, wrapped)
            env.sim.env_step(action=env._keep_act, nforward_ticks=2, flags=32, active=active); rec(e[2])
            return
        rec(e[0]); env.solver_sim.step_tcp(env.sim, actions, env.tcp, active=active); rec(e[1])
        env.sim.env_step(nforward_ticks=2, flags=32, active=active); rec(e[2])
    env._physics = timed
    if distributed:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = step()
    gather.finish()
    if distributed:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    env._physics = orig
    if emit and rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, last)
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if emul_path:
        ms_solver = ms_main = 0.5e3 * elapsed / args.steps
    else:
        ms_solver = float(np.mean([e[0].elapsed_time(e[1]) for e in ev])); ms_main = float(np.mean([e[1].elapsed_time(e[2]) for e in ev]))
    res = {}
    total_bytes = 0.0
    for name, sim, obs_dim in [("main", env.sim, env.obs_dim)] + ([] if env.solver_sim is None else [("solver", env.solver_sim, 0)]):
        st = sim.stats.sum(0).cpu().numpy(); n = max(st[3], 1.0)
        ncon, nefc, iters = float(st[0] / n), float(st[1] / n), float(st[2] / n)

        class _M:
            dims = sim.model.dims
            arrays = {"k_dims": None}
            k_dims = [0, 0, sim.info["nM"]]
        bd, _ = algorithmic_bytes_per_env_step(_M, ncon, nefc, iters, sim.n_substeps, obs_dim)
        bs, _ = algorithmic_bytes_sparse(_M, sim.info["nM"], ncon, nefc, iters, sim.n_substeps, obs_dim)
        res[name] = dict(mean_ncon=ncon, mean_nefc=nefc, mean_newton_iters=iters, algorithmic_bytes_dense=bd, algorithmic_bytes_sparse_J=bs)
        total_bytes += bd
    achieved = B * res["main"]["algorithmic_bytes_dense"] / (ms_main * 1e-3)
    out = {
        "metric": ("env-steps/sec (whole node) rearrange/ycb num_objects=8 batch 4096 per GPU (BASELINE.json configs[4]: 32768 on 8 GPUs); FIXED object set per model, "
                   "unwrapped env.step incl. the TCP solver's second simulation; parity vs the in-repo CPU oracle (physics unpinned vs MuJoCo; the controller chain holds the reference's own rearrange tests at their tolerances)") if ycb else
                  "env-steps/sec rearrange/blocks num_objects=5 batch 4096 (BASELINE.json configs[3]); unwrapped env.step incl. the TCP solver's second simulation; parity vs the in-repo CPU oracle (physics unpinned vs MuJoCo; the controller chain holds the reference's own rearrange tests at their tolerances)",
        "value": world * B * args.steps / elapsed, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": ("rearrange/ycb (UR16e + 2f-85 gripper + table, 8 YCB objects %s as convex-part mesh geoms: nv=56, %d geoms, elliptic cones, impratio 10)" % (getattr(env, "object_names", []), env.sim.info["ngeom"]) if ycb else "rearrange/blocks (UR16e + 2f-85 gripper + table, 5 blocks: nv=38, elliptic cones, impratio 10)") + " with its TCP solver world (nv=8, mocap weld), batch %d, iid U(-1,1) relative tcp+roll+yaw actions, 40 + 40 substeps x 0.001 s + 2 forwards; after the reset recipe%s" % (B, " (shortened: --quick-reset)" if quick else ""),
                   "batch_per_gpu": B, "global_batch": world * B, "parallelism": "dp%d (envs sharded, all-gather of the packed observation rows)" % world, "collective_backend": (dist.get_backend() if distributed else None), "reset_seconds": t_reset, "main": res["main"], "solver": res.get("solver"), "status_bits": int(max(env.sim.status.max().item(), 0 if env.solver_sim is None else env.solver_sim.status.max().item())),
                   "done_fraction_last_step": float(env.done.float().mean().item()), "launch_ms": {"solver_world": ms_solver, "main_world": ms_main}, "lds_bytes_per_workgroup": env.sim.info["lds_bytes"], "per_env_parameters": bool(env.per_env_parameters)},
        "roofline": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": achieved / HBM_PEAK, "traffic": rb_traffic("ycb" if ycb else "rearrange_blocks", B), "traffic_unit": "GB per launch (PMC, profiles/hbm_traffic.json)", "traffic_note": rb_traffic_note("ycb" if ycb else "rearrange_blocks", B), "kernel": "rb_step_kernel (main world launch)", "kernel_ms": ms_main,
                     "algorithmic_bytes_per_env_step": res["main"]["algorithmic_bytes_dense"], "frac_sparse_J": B * res["main"]["algorithmic_bytes_sparse_J"] / (ms_main * 1e-3) / HBM_PEAK,
                     "note": "dominant kernel = the main world's launch; SURVEY 8(d) dense byte model with the run's ncon / nefc / iterations; frac_sparse_J counts a constraint row at <= 16 dofs and M tree-sparse (what the stepper stores)"},
    }
    if args.full and not args.no_cpu_baseline and world == 1 and not emul_path:
        from oracle import cpu_baseline as cb

        out["cpu_baseline"] = cb.run_rearrange_blocks(4.0, ycb=ycb, joint=joint)
    if joint:
        out["metric"] = out["metric"].replace("unwrapped env.step incl. the TCP solver's second simulation", "control_mode joint (7 action numbers, no TCP solver world): unwrapped env.step = the main world's launch + the env kernel")
        out["config"]["control_mode"] = "joint"
        out["config"]["workload"] = out["config"]["workload"].replace(" with its TCP solver world (nv=8, mocap weld)", ", control_mode joint: no TCP solver world").replace(
            "relative tcp+roll+yaw actions, 40 + 40 substeps", "relative joint actions (7 numbers), 40 substeps")
    if emit and rank == 0:
        print(json.dumps(out, default=float))
    if distributed:
        dist.destroy_process_group()
    del env
    if not emul_path:
        torch.cuda.empty_cache()
    return out


def bench_rearrange_steady(args, ycb=False, knock_per_step=4, warm_steps=215, device_reset=True):
    """The rearrange envs WITH episode ends, as driver evidence: `pipelined_reset=True`, the reference's full reset recipe (100 stabilisation
    steps, 10 of one random action, 100 of the zero action) running inside the step calls.  Random actions almost never reach a goal, so episodes of this workload
    end by the goal time-out (200 steps per object) or by an object leaving the table; to see the steady-state MIX inside a short run, `knock_per_step` live envs per
    step have one object put off the table (their episode ends on that step: done, penalty, recipe starts) during `warm_steps` >= one recipe length, so that at the
    timed window ~ knock_per_step x 210 / B of the envs are spread over all stages of the recipe -- the share a 1000-step time-out gives (210 / 1210 = 17 %).
    `device_reset` (default): the recipe's stage machine and the placement / goal sampling in ra_recipe_kernel, no readback inside a step call -- the knocked envs are
    drawn on the device too and the counters are read after the window; False: the host recipe behind one readback of the flags per step."""
    from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv
    from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.batch if args.batch != 8192 else 4096
    env = (BatchedYcbRearrangeEnv if ycb else BatchedBlockRearrangeEnv)(B, device=dev, starting_seed=20200901 + 5, pipelined_reset=True, device_reset=bool(device_reset))
    # (the FIRST reset is shortened -- it only places the objects; every recipe that runs inside the steps is the full one)
    full = (env.stabilize_steps, env.n_random_initial_steps, env.settle_steps)
    env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = 20, 2, 20
    env.reset()
    env.stabilize_steps, env.n_random_initial_steps, env.settle_steps = full
    gen = torch.Generator(device=dev); gen.manual_seed(20200901 + 5)
    rng = np.random.RandomState(20200901 + 5)
    ended = started = 0
    inside = 0.0
    if device_reset:
        ended, started, inside = torch.zeros((), device=dev), torch.zeros((), device=dev), torch.zeros((), device=dev)

    def step(knock):
        nonlocal ended, started, inside
        if knock and device_reset:
            rows = torch.multinomial((env.stage == 0).float() + 1.0e-9, knock, generator=gen)      # (live envs, drawn without a readback)
            env.sim.qpos[rows, env.obj_q[0]] = 3.0
        elif knock:
            live = np.nonzero(env._stage == 0)[0]
            rows = torch.as_tensor(rng.choice(live, size=min(knock, len(live)), replace=False), device=dev, dtype=torch.long)
            env.sim.qpos[rows, env.obj_q[0]] = 3.0          # object 0 far off the table: check_objects_off_table ends the episode on this step
        obs, reward, done, info = env.step(torch.rand((B, 6), generator=gen, device=dev) * 2 - 1)
        return done, info

    for _ in range(warm_steps):
        step(knock_per_step)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        done, info = step(knock_per_step)
        if device_reset:
            ended += done.sum(); started += info["episode_started"].sum(); inside += info["resetting"].float().mean()
        else:
            ended += int(done.sum()); started += int(info["episode_started"].sum()); inside += float(info["resetting"].float().mean())
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    ended, started, inside = int(ended), int(started), float(inside)
    out = {"metric": "env-steps/sec rearrange/%s batch %d WITH episode ends: pipelined in-step resets (the reference's full reset recipe inside the step calls), recipe steps counted as env-steps" % ("ycb num_objects=8" if ycb else "blocks num_objects=5", B),
           "value": B * args.steps / elapsed, "unit": "env-steps/s", "n_gpus": 1, "steps": args.steps, "warmup": warm_steps, "ms_per_step": 1e3 * elapsed / args.steps, "dtype": "f32", "data": "synthetic",
           "config": {"workload": "as the rearrange line above; episode ends forced at %d live envs per step (one object put off the table) through %d warm-up steps and the timed window" % (knock_per_step, warm_steps),
                      "fraction_of_env_steps_inside_the_reset_recipe": inside / max(args.steps, 1), "episodes_ended_in_window": ended, "episodes_started_in_window": started, "device_reset": bool(device_reset),
                      "placements_out_of_trials": int(env.placement_failed.sum()) if device_reset else None,
                      "status_bits": int(max(env.sim.status.max().item(), env.solver_sim.status.max().item()))},
           "roofline": None, "cpu_baseline": None, "note": "same kernels and byte model as the rearrange line; envs that stabilise their objects skip the solver world's launch"}
    del env
    torch.cuda.empty_cache()
    return out


def bench_full_perpendicular(args, emit=True):
    """BASELINE.json configs[2]: dactyl/full_perpendicular (Shadow hand + full Rubik's cube, nv 168, condim-6 contacts), batch 4096
    on one MI355X: `BatchedFullPerpendicularEnv.step` = the large-model stepper (rb_step_kernel: action map, 10 mj_step, 3 PID ticks)
    + the env kernel (rb_post_step_kernel: FaceFreeGoal distances, reward, success, tracker, goal generation, observation row), after
    the reference's reset recipe (scrambled cubes).  One JSON line with its own roofline (the physics launch); single GPU."""
    from robogym_amd.envs.dactyl.full_perpendicular import BatchedFullPerpendicularEnv

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    B = args.batch if args.batch != 8192 else 4096
    env = BatchedFullPerpendicularEnv(B, device=dev, starting_seed=20200901 + 2, pipelined_reset=args.pipelined_reset)
    env.stop_on_fall = bool(args.pipelined_reset)      # (with in-step resets a dropped cube ends the episode, as under the reference's StopOnFallWrapper)
    sim, model = env.sim, env.model
    env.constants.max_pose_resets = 6        # (bounded set-up time: envs whose cube is still off the palm after 6 passes of the recipe are stepped as they are)
    env.reset()
    on_palm0 = float((sim.scratch("site_xpos")[:, 3 * sim.center_site + 2] > 0.04).float().mean().item())
    gen = torch.Generator(device=dev); gen.manual_seed(20200901 + 2)
    step = lambda: env.step(torch.rand((B, 20), generator=gen, device=dev) * 2 - 1)
    for _ in range(args.warmup):
        step()
    sim.stats.zero_()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for pair in ev:
        env._physics_events = pair
        last = step()
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    env._physics_events = None
    if emit and args.dump_outputs:
        dump_outputs(args.dump_outputs, last)
    kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
    on_palm = float((sim.scratch("site_xpos")[:, 3 * sim.center_site + 2] > 0.04).float().mean().item())
    st = sim.stats.sum(0).cpu().numpy()
    nsub = max(st[3], 1.0)
    ncon, nefc, iters = float(st[0] / nsub), float(st[1] / nsub), float(st[2] / nsub)

    class _M:   # the byte model reads dims / k_dims
        dims = model.dims
        arrays = {"k_dims": None}
        k_dims = [0, 0, sim.info["nM"]]
    b_step, b_sub = algorithmic_bytes_per_env_step(_M, ncon, nefc, iters, sim.n_substeps, sim.nq + sim.nv)
    achieved = B * b_step / (kern_ms * 1e-3)
    out = {
        "metric": "env-steps/sec dactyl/full_perpendicular batch 4096 (BASELINE.json configs[2]); unwrapped env.step, parity vs the in-repo CPU oracle (unpinned; also unpinned: the reset "
                  "recipe's scramble restates pycuber's turn convention from memory, the PID clamp / smoothing order is restated from mujoco-py's documented semantics)",
        "value": B * args.steps / elapsed, "unit": "env-steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": "dactyl/full_perpendicular (Shadow hand + full Rubik's cube, nv=168, 135 bodies, condim-6 contacts), batch %d, iid U(-1,1) relative actions, 10 substeps x 0.008 s; env.step = physics + env kernel (face_free goals), after the reset recipe with scrambled cubes" % B,
                   "batch_per_gpu": B, "pipelined_reset": bool(args.pipelined_reset), "cube_on_palm_fraction_after_reset": on_palm0, "cube_on_palm_fraction_at_end": on_palm, "goals_so_far_mean": float(env.multi_goal_tracker.goals_so_far.float().mean().item()), "mean_ncon": ncon, "mean_nefc": nefc, "mean_newton_iters": iters, "status_bits": int(sim.status.max().item()), "lds_bytes_per_workgroup": sim.info["lds_bytes"]},
        "roofline": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": achieved / HBM_PEAK, "traffic": rb_traffic("full_perpendicular", B), "traffic_unit": "GB per launch (PMC, profiles/hbm_traffic.json)", "traffic_note": rb_traffic_note("full_perpendicular", B), "kernel": "rb_step_kernel", "kernel_ms": kern_ms,
                     "algorithmic_bytes_per_env_step": b_step, "algorithmic_bytes_per_substep": b_sub,
                     "frac_sparse_J": B * algorithmic_bytes_sparse(_M, sim.info["nM"], ncon, nefc, iters, sim.n_substeps, sim.nq + sim.nv)[0] / (kern_ms * 1e-3) / HBM_PEAK,
                     "note": "frac = SURVEY 8(d) DENSE byte model (nefc x nv Jacobian, 2 nv^2 solver terms) with this model's dimensions (nM 1193) and the run's measured ncon / nefc / iterations; frac_sparse_J = the same model with a constraint row counted at <= 16 dofs and M tree-sparse, which is what the stepper stores: the dense figure overstates the bytes of a kernel whose Jacobians are sparse"},
    }
    if args.full and not args.no_cpu_baseline:
        from oracle import cpu_baseline as cb

        out["cpu_baseline"] = cb.run_full_perpendicular(2.0)
    if emit:
        print(json.dumps(out, default=float))
    del env
    torch.cuda.empty_cache()
    return out


def bench_locked_variant(args, emit=True, pipelined_reset=False, default_make_env=False):
    """configs[1] in its two other shapes: the steady state with episode ends (pipelined in-step resets; the window starts after
    `warmup` steps so that recipe and live envs are mixed) and the reference's default `make_env()` (wrapper stack, randomize=True)."""
    from robogym_amd.envs.dactyl import locked as LK

    dev = torch.device("cuda", 0)
    B = args.batch
    if default_make_env:
        env = LK.make_env(batch_size=B, device=dev, starting_seed=20200901 + 1)
        label = "default make_env() (reference wrapper stack incl. randomize=True), unwrapped physics underneath"
    else:
        env = LK.make_simple_env(batch_size=B, device=dev, starting_seed=20200901 + 1, pipelined_reset=True)
        label = "make_simple_env(pipelined_reset=True): finished episodes run the reset recipe inside the step launches"
    env.reset()
    gen = torch.Generator(device=dev); gen.manual_seed(20200901 + 1)
    nu = 20
    if default_make_env:
        act = lambda: torch.randint(0, 11, (B, nu), generator=gen, device=dev)
    else:
        act = lambda: torch.rand((B, nu), generator=gen, device=dev) * 2 - 1
    for _ in range(args.warmup):
        env.step(act())
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        env.step(act())
    torch.cuda.synchronize(dev)
    elapsed = time.perf_counter() - t0
    out = {"metric": "env-steps/sec dactyl/locked batch %d: %s" % (B, label), "value": B * args.steps / elapsed, "unit": "env-steps/s", "n_gpus": 1, "steps": args.steps,
           "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "dtype": "f32", "data": "synthetic",
           "roofline": None, "cpu_baseline": None, "note": "same kernels and byte model as the headline line; its roofline / cpu_baseline objects apply"}
    if emit:
        print(json.dumps(out, default=float))
    del env
    torch.cuda.empty_cache()
    return out


def compact_secondary(e):
    """A secondary entry without its prose: the numbers, the workload's short name, what bounds it.  (The full entries made the one JSON line 19 kB; the text is in
    DESIGN.md section 6 and, with --verbose-secondary, in profiles/rNN_bench.json.)"""
    if "error" in e:
        return e
    r = lambda v, n: round(v, n) if isinstance(v, float) else v
    out = {"metric": e["metric"].split(";")[0].split(" (BASELINE")[0][:120], "value": r(e["value"], 1), "unit": e.get("unit"), "steps": e.get("steps"), "warmup": e.get("warmup"),
           "ms_per_step": r(e.get("ms_per_step"), 3), "dtype": e.get("dtype")}
    c = e.get("config")
    if isinstance(c, dict):
        cc = {"workload": str(c.get("workload", "")).split(" (")[0][:60]}
        for k in ("batch_per_gpu", "status_bits"):
            if k in c:
                cc[k] = c[k]
        if isinstance(c.get("launch_ms"), dict):
            cc["launch_ms"] = {k: r(v, 2) for k, v in c["launch_ms"].items()}
        for k in ("mean_ncon", "mean_nefc", "mean_newton_iters"):
            src = c.get("main", c)
            if isinstance(src, dict) and k in src:
                cc[k] = r(src[k], 2)
        out["config"] = cc
    elif c is not None:
        out["config"] = {"workload": str(c)[:60]}
    rf = e.get("roofline")
    if isinstance(rf, dict):
        out["roofline"] = {k: (r(rf[k], 4) if k in ("frac", "frac_sparse_J") else r(rf[k], 2)) for k in ("bound", "achieved", "peak", "unit", "frac", "frac_sparse_J", "traffic", "kernel_ms") if k in rf}
    cb = e.get("cpu_baseline")
    if isinstance(cb, dict):
        out["cpu_baseline"] = {k: r(cb[k], 1) for k in ("value", "unit", "cores", "kind") if k in cb}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="locked", choices=["locked", "full_perpendicular", "rearrange_blocks", "ycb"], help="locked = BASELINE.json configs[1] (the headline); full_perpendicular = configs[2]; rearrange_blocks = configs[3]")
    ap.add_argument("--full", action="store_true", help="also measure what the headline does not need: the CPU baseline, the long window and (locked) the shortened runs of every other built config under 'secondary'")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the arrays the last timed env.step returned (obs / reward / done / info) as DIR/<name>.npy, float32, <= 64 MB in all")
    ap.add_argument("--verbose-secondary", action="store_true", help="with --full: keep every field of the secondary entries (the line carries their numbers only: it stays under ~10 kB; tools/final_cycle.sh passes this for profiles/)")
    ap.add_argument("--no-secondary", action="store_true", help="with --full: skip the shortened runs of the other built configs that the line carries under 'secondary', and the long window")
    ap.add_argument("--control-mode", default="tcp+roll+yaw", choices=["tcp+roll+yaw", "joint"], help="rearrange workloads: robot_control_params.control_mode")
    ap.add_argument("--quick-reset", action="store_true", help="rearrange_blocks: a shortened reset recipe (20 / 2 / 20 steps instead of 100 / 10 / 100)")
    ap.add_argument("--gpus", type=int, default=1)
    # default window: the 20 steps right after the reset, where the cubes are still in the hands (iid random actions throw them off
    # over time and the workload gets cheaper: 100 steps after 10 warm-up steps measure ~10 % more; the line reports the on-palm fraction)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8192, help="envs per GPU")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-per-env-params", action="store_true", help="rearrange workloads: without the per-env model parameter rows (what the simulation randomizers and stabilize_objects write); default: with")
    ap.add_argument("--no-long-window", action="store_true", help="with --full: skip the >= 2 s continuation of the headline rollout (config.long_window)")
    ap.add_argument("--long-steps", type=int, default=300)
    ap.add_argument("--pipelined-reset", action="store_true", help="finished episodes run the reset recipe inside the step launches")
    ap.add_argument("--launch-flags", type=int, default=0, help="diagnostic: extra rg_step_args.flags of the step launches (4: no per-pair collision cache)")
    ap.add_argument("--sort-dispatch", type=int, default=1, help="dispatch the envs longest-expected-first (previous step's cycles)")
    args = ap.parse_args()

    if args.workload == "full_perpendicular":
        return bench_full_perpendicular(args)
    if args.workload in ("rearrange_blocks", "ycb"):
        return bench_rearrange_blocks(args, ycb=args.workload == "ycb", joint=args.control_mode == "joint")
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(relaunch_with_ranks(args.gpus))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        sys.exit("bench.py: --gpus %d but the launcher started %d ranks (WORLD_SIZE)" % (args.gpus, world))
    # RG_BENCH_FORCE_DIST=1: take the distributed branch (process group, barriers, all-gather, max-reduce) even with one rank, so the
    # RCCL code path can be executed on a 1-GPU box: torchrun --nproc-per-node 1 bench.py --gpus 1
    distributed = world > 1 or os.environ.get("RG_BENCH_FORCE_DIST") == "1"
    # TEST HOOK (tests/test_distributed.py): run this very code path on CPU, 2 ranks, gloo, kernel source on the emulation harness
    emul_path = os.environ.get("RG_BENCH_EMUL_LIB")
    lib = None
    if emul_path:
        from robogym_amd import _native
        lib = _native.bind(emul_path)
        dev = torch.device("cpu")
    else:
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    if distributed:
        import torch.distributed as dist

        if emul_path:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        assert dist.get_world_size() == args.gpus, (dist.get_world_size(), args.gpus)

    from robogym_amd.envs.dactyl.locked import LockedEnvConstants, make_simple_env

    B = args.batch
    kw = dict(lib=lib, constants=LockedEnvConstants(mujoco_substeps=1, reset_initial_steps=1, n_random_initial_steps=1)) if emul_path else {}
    env = make_simple_env(batch_size=B, device=dev, starting_seed=20200901 + 1 + rank, pipelined_reset=args.pipelined_reset,
                          sort_dispatch=bool(args.sort_dispatch) and not emul_path, **kw)
    env.reset()
    env.launch_flags = int(args.launch_flags)
    sim = env.mujoco_simulation
    gen = torch.Generator(device=dev)
    gen.manual_seed(20200901 + 1 + 1000 * rank)
    from robogym_amd.distributed import ShardedObservationGather

    gather = ShardedObservationGather(B, env.packed_dim, dev)

    def on_palm_fraction():
        return float(((sim.cube_body_z + sim.get_qpos("cube_position")[:, 2]) > 0.04).float().mean().item())

    def one_step():
        a = torch.rand((B, 20), generator=gen, device=dev) * 2 - 1
        obs, reward, done, info = env.step(a)
        # the only exchange of the path: the full observation (166 scalars) with reward and done riding in
        # the same buffer, all-gathered over RCCL/xGMI when N > 1, overlapped with the next step
        gather.start(env.packed_observation(reward, done))
        return obs, reward, done, info

    for _ in range(args.warmup):
        one_step()
    sim.set_field(7, torch.zeros((B, 4), device=dev))  # reset kernel statistics
    status_before = int(sim.status.max().item())       # capacity flags raised by the reset recipe / warm-up (sticky bits)
    sim.set_field(6, torch.zeros((B, 1), dtype=torch.int32, device=dev))
    on_palm_start = on_palm_fraction()
    # physics-kernel timing with events on the launch stream
    mk_event = (lambda: torch.cuda.Event(enable_timing=True)) if not emul_path else (lambda: None)
    ev = [(mk_event(), mk_event()) for _ in range(args.steps)]
    orig_env_step = sim.env_step
    state = {"i": 0}

    def timed_env_step(*a, **k):
        if k.get("action") is not None:
            s, e = ev[state["i"] % len(ev)]
            if s is not None: s.record()
            orig_env_step(*a, **k)
            if e is not None: e.record()
            state["i"] += 1
        else:
            orig_env_step(*a, **k)

    sim.env_step = timed_env_step
    sync = (lambda: torch.cuda.synchronize(dev)) if not emul_path else (lambda: None)
    if distributed:
        dist.barrier()
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = one_step()
    gather.finish()
    if distributed:
        dist.barrier()
    sync()
    elapsed = time.perf_counter() - t0
    sim.env_step = orig_env_step
    if rank == 0 and args.dump_outputs:      # (before the long window: the step's outputs are views of buffers the next step rewrites)
        dump_outputs(args.dump_outputs, last)
    if distributed:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    kern_ms = float(np.mean([s.elapsed_time(e) for s, e in ev])) if not emul_path else 1e3 * elapsed / args.steps
    on_palm_end = on_palm_fraction()
    stats = sim.get_field(7).sum(0).cpu().numpy()
    nsub_total = max(stats[3], 1.0)
    ncon, nefc, iters = float(stats[0] / nsub_total), float(stats[1] / nsub_total), float(stats[2] / nsub_total)
    status = int(sim.status.max().item())
    # the same rollout carried on over a window of >= 2 s (the driver's --steps 20 is 0.12 s of GPU time): reported next to the contract's K-step value, not as it
    long_window = None
    if args.full and not emul_path and not args.no_long_window and not args.no_secondary:      # (profiling runs pass --no-secondary: their kernel statistics then hold the K timed launches only)
        sync()
        tl = time.perf_counter()
        for _ in range(args.long_steps):
            one_step()
        gather.finish()
        if distributed:
            dist.barrier()
        sync()
        tl = time.perf_counter() - tl
        if distributed:
            t = torch.tensor([tl], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            tl = float(t.item())
        long_window = {"steps": args.long_steps, "seconds": tl, "value": world * B * args.long_steps / tl, "cube_on_palm_fraction_at_end": on_palm_fraction(),
                       "note": "the next %d steps of the same rollout; iid random actions throw the cubes off over time, so the workload gets cheaper (on-palm fraction)" % args.long_steps}

    if rank == 0:
        from robogym_amd.mujoco import simulation_interface as _si
        kernel_name = "rg_step_items_kernel (substep-granular dispatch) + masked rg_step_kernel (large configuration)" if (_si.SUBSTEP_ITEMS and not emul_path) else "rg_step_kernel"
        value = world * B * args.steps / elapsed
        b_step, b_sub = algorithmic_bytes_per_env_step(env.model, ncon, nefc, iters, sim.n_substeps, 166)
        achieved = B * b_step / (kern_ms * 1e-3)
        # HBM bytes per launch from the round's PMC passes (tools/profile_round.sh + summarize_profile.py); counters
        # cannot be read from inside this process, so the figure is the committed one IF it was measured on this very
        # kernel source (hash stamp) and batch size, else null
        traffic, tnote = None, ""
        try:
            t = json.load(open(os.path.join(ROOT, "profiles", "hbm_traffic.json")))
            if int(t["batch_per_gpu"]) == B and t.get("kernel_source_hash") == kernel_source_hash():
                traffic, tnote = float(t["bytes_per_launch"]) / 1e9, "; traffic (GB per launch) from profiles/hbm_traffic.json: " + t["source"]
            else:
                tnote = "; traffic null: profiles/hbm_traffic.json was measured on another kernel build"
        except (OSError, ValueError, KeyError):
            pass
        out = {
            "metric": "env-steps/sec (whole node) dactyl/locked batch 8192; qpos L\u221e vs MuJoCo (as restated by the in-repo CPU oracle: parity unpinned)",
            "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": "dactyl/locked (Shadow hand + locked cube, nv=36), batch %d per GPU, iid U(-1,1) relative actions, 10 substeps x 0.008 s" % B,
                       "batch_per_gpu": B, "global_batch": world * B, "parallelism": "dp%d (envs sharded, RCCL all-gather of obs rows)" % world,
                       "ranks": (dist.get_world_size() if distributed else 1), "collective_backend": (dist.get_backend() if distributed else None),
                       "mean_ncon": float(ncon), "mean_nefc": float(nefc), "mean_newton_iters": float(iters), "status_bits": status, "status_bits_before_timed_region": status_before,
                       "cube_on_palm_fraction": {"start_of_timed_region": on_palm_start, "end_of_timed_region": on_palm_end},
                       "parity": {"oracle": "in-repo CPU restatement of MuJoCo 2.0 (fp64); physics unpinned against MuJoCo itself (absent offline), env layer pinned by fixtures generated from the reference's source",
                                  "protocol": "re-synchronised one-env.step error (kernel restarted from the oracle's fp32-rounded state before every env.step): the stated fp32 tolerance; "
                                              "free-running first step with qpos L-inf > 1e-4 under THIS workload's iid random actions, next to the oracle's own source built in float (the algorithm's fp32 limit)",
                                  "measured": parity_measured(),
                                  "north_star_drift_statement": "<= 1e-4 over 1000 steps is met on the contact-light hold-pose protocol in the portal-plane configuration only (tests/test_gpu_parity.py); "
                                                                "under random actions no fp32 build of the algorithm meets it (tests/test_oracle.py::test_free_running_divergence_of_the_default_is_a_property_of_the_algorithm_at_fp32)",
                                  "source": "profiles/parity.json (tests/tools/parity_json.py: measured on the MI355X, stamped with the kernel-source hash; `measured` is null when the stamp is not this build's); asserted by tests/test_gpu_parity.py"},
                       "long_window": long_window, "pipelined_reset": bool(args.pipelined_reset), "sort_dispatch": bool(args.sort_dispatch), "substep_items": bool(_si.SUBSTEP_ITEMS),
                       "gathered_row": "obs 166 + reward 3 + done 1 = %d floats per env" % env.packed_dim},
            "roofline": {"bound": "hbm", "achieved": achieved / 1e9, "peak": HBM_PEAK / 1e9, "unit": "GB/s", "frac": achieved / HBM_PEAK, "traffic": traffic, "traffic_unit": "GB per launch (PMC)", "algorithmic_gb_per_launch": b_step * B / 1e9,
                         "kernel": kernel_name, "kernel_ms": kern_ms, "algorithmic_bytes_per_env_step": b_step, "algorithmic_bytes_per_substep": b_sub,
                         "note": "algorithmic bytes = SURVEY 8(d) stage-boundary model with measured ncon/nefc/iters; the fused kernel keeps stage arrays in LDS, so real HBM traffic is far below the algorithmic figure" + tnote},
        }
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline()
        if args.full and world == 1 and not emul_path and not args.no_secondary:
            # every other built config in the one line: shortened runs, each with its own roofline and cpu_baseline
            del env, sim, gather
            torch.cuda.empty_cache()
            import copy
            sec = []
            # windows of >= 2 s each whatever the driver's --steps: 300 steps of ~6 ms, 20 of ~115 ms, 30 of 64-90 ms
            plan = ((bench_locked_variant, dict(pipelined_reset=True), (300, 40, 8192)), (bench_locked_variant, dict(default_make_env=True), (300, 40, 8192)),
                    (bench_full_perpendicular, {}, (20, 2, 4096)), (bench_rearrange_blocks, {}, (30, 3, 4096)), (bench_rearrange_steady, {}, (30, 0, 4096)),
                    (bench_rearrange_blocks, dict(ycb=True), (30, 3, 4096)), (bench_rearrange_steady, dict(ycb=True), (30, 0, 4096)),
                    (bench_rearrange_blocks, dict(joint=True), (30, 3, 4096)))
            for fn, kw, (st_, wu_, b_) in plan:
                a2 = copy.copy(args); a2.steps, a2.warmup, a2.batch = st_, wu_, b_
                a2.pipelined_reset = False
                try:
                    sec.append(fn(a2, **kw) if fn is bench_rearrange_steady else fn(a2, emit=False, **kw))
                except Exception as ex:   # a secondary run must not cost the headline
                    sec.append({"metric": getattr(fn, "__name__", "?"), "error": repr(ex)})
            names = ("locked_pipelined_resets", "locked_default_make_env", "full_perpendicular", "rearrange_blocks", "rearrange_blocks_episode_ends", "ycb", "ycb_episode_ends", "rearrange_blocks_joint")
            out["secondary"] = sec if args.verbose_secondary else [compact_secondary(e) for e in sec]
            # every number of the line once more, at its very END: a reader who keeps only the tail of the run's stdout (the driver's log did) still sees all of them
            out["summary"] = dict([("headline_env_steps_per_s", round(out["value"])), ("roofline_frac", round(out["roofline"]["frac"], 4))] +
                                  [(n, round(e["value"]) if "value" in e else None) for n, e in zip(names, sec)])
        print(json.dumps(out, default=float))
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
