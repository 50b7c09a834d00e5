"""Digests of the rearrange envs' device state over a fixed seeded matrix, for comparing two builds of the library bit for bit (a refactor of the ra_* kernels
against its parent commit): one sha256 per reset / step / reset_goals call over the bytes of the packed observation row, the goal rows, the tracker, the recipe's rows
and both worlds' qpos, and of the per-env parameter block where the env has one.

    python tools/ra_identity_digest.py --lib A/librgstep.so --tier gpu > a.txt          # one process per library
    python tools/ra_identity_digest.py --lib B/librgstep.so --tier gpu > b.txt
    python tools/ra_identity_digest.py --compare a.txt b.txt [--baseline a2.txt]        # exit code 1 when a line differs (on which a.txt == a2.txt)

Tiers as tests/test_rearrange_sync_reset.py: emul (the emulation harness' library, B = 4, n_substeps = 1) and gpu (B = 64, n_substeps = 2), with its FAST recipe and a
goal time-out of one step per object, so that episodes end and restart through the recipe inside the steps taken.  The matrix: the nine goal kinds through their tasks'
make_env, rot_dist_type full / mod90 / mod180 and icp (ycb), object_groups single / sample, mixed per-env object counts, masked observations with soft_mask, control modes,
wrapped and unwrapped, pipelined device resets, the synchronous reset(mask) / reset_goals() on the device, and three rows of the host route (device_reset=False):
pipelined resets, the synchronous reset(mask), and a recorded scene whose goals advance; last, the synchronous reset(mask) on the device of a wrapped env."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TIERS = dict(emul=dict(device="cpu", B=4, n_substeps=1), gpu=dict(device="cuda:0", B=64, n_substeps=2))
ROWS = ("packed", "goal", "goal_rot", "qpos_goal", "static_obs", "goal_in_area", "obj_group", "num_active", "t", "steps", "ssl", "successes", "consecutive", "prev_valid",
        "prev_nsucc", "reward", "done", "stage", "left", "yaw", "hold", "scripted", "frozen", "reobserve", "nticks", "placement_failed")
STEPS = 30


def digest(env):
    env.sync()
    h = hashlib.sha256()
    worlds = [env.sim.qpos] + ([env.solver_sim.qpos] if env.solver_sim is not None else [])
    params = [env.sim.params.block] if env.per_env_parameters else []
    for ten in [getattr(env, name, None) for name in ROWS] + worlds + params:
        if ten is not None:
            h.update(ten.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def actions(env, gen):
    if env.wrapped:
        return torch.randint(0, env.n_action_bins, (env.B, env.action_dim), generator=gen).to(env.device)
    return (torch.rand((env.B, env.action_dim), generator=gen) * 2 - 1).to(env.device)


def matrix(tier, lib):
    """(name, env factory, protocol) rows"""
    from robogym_amd.envs.rearrange import blocks, blocks_attached, blocks_pickandplace, blocks_reach, blocks_stack, blocks_train, dominos, ycb
    kw = dict(batch_size=tier["B"], device=tier["device"], n_substeps=tier["n_substeps"], stabilize_steps=2, settle_steps=2, device_reset=True, starting_seed=3)
    if lib is not None:
        kw["lib"] = lib

    def task(mod, sp=None, constants=None, rc=None, wrapped=False, pipelined=True, **extra):
        parameters = {"n_random_initial_steps": 1, "simulation_params": dict(sp or {}), "robot_control_params": dict(rc or {})}
        constants = dict({"max_timesteps_per_goal_per_obj": 1}, **(constants or {}))
        return lambda: mod.make_env(parameters=parameters, constants=constants, apply_wrappers=wrapped, pipelined_reset=pipelined, **dict(kw, **extra))

    def fixed():
        rel = np.array([[0.1, 0.2], [0.5, 0.5], [0.9, 0.3], [0.3, 0.8], [0.7, 0.9]])
        yaw = np.linspace(0.0, 1.2, 5)
        quats = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], 1)
        args = dict(kw, n_random_initial_steps=1, max_timesteps_per_goal_per_obj=1, pipelined_reset=True, goal_kind="fixed", relative_placements=rel, init_quats=quats)
        return blocks.BatchedBlockRearrangeEnv(args.pop("batch_size"), **args)

    def recorded():
        golden = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "rearrange_holdout_initial_state_4_blocks_stacked.npz")
        base = blocks.load_state(golden, 4)
        moved = lambda dx, dy: {"obj_pos": base[:, :3] + [dx, dy, 0.0], "obj_quat": base[:, 3:]}
        args = dict(kw, device_reset=False, n_random_initial_steps=0, pipelined_reset=True, num_objects=4, initial_states=[moved(0.0, 0.0), moved(-0.3, 0.2)],
                    goal_states=[[moved(-0.2, 0.1), moved(0.0, 0.0)], [moved(-0.1, 0.3)]], advance_goals=True, successes_needed=3,
                    success_threshold={"obj_pos": 10.0, "obj_rot": 10.0, "rel_dist": 10.0})
        return blocks.BatchedBlockRearrangeEnv(args.pop("batch_size"), **args)

    rot = lambda kind: {"goal_args": {"rot_dist_type": kind, "randomize_goal_rot": True}}
    rows = [("kind object_state", task(blocks), "steps"), ("kind pickandplace", task(blocks_pickandplace, sp={"num_objects": 2}), "steps"),
            ("kind stack", task(blocks_stack), "steps"), ("kind reach", task(blocks_reach), "steps"),
            ("kind det-reach", task(blocks_reach, constants={"goal_generation": "det-state"}), "steps"), ("kind train", task(blocks_train), "steps"),
            ("kind dominos", task(dominos, constants={"is_holdout": True}), "steps"), ("kind attached", task(blocks_attached), "steps"), ("kind fixed", fixed, "steps")]
    rows += [("rot %s" % k, task(blocks, constants=rot(k)), "steps") for k in ("full", "mod90", "mod180")]
    rows += [("rot icp (ycb)", task(ycb, constants=rot("icp")), "steps")]
    rows += [("groups %s" % g, task(blocks, sp={"object_groups": g}), "steps") for g in ("single", "sample")]
    rows += [("counts mixed", task(blocks, sp={"num_objects": 3, "max_num_objects": 5}), "counts"),
             ("mask_obs soft", task(blocks, constants={"mask_obs_outside_placement_area": True, "goal_args": {"soft_mask": True}}), "steps"),
             ("mask_obs counts", task(blocks, sp={"num_objects": 3, "max_num_objects": 5}, constants={"mask_obs_outside_placement_area": True}), "counts")]
    rows += [("control %s" % c, task(blocks, rc={"control_mode": c}), "steps") for c in ("joint", "tcp+wrist")]
    rows += [("wrapped", task(blocks, wrapped=True), "steps"), ("wrapped stack", task(blocks_stack, wrapped=True), "steps"),
             ("sync reset(mask)", task(blocks, pipelined=False), "sync"),
             ("sync reset_goals", task(blocks, pipelined=False, constants={"success_threshold": {"obj_pos": 10.0, "obj_rot": 10.0}}), "regoal"),
             ("sync reset_goals reach", task(blocks_reach, pipelined=False, constants={"success_threshold": {"obj_pos": 10.0, "obj_rot": 10.0}}), "regoal")]
    rows += [("host pipelined", task(blocks, device_reset=False), "steps"), ("host reset(mask)", task(blocks, pipelined=False, device_reset=False), "sync host"),
             ("host recorded goals", recorded, "steps"),
             # (a wrapped env's synchronous reset: its launches take the recipe's scripted actions, the steps around them bin indices through the filter)
             ("sync reset(mask) wrapped", task(blocks, pipelined=False, wrapped=True), "sync")]
    return rows


def run(name, make, protocol):
    env = make()
    gen = torch.Generator(); gen.manual_seed(17)
    B, k = env.B, 0

    def say(what):
        nonlocal k
        print("%-24s %3d %-12s %s" % (name, k, what, digest(env)), flush=True)
        k += 1
    if protocol in ("counts",):
        env.reset(); say("reset")
        want = (np.arange(B) % 5 + 1).astype(np.int32); want[0], want[B - 1] = 1, 2      # with B = 4: counts (1, 2, 3, 2)
        env.set_num_objects_next(want)
    env.reset(); say("reset")
    for s in range(STEPS):
        env.step(actions(env, gen)); say("step")
        if protocol in ("sync", "sync host") and s % 6 == 5:        # finished envs, then a fixed subset whatever its state
            mask = env.done.clone() if s % 12 == 5 else torch.zeros(B, dtype=torch.bool, device=env.device).index_fill_(0, torch.tensor([0, B - 1], device=env.device), True)
            env.reset(mask=mask, on_device=protocol == "sync"); say("reset(mask)")
        if protocol == "regoal" and s % 3 == 0:
            env.reset_goals(on_device=True); say("reset_goals")
            if s >= 12:
                break
    ended = int(env.placement_failed.max()) if getattr(env, "placement_failed", None) is not None else -1
    print("%-24s     %-12s nticks %s placement_failed %d" % (name, "end", sorted(set(env.nticks.cpu().tolist())) if getattr(env, "nticks", None) is not None else "-", ended), flush=True)


def compare(a, b, baseline):
    la, lb = open(a).read().splitlines(), open(b).read().splitlines()
    lc = open(baseline).read().splitlines() if baseline else la
    unstable = [i for i, (x, y) in enumerate(zip(la, lc)) if x != y]
    bad = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y and i not in unstable]
    print("%s vs %s: %d / %d lines, %d differ%s" % (a, b, len(la), len(lb), len(bad), "" if not baseline else "; %s vs %s (the protocol against itself): %d lines differ" % (a, baseline, len(unstable))))
    for i in unstable:
        print("  not reproducible: %s" % la[i])
    for i in bad[:20]:
        print("  DIFFERENT: %s\n         vs: %s" % (la[i], lb[i]))
    return 1 if bad or len(la) != len(lb) or len(la) != len(lc) or not la else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib"); ap.add_argument("--tier", choices=sorted(TIERS), default="gpu"); ap.add_argument("--only", default=None, help="substring of the row names to run")
    ap.add_argument("--compare", nargs=2); ap.add_argument("--baseline", default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(args.compare[0], args.compare[1], args.baseline))
    lib = None
    if args.tier == "gpu":      # the product library is the one the package loads (RGSTEP_LIB); the emulation harness' goes through the envs' lib=
        os.environ["RGSTEP_LIB"] = os.path.abspath(args.lib)
    else:
        from robogym_amd import _native
        lib = _native.bind(os.path.abspath(args.lib))
    for name, make, protocol in matrix(TIERS[args.tier], lib):
        if args.only is None or args.only in name:
            run(name, make, protocol)


if __name__ == "__main__":
    main()
