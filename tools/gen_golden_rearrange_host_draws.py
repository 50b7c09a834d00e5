"""Golden record of the host reset / goal recipe of envs/rearrange/blocks.py (tests/golden/rearrange_host_draws.npz): for one small env per goal kind and option that
takes another branch, what `_begin_episode_state`, `_next_goal` and `_write_goal` leave behind for seed 7 -- the drawn yaws, the objects' poses, the static
observation, the group and count rows, two goals in a row -- and one more draw of the env's generator, which pins how many draws were consumed.  The samplers have
goldens of their own (tools/gen_golden_rearrange_*.py, from the reference's code); this pins the ORDER in which the env calls them.  No physics runs, so nothing here
depends on the stepper.

`record_host_draws(lib)` is shared with tests/test_rearrange_env.py::test_host_recipe_draws_are_pinned_emul, which replays it.

    make -C tests/emul && python tools/gen_golden_rearrange_host_draws.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
OUT = os.path.join(ROOT, "tests", "golden", "rearrange_host_draws.npz")

B, SEED = 3, 7
FAST = dict(n_substeps=1, stabilize_steps=1, n_random_initial_steps=0, settle_steps=0)
FIXED_PLACEMENTS = [[0.1, 0.2], [0.9, 0.15], [0.5, 0.5], [0.3, 0.85], [0.75, 0.7]]
FIXED_YAWS = [0.0, 0.4, -1.3, 2.9, 1.0]


def configurations(lib):
    """name -> a function that builds the env (the smallest one that takes each branch of the recipe)"""
    import torch  # noqa: F401

    from robogym_amd.envs.rearrange import blocks_attached
    from robogym_amd.envs.rearrange.blocks import BatchedBlockRearrangeEnv as Env
    from robogym_amd.envs.rearrange.xml import load_dominos_model
    from robogym_amd.envs.rearrange.ycb import BatchedYcbRearrangeEnv

    kw = dict(device="cpu", lib=lib, starting_seed=SEED, **FAST)
    mk = lambda cls=Env, **more: (lambda: cls(B, **kw, **more))
    quats = [[np.cos(0.5 * y), 0.0, 0.0, np.sin(0.5 * y)] for y in FIXED_YAWS]
    train = dict(goal_kind="train", pickup_proba=0.3, stacking_proba=0.3, goal_distance_ratio=[0.2, 0.6, 1.0])

    def counted(**more):
        def make():
            env = Env(B, num_objects=3, max_num_objects=5, **kw, **more)
            env.set_num_objects_next([1, 3, 5])
            return env
        return make

    return {
        "object_state": mk(num_objects=5, goal_kind="object_state"),
        "object_state_rot_groups": mk(num_objects=5, goal_kind="object_state", randomize_goal_rot=True, object_groups="sample"),
        "pickandplace": mk(num_objects=5, goal_kind="pickandplace"),
        "stack": mk(num_objects=2, goal_kind="stack"),
        "reach": mk(num_objects=1, goal_kind="reach"),
        "det-reach": mk(num_objects=1, goal_kind="det-reach"),
        "train": mk(num_objects=5, **train),
        "dominos": mk(num_objects=5, goal_kind="dominos", model=load_dominos_model(5), rot_dist_type="mod180", randomize_goal_rot=True),
        "attached": lambda: blocks_attached.make_simple_env(batch_size=B, **kw),
        "fixed": mk(num_objects=5, goal_kind="fixed", relative_placements=FIXED_PLACEMENTS, init_quats=quats),
        "counts_object_state": counted(goal_kind="object_state", randomize_goal_rot=True, object_groups="sample"),
        "counts_train": counted(**train),
        "ycb": mk(BatchedYcbRearrangeEnv, num_objects=8, goal_kind="object_state"),
    }


def record_host_draws(lib):
    """-> {"<configuration>/<what>": array}: float64 for host values, float32 / int32 for device rows"""
    import torch

    out = {}
    for name, make in configurations(lib).items():
        env = make()
        rows, idx = np.arange(B), torch.arange(B)
        put = lambda what, v: out.__setitem__("%s/%s" % (name, what), v.cpu().numpy().copy() if isinstance(v, torch.Tensor) else np.asarray(v, dtype=np.float64).copy())
        yaw = env._begin_episode_state(rows, idx)
        put("yaw", yaw)
        put("obj_qpos", torch.stack([env.sim.qpos[:, qa:qa + 7] for qa in env.obj_q], 1))
        put("static_obs", env.static_obs)
        for what in ("obj_group", "num_active"):
            if getattr(env, what) is not None:
                put(what, getattr(env, what))
        for k in (1, 2):
            env._write_goal(rows, *env._next_goal(rows, yaw))
            for what in ("goal", "goal_rot", "qpos_goal"):
                put("%s%d" % (what, k), getattr(env, what))
            if env.goal_kind_name in ("reach", "det-reach"):
                put("qpos%d" % k, env.sim.qpos)
            if env.goal_kind_name == "det-reach":
                put("goal_index%d" % k, env.goal_index)
            yaw = env.goal_rot[idx, :, 2].cpu().numpy().astype(np.float64)      # (the next goal as reset_goals makes it)
        put("next_uniform", env._rng.uniform())
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from robogym_amd import _native

    rec = record_host_draws(_native.bind(os.path.join(ROOT, "tests", "emul", "librgstep_emul.so")))
    np.savez_compressed(OUT, **rec)
    print("wrote %s: %d arrays, %d bytes" % (os.path.relpath(OUT, ROOT), len(rec), os.path.getsize(OUT)))
