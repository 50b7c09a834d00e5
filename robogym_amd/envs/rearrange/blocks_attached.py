"""rearrange/blocks_attached (/root/reference/robogym/envs/rearrange/blocks_attached.py over goals/attached_block_state.py): the blocks env with EIGHT blocks whose goals
are tightly attached to each other in a fixed lattice,

         [ ][ ]
      [ ][ ][ ][ ]
         [ ][ ]

`AttachedBlockStateGoal`, goal kind "attached": a random permutation decides which block goes to which cell, one uniform draw where the lattice sits in the placement
area, and `place_targets_with_fixed_position` puts the goals there (ra_recipe_kernel's ra_attached_table + ra_place_fixed; `attached_goal` + `fixed_goal` on the host path).
The goals' orientations are the identity, always: the generator sets them itself, so `goal_args.randomize_goal_rot` has no effect, as in the reference.

The world is the shipped 5-block model grown to eight blocks (envs/rearrange/xml.py `load_blocks_model(8)`: nv 56, nq 64 -- rb_step_kernel's medium configuration, as
rearrange/ycb).
Everything else -- physics, observation, reward, tracker, wrappers, pipelined / device resets, control modes, object groups -- is envs/rearrange/blocks.py's."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import refuse_max_num_objects, split_task_args
from robogym_amd.envs.rearrange.blocks_train import OBJECT_SIZE

#: AttachedBlockRearrangeEnvParameters.simulation_params (blocks_attached.py:18-22); the goal generator hard-codes eight target quaternions (attached_block_state.py:21)
NUM_OBJECTS = 8


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`AttachedBlockRearrangeEnv.build`: blocks.make_env with eight blocks and the attached goal.  simulation_params.num_objects (8, nothing else), constants.goal_args:
    rot_dist_type full / mod90 / mod180, randomize_goal_rot (accepted, without effect on this goal), rot_randomize_type "z_axis"."""
    refuse_max_num_objects(parameters, "rearrange/blocks_attached (AttachedBlockStateGoal places eight blocks)")
    parameters, constants, task = split_task_args(parameters, constants, num_objects_default=NUM_OBJECTS, constant_names=("goal_args",))
    n = int(parameters["simulation_params"]["num_objects"])
    if n != NUM_OBJECTS:
        raise NotImplementedError("num_objects=%d: rearrange/blocks_attached is built for %d blocks (AttachedBlockStateGoal places eight)" % (n, NUM_OBJECTS))
    args = blocks.goal_rot_args(task.get("goal_args"))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                           goal_kind="attached", object_size=OBJECT_SIZE, **args, **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
