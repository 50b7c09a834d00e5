"""rearrange/blocks_stack (/root/reference/robogym/envs/rearrange/blocks_stack.py): the blocks env with `ObjectStackGoal` (goals/object_stack_goal.py) -- object 0's
box placed without the grid, the others stacked on that spot at + i * 2 * object_size, in a shuffled order unless the constant `fixed_order` (False by default, as
`BlockStackEnvConstants`); info gains `goal_dist_gripper_pos` (sum of |obj_pos - grip site|) and `goal_dist_grasped` (sum of the finger contacts).  Reward and success
read obj_pos / obj_rot only, as the reference's.  The reference's defaults: num_objects 2."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import check_block_count, split_task_args

#: ObjectStackGoal's `simulation_params.object_size` (simulation/base.py:71): the blocks' half size; the shipped worlds are built at this size
OBJECT_SIZE = 0.0254


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`BlockStackEnv.build`: blocks.make_env with goal_kind "stack", two blocks by default; constants.fixed_order."""
    parameters, constants, task = split_task_args(parameters, constants, num_objects_default=2, constant_names=("fixed_order",))
    check_block_count(parameters["simulation_params"]["num_objects"], parameters["simulation_params"].get("max_num_objects"))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                           goal_kind="stack", object_size=OBJECT_SIZE, fixed_order=bool(task.get("fixed_order", False)), **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
