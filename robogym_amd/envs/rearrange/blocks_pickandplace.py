"""rearrange/blocks_pickandplace (/root/reference/robogym/envs/rearrange/blocks_pickandplace.py): the blocks env with `PickAndPlaceGoal` (goals/pickandplace.py) --
`ObjectStateGoal`'s placement, then one random object's goal raised by uniform(0.05, 0.25) (`move_one_object_to_the_air`).  The reference's defaults: num_objects 1.
Everything else -- physics, observation, reward, wrappers, pipelined / device resets -- is envs/rearrange/blocks.py's."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import check_block_count, split_task_args


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`BlocksPickAndPlaceEnv.build`: blocks.make_env with goal_kind "pickandplace" and one block by default."""
    parameters, constants, _ = split_task_args(parameters, constants, num_objects_default=1)
    check_block_count(parameters["simulation_params"]["num_objects"], parameters["simulation_params"].get("max_num_objects"))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                           goal_kind="pickandplace", **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
