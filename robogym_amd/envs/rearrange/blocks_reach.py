"""rearrange/blocks_reach (/root/reference/robogym/envs/rearrange/blocks_reach.py): one block and `ObjectReachGoal` / `DeterministicReachGoal`
(goals/object_reach_goal.py, the constant `goal_generation` = "state" | "det-state") -- each goal moves the block itself to a new spot (`set_object_pos`) and sits
`simulation_params.target_height` (0.1) above it; the achieved position is the robot0:grip site, the achieved rotation zero; the goal-distance reward is the decrease
of the obj_pos distance (`_calculate_goal_distance_reward`)."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import refuse_max_num_objects, split_task_args

GOAL_GENERATIONS = {"state": "reach", "det-state": "det-reach"}


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`BlocksReachEnv.build`: blocks.make_env with goal_kind "reach" / "det-reach", one block."""
    refuse_max_num_objects(parameters, "rearrange/blocks_reach (the reach goals take exactly one object)")
    parameters, constants, task = split_task_args(parameters, constants, num_objects_default=1, sim_names=("target_height",), constant_names=("goal_generation",))
    if int(parameters["simulation_params"]["num_objects"]) != 1:
        raise NotImplementedError("blocks_reach: num_objects must be 1 (ObjectReachGoal: reach only supports one object)")
    gen = task.get("goal_generation", "state")
    if gen not in GOAL_GENERATIONS:
        raise ValueError("goal_generation %r is not one of %s (BlocksReachEnvConstants)" % (gen, ", ".join(GOAL_GENERATIONS)))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                           goal_kind=GOAL_GENERATIONS[gen], target_height=float(task.get("target_height", 0.1)), **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
