"""rearrange/blocks_duplicate (/root/reference/robogym/envs/rearrange/blocks_duplicate.py): the blocks env whose blocks are all duplicates of one another --
`DuplicateBlockRearrangeEnv._sample_random_object_groups` returns ONE group holding every object, so any block on any goal counts: the env kernel matches blocks to
goals greedily by distance (ra_group_match, robogym_amd/csrc/ra_env_kernel.h) before it measures relative goal, distances and success.  The reference's defaults:
num_objects 2.  Everything else -- physics, observation, reward, wrappers, pipelined / device resets -- is envs/rearrange/blocks.py's."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import check_block_count, split_task_args


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`DuplicateBlockRearrangeEnv.build`: blocks.make_env with object_groups "single" and two blocks by default."""
    parameters, constants, task = split_task_args(parameters, constants, num_objects_default=2, sim_names=("object_groups",))
    check_block_count(parameters["simulation_params"]["num_objects"], parameters["simulation_params"].get("max_num_objects"))
    if task.get("object_groups", "single") != "single":
        raise ValueError("blocks_duplicate puts every block in one group; object_groups=%r belongs to envs/rearrange/blocks.py" % (task["object_groups"],))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                           object_groups="single", **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
