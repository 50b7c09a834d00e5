"""Shared plumbing of the rearrange block tasks (blocks_pickandplace.py, blocks_stack.py, blocks_reach.py, ycb_pickandplace.py): each is `BatchedBlockRearrangeEnv` /
`BatchedYcbRearrangeEnv` with another goal generator (`goal_kind`), built through the blocks / ycb `make_env` surface with the task's own defaults and names."""

#: object counts the task envs are built and tested for: the shipped 5-block world and the 1- and 2-block worlds cut out of it (envs/rearrange/xml.py
#: blocks_world_subset)
SHIPPED_BLOCK_COUNTS = (1, 2, 5)


def split_task_args(parameters, constants, num_objects_default, sim_names=(), constant_names=()):
    """(parameters, constants, task) with the task's own names taken out: `sim_names` from parameters.simulation_params, `constant_names` from constants; the
    default object count filled in."""
    parameters, constants = dict(parameters or {}), dict(constants or {})
    sp = dict(parameters.get("simulation_params", {}))
    sp.setdefault("num_objects", num_objects_default)
    task = {k: sp.pop(k) for k in sim_names if k in sp}
    task.update({k: constants.pop(k) for k in constant_names if k in constants})
    parameters["simulation_params"] = sp
    return parameters, constants, task


def check_block_count(num_objects, max_num_objects=None):
    """`max_num_objects` (per-env object counts): the world is the one with that many blocks, and `num_objects`, the first count of every env, any of 1..max."""
    n = int(num_objects)
    counts = SHIPPED_BLOCK_COUNTS
    if max_num_objects is not None:
        if int(max_num_objects) not in counts:
            raise NotImplementedError("max_num_objects=%d: the block tasks are built for worlds of %s objects" % (int(max_num_objects), ", ".join(map(str, counts))))
        if not 1 <= n <= int(max_num_objects):
            raise ValueError("num_objects=%d is outside 1..max_num_objects=%d" % (n, int(max_num_objects)))
        return
    if n not in counts:
        raise NotImplementedError("num_objects=%d: the block tasks are built for %s objects" % (n, ", ".join(map(str, counts))))


def refuse_max_num_objects(parameters, task):
    """the tasks whose goal generator or world is not built for per-env object counts name the parameter they refuse"""
    if "max_num_objects" in dict((parameters or {}).get("simulation_params", {})):
        raise NotImplementedError("parameters.simulation_params.max_num_objects (per-env object counts) is not implemented for %s by the batched rearrange env" % task)
