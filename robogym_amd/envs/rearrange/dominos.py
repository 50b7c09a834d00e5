"""rearrange/dominos (/root/reference/robogym/envs/rearrange/dominos.py over simulation/dominos.py and goals/dominos.py): the blocks env with its boxes skewed by
`domino_eccentricity` (half sizes object_size * [1 / e, 1, e]: thinner, taller, the same volume) and the rotation distance "mod180" -- a domino turned by half a turn
about any of its axes is the same domino.  `constants.is_holdout = False` (default): `TrainStateGoal`, goal kind "train" with blocks_train's arguments; `True`:
`DominoStateGoal`, goal kind "dominos" -- the dominos on a circle arc, `object_size * domino_distance_mul` apart, each turned along the arc (ra_recipe_kernel's
ra_domino_arc; `domino_goal` on the host path).

The world is derived from the shipped 5-block model (envs/rearrange/xml.py `dominos_world`): no model file of its own.  One eccentricity per batch; `num_objects` 1, 2
or 5.  Everything else -- physics, observation, reward, tracker, wrappers, pipelined / device resets, object groups -- is envs/rearrange/blocks.py's."""
from robogym_amd.envs.rearrange import blocks
from robogym_amd.envs.rearrange._tasks import check_block_count, refuse_max_num_objects, split_task_args
from robogym_amd.envs.rearrange.blocks_train import HEIGHT_RANGE, OBJECT_SIZE
from robogym_amd.envs.rearrange.xml import load_dominos_model

#: DominosRearrangeSimParameters (simulation/dominos.py:15-23) and DominosRearrangeEnvConstants.goal_args (dominos.py:31-33)
DOMINO_ECCENTRICITY = 1.5
DOMINO_DISTANCE_MUL = 4.0
GOAL_ARGS = {"rot_dist_type": "mod180"}


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`DominosRearrangeEnv.build`: blocks.make_env on the domino world.  simulation_params.num_objects (5; 1, 2, 5) / domino_eccentricity (1.5) / domino_distance_mul (4),
    constants.is_holdout, constants.goal_args (default {"rot_dist_type": "mod180"}; a given dict replaces it as a whole, as the reference's attrs field does):
    rot_dist_type full / mod90 / mod180, randomize_goal_rot, rot_randomize_type "z_axis", and -- not holdout -- height_range, pickup_proba, stacking_proba."""
    refuse_max_num_objects(parameters, "rearrange/dominos (the domino world)")
    parameters, constants, task = split_task_args(parameters, constants, num_objects_default=5, sim_names=("domino_eccentricity", "domino_distance_mul"),
                                                  constant_names=("goal_args", "is_holdout"))
    n = parameters["simulation_params"]["num_objects"]
    check_block_count(n)
    holdout = bool(task.get("is_holdout", False))
    goal_args = dict(GOAL_ARGS if task.get("goal_args") is None else task["goal_args"])
    train_keys = () if holdout else ("height_range", "pickup_proba", "stacking_proba")
    args = blocks.goal_rot_args(goal_args, other=train_keys)
    if holdout:
        args.update(goal_kind="dominos")
    else:
        args.update(goal_kind="train", height_range=tuple(goal_args.get("height_range", HEIGHT_RANGE)), pickup_proba=float(goal_args.get("pickup_proba", 0.0)),
                    stacking_proba=float(goal_args.get("stacking_proba", 0.0)))
    model = load_dominos_model(int(n), float(task.get("domino_eccentricity", DOMINO_ECCENTRICITY)))
    return blocks.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers, model=model,
                           object_size=OBJECT_SIZE, domino_distance_mul=float(task.get("domino_distance_mul", DOMINO_DISTANCE_MUL)), **args, **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
