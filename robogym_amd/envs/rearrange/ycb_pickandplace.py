"""rearrange/ycb_pickandplace (/root/reference/robogym/envs/rearrange/ycb_pickandplace.py): the ycb env (envs/rearrange/ycb.py, its shipped object sets) with
`PickAndPlaceGoal` -- one random object's goal raised by uniform(0.05, 0.25) after the placement."""
from robogym_amd.envs.rearrange import ycb


def make_env(batch_size: int = 4096, device="cuda:0", parameters=None, constants=None, starting_seed: int = 0, apply_wrappers: bool = True, **kw):
    """`YcbPickAndPlaceEnv.build`: ycb.make_env with goal_kind "pickandplace"."""
    return ycb.make_env(batch_size, device=device, parameters=parameters, constants=constants, starting_seed=starting_seed, apply_wrappers=apply_wrappers,
                        goal_kind="pickandplace", **kw)


def make_simple_env(*a, **kw):
    kw["apply_wrappers"] = False
    return make_env(*a, **kw)
