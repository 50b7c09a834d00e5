"""The vectorised default wrapper stack (robogym_amd/wrappers/dactyl_cube.py) against the REAL reference
stack: tests/golden/wrappers.npz holds what the reference's own wrapper classes, stacked by its construct_default_wrappers /
apply_named_wrappers (randomize=False), produce around a scripted inner env (tools/gen_golden_wrappers.py); the batched
stack around the same scripted inner env must return the same observation keys in the same order, the same values, rewards
(with the drop term), dones and info, and must hand the same continuous actions down to the env."""
import os
import types

import numpy as np
import pytest
import torch

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = [torch.device("cpu")]     # the golden replays run on this device (the `_gpu` variants switch it to cuda:0)
OBS_KEYS = ["cube_pos", "cube_quat", "qpos", "qvel", "hand_angle", "fingertip_pos", "goal_pos", "goal_quat", "qpos_goal", "is_goal_achieved"]


class ScriptedBatchedEnv:
    """Batched stand-in for BatchedLockedEnv replaying the golden script in every row."""

    def __init__(self, g, B=3):
        self.g, self.batch_size, self.device, self.num_actions, self._seed, self.t = g, B, DEV[0], 20, 0, 0
        self.mujoco_simulation = types.SimpleNamespace(cube_body_z=0.2, n_substeps=10, model=types.SimpleNamespace(opt_timestep=np.array([0.008])))
        self.received = []
        self.stop_on_fall = True

    def _emit(self):
        rep = lambda a: torch.as_tensor(np.repeat(a[None], self.batch_size, 0), dtype=torch.float64, device=self.device)
        obs = {k: rep(self.g["script_obs_" + k][self.t]) for k in OBS_KEYS}
        self._goal_quat = obs["goal_quat"]
        return obs

    def reset(self, mask=None):
        self.t = 0
        return self._emit()

    def step(self, a):
        self.received.append(a[0].cpu().numpy().copy())
        self.t += 1
        rep = lambda a: torch.as_tensor(np.repeat(np.asarray(a)[None], self.batch_size, 0), device=self.device)
        info = {"successes_so_far": rep(int(self.g["script_successes_so_far"][self.t])).to(torch.int32)}
        return self._emit(), rep(self.g["script_reward"][self.t]).double(), rep(bool(self.g["script_done"][self.t])), info


def test_default_wrapper_stack_matches_reference_stack():
    _default_golden_replay()


@pytest.mark.gpu
def test_default_wrapper_stack_matches_reference_stack_gpu():
    """The same golden replay with every tensor of the stack on the MI355X (the goldens ran on CPU tensors only)."""
    DEV[0] = torch.device("cuda:0")
    try:
        _default_golden_replay()
    finally:
        DEV[0] = torch.device("cpu")


def _default_golden_replay():
    from robogym_amd.wrappers.dactyl_cube import BatchedDactylCubeWrappers

    g = np.load(os.path.join(G, "wrappers.npz"))
    inner = ScriptedBatchedEnv(g)
    env = BatchedDactylCubeWrappers(inner, randomize=False)
    keys = [str(k) for k in g["obs_keys"]]
    obs = env.reset()
    T = len(g["actions"])
    for t in range(T + 1):
        if t > 0:
            obs, reward, done, info = env.step(torch.as_tensor(np.repeat(g["actions"][t - 1][None], inner.batch_size, 0), device=DEV[0]))
            np.testing.assert_allclose(reward[0].cpu().numpy(), g["wreward"][t - 1], atol=1e-6, err_msg="reward at step %d" % t)
            assert bool(done[0]) == bool(g["wdone"][t - 1]), t
            for k in ("fell_down", "drops_so_far", "first_drop"):
                assert int(info[k][0]) == int(g["winfo_" + k][t - 1]), (k, t)
            assert (reward == reward[0]).all() and (done == done[0]).all()     # every row of the batch alike
        assert list(obs.keys()) == keys, (list(obs.keys()), keys)
        for k in keys:
            np.testing.assert_allclose(obs[k][0].double().cpu().numpy().ravel(), g["wobs_" + k][t], atol=1e-6, err_msg="%s at step %d" % (k, t))
    np.testing.assert_allclose(np.stack(inner.received), g["received_actions"], atol=1e-6)   # what reaches the env: binned, smoothed, clipped
    assert env.action_space["nvec"] == [11] * 20


# ---------------------------------------------------------------------------------------------------------------------------
# the same stack around the FULL cube's observation set, with FaceFreeGoal.relative_goal (tests/golden/wrappers_full.npz: the reference's wrapper classes and the goal
# class's own relative_goal source, tools/gen_golden_wrappers.py main_full)
FULL_OBS_KEYS = ["cube_pos", "cube_quat", "cube_face_angle", "qpos", "qvel", "perp_qpos", "perp_qvel", "hand_angle", "fingertip_pos", "goal_pos", "goal_quat", "goal_face_angle"]


class FullScriptedBatchedEnv(ScriptedBatchedEnv):
    """Batched stand-in for BatchedFullPerpendicularEnv: the script's observations and goal rows in the env's own layout (quat 4, face angles 6, goal_type, axis_nr,
    axis_sign), `relative_goal` = the real env's method."""

    def _emit(self):
        from robogym_amd import _native

        rep = lambda a: torch.as_tensor(np.repeat(np.asarray(a)[None], self.batch_size, 0), dtype=torch.float64, device=self.device)
        obs = {k: rep(self.g["script_obs_" + k][self.t]) for k in FULL_OBS_KEYS}
        goal = torch.zeros((self.batch_size, _native.RB_GOAL_WORDS), dtype=torch.float64, device=self.device)
        goal[:, 0:4], goal[:, 4:10] = obs["goal_quat"], obs["goal_face_angle"]
        goal[:, 10], goal[:, 11], goal[:, 12] = float(self.g["script_goal_rotation"][self.t]), float(self.g["script_axis_nr"][self.t]), float(self.g["script_axis_sign"][self.t])
        self._goal = goal
        return obs

    def relative_goal(self, key, current):
        from robogym_amd.envs.dactyl.full_perpendicular import BatchedFullPerpendicularEnv

        return BatchedFullPerpendicularEnv.relative_goal(self, key, current)


def _full_golden_replay():
    from robogym_amd.wrappers.dactyl_cube import BatchedDactylCubeWrappers

    g = np.load(os.path.join(G, "wrappers_full.npz"))
    inner = FullScriptedBatchedEnv(g)
    env = BatchedDactylCubeWrappers(inner, randomize=False)
    assert env.full_cube and sorted(env.levels) == ["cube_face_angle", "cube_pos", "cube_quat", "fingertip_pos", "hand_angle"]
    keys = [str(k) for k in g["obs_keys"]]
    obs = env.reset()
    T = len(g["actions"])
    kinds = set()
    for t in range(T + 1):
        if t > 0:
            obs, reward, done, info = env.step(torch.as_tensor(np.repeat(g["actions"][t - 1][None], inner.batch_size, 0), device=DEV[0]))
            np.testing.assert_allclose(reward[0].cpu().numpy(), g["wreward"][t - 1], atol=1e-6, err_msg="reward at step %d" % t)
            assert bool(done[0]) == bool(g["wdone"][t - 1]), t
            for k in ("fell_down", "drops_so_far", "first_drop"):
                assert int(info[k][0]) == int(g["winfo_" + k][t - 1]), (k, t)
        assert list(obs.keys()) == keys, (list(obs.keys()), keys)
        for k in keys:
            np.testing.assert_allclose(obs[k][0].double().cpu().numpy().ravel(), g["wobs_" + k][t], atol=1e-6, err_msg="%s at step %d" % (k, t))
        kinds.add(bool(g["script_goal_rotation"][t]))
    assert kinds == {True, False}                      # both goal types of FaceFreeGoal.relative_goal went through
    np.testing.assert_allclose(np.stack(inner.received), g["received_actions"], atol=1e-6)
    assert obs["relative_goal"].shape == (inner.batch_size, 3 + 4 + 12) and obs["goal"].shape == (inner.batch_size, 19)
    with pytest.raises(NotImplementedError):
        BatchedDactylCubeWrappers(FullScriptedBatchedEnv(g), randomize=True)


def test_full_cube_wrapper_stack_matches_reference_stack():
    _full_golden_replay()


@pytest.mark.gpu
def test_full_cube_wrapper_stack_matches_reference_stack_gpu():
    DEV[0] = torch.device("cuda:0")
    try:
        _full_golden_replay()
    finally:
        DEV[0] = torch.device("cpu")


@pytest.mark.gpu
def test_full_cube_make_env_with_wrappers_gpu():
    """`full_perpendicular.make_env(constants={"randomize": False})` around the real batched env on the MI355X: the wrapped keys and widths, MultiDiscrete actions
    through the launch, the relative goal consistent with the env kernel's own goal distance (|relative face angles| = cube_face_angle distance), drop penalty."""
    from robogym_amd.envs.dactyl.full_perpendicular import make_env

    with pytest.raises(NotImplementedError):
        make_env(batch_size=2)                                                            # the reference's default is randomize=True: not silently narrowed
    env = make_env(constants={"randomize": False}, batch_size=8, starting_seed=3)
    obs = env.reset()
    g = np.load(os.path.join(G, "wrappers_full.npz"))
    assert list(obs.keys()) == [str(k) for k in g["obs_keys"]]
    assert obs["relative_goal"].shape == (8, 19) and obs["noisy_cube_face_angle"].shape == (8, 12) and obs["cube_face_angle"].shape == (8, 12) and obs["reward"].shape == (8, 2)
    gen = torch.Generator(device="cpu").manual_seed(0)
    for _ in range(5):
        obs, reward, done, info = env.step(torch.randint(0, 11, (8, 20), generator=gen).to(env.device))
    assert reward.shape == (8, 4) and bool(torch.isfinite(obs["relative_goal"]).all()) and int(env.unwrapped.mujoco_simulation.status.max()) == 0
    raw = env.unwrapped
    rel = raw.relative_goal("cube_face_angle", raw.observe()["cube_face_angle"])
    assert torch.allclose(rel.norm(dim=1), info["goal_dist"]["cube_face_angle"], atol=1e-4)
    relq = raw.relative_goal("cube_quat", raw.observe()["cube_quat"])
    from robogym_amd.utils import rotation
    assert torch.allclose(rotation.quat_magnitude(relq), info["goal_dist"]["cube_quat"], atol=1e-4)


def test_wrapper_stack_on_the_kernel_emul(locked_model, emul_lib):
    """make_env() default (apply_wrappers=True) around the real batched env: shapes, drop penalty and done when the cube is
    thrown off, noise statistics with randomize=True, per-env physics rows actually written."""
    from robogym_amd.envs.dactyl.locked import make_env

    env = make_env(constants={"mujoco_substeps": 2, "reset_initial_steps": 1, "n_random_initial_steps": 1, "randomize": True}, batch_size=3, model=locked_model, lib=emul_lib, starting_seed=2)
    obs = env.reset()
    assert obs["hand_angle"].shape == (3, 48) and obs["noisy_hand_angle"].shape == (3, 48) and obs["goal"].shape == (3, 7) and obs["relative_goal"].shape == (3, 7)
    assert obs["reward"].shape == (3, 2) and obs["previous_action"].shape == (3, 20) and obs["fell_down"].shape == (3, 1)
    P = env.unwrapped.mujoco_simulation.params
    assert not torch.equal(P["gravity"][0], P["gravity"][1]) and not torch.equal(P["dof_damping"][0], P["dof_damping"][1])   # per-env physics draws
    assert (P["geom_friction"][:, :, 0] > 0).all()
    assert not torch.equal(obs["noisy_cube_pos"], obs["cube_pos"])                               # observation noise on
    a = torch.randint(0, 11, (3, 20))
    obs, reward, done, info = env.step(a)
    assert reward.shape == (3, 4) and done.shape == (3,) and (reward[:, 3] == 0).all()
    # throw the cube of env 1 away: next step reports the drop once
    sim = env.unwrapped.mujoco_simulation
    q = sim.view(0); q[1, 2] = -0.5; sim.touch_qpos()
    obs, reward, done, info = env.step(a)
    assert bool(done[1]) and float(reward[1, 3]) == -20.0 and bool(info["fell_down"][1]) and int(info["drops_so_far"][1]) == 1
    assert not bool(info["fell_down"][0]) and float(reward[0, 3]) == 0.0
    obs, reward, done, info = env.step(a)
    assert float(reward[1, 3]) == 0.0 and int(info["drops_so_far"][1]) == 2                      # penalised on the first frame only


# ---------------------------------------------------------------------------------------------------------------------------
# randomize=True: the full default stack of LockedEnv replayed on the draw log of the REAL reference wrapper classes
class ReplayDraws:
    """Feeds the vectorised stack the values the reference's wrappers drew from the env's RandomState (in the reference's order;
    a mismatch of draw kind or size fails), the same in every row of the batch."""

    def __init__(self, g, B):
        self.names, self.off, self.val, self.B, self.i = [str(n) for n in g["draw_names"]], g["draw_offsets"], g["draw_values"], B, 0

    def _next(self, name, shape):
        assert self.i < len(self.names), "the stack draws more often than the reference"
        assert self.names[self.i] == name, "draw %d: the reference drew %s, the stack asks for %s%s" % (self.i, self.names[self.i], name, tuple(shape))
        v = self.val[self.off[self.i]:self.off[self.i + 1]]
        assert len(v) == max(int(np.prod(shape)), 1), "draw %d (%s): %d values recorded, %s requested" % (self.i, name, len(v), tuple(shape))
        self.i += 1
        return torch.as_tensor(v, dtype=torch.float64, device=DEV[0]).reshape(tuple(shape))[None].repeat((self.B,) + (1,) * len(shape))

    def uniform(self, low, high, shape=()):
        return self._next("uniform", shape)

    def randn(self, shape):
        return self._next("randn", shape)

    def randn_where(self, cond, shape):
        return self._next("randn", shape) if bool(cond[0]) else torch.zeros((self.B,) + tuple(shape), dtype=torch.float64, device=DEV[0])

    def random_sample(self, shape=()):
        return self._next("random_sample", shape)

    def exponential(self, scale, shape=()):
        return self._next("exponential", shape)

    def randint(self, low, high, shape):
        return self._next("randint", shape).long()

    def choice(self, values):
        return self._next("choice", ())


class RandomizedScriptedBatchedEnv(ScriptedBatchedEnv):
    """... plus the simulation surface the randomizations touch: per-env parameter rows, qpos, the contact list."""

    def __init__(self, g, model, B=2):
        super().__init__(g, B)
        A = model.arrays
        rows = lambda a: torch.as_tensor(np.asarray(a, dtype=np.float64), device=DEV[0])[None].repeat((B,) + (1,) * np.asarray(a).ndim)
        self.params = {"gravity": rows(A["opt_gravity"]), "timestep": rows(A["opt_timestep"]), "dof_damping": rows(A["dof_damping"]), "body_inertia": rows(A["body_inertia"]),
                       "body_mass": rows(A["body_mass"]), "geom_friction": rows(A["geom_friction"]), "actuator_gainprm": rows(A["actuator_gainprm"][:, :10]),
                       "jnt_range": rows(A["jnt_range"]), "tendon_range": rows(A["tendon_range"]), "actuator_ctrlrange": rows(A["actuator_ctrlrange"]),
                       "site_pos": rows(A["site_pos"]), "geom_scale": torch.ones((B, 1), dtype=torch.float64, device=DEV[0]), "xfrc_applied": torch.zeros((B, len(A["body_mass"]), 6), dtype=torch.float64, device=DEV[0])}
        hand_q = np.array([int(A["jnt_qposadr"][j]) for j, n in enumerate(model.names["joint"]) if n.startswith("robot0:")])
        self.constants = types.SimpleNamespace(relative_action=True)
        con = g["script_contacts"]
        self._contacts = [con[con[:, 0] == t][:, 1:] for t in range(len(g["script_obs_qpos"]))]
        self.mujoco_simulation = types.SimpleNamespace(cube_body_z=0.2, n_substeps=10, model=model, params=self.params, pos_to_ctrl=g["pos_to_ctrl"],
                                                       qpos_idxs={"hand_angle": hand_q}, qpos=None, data=types.SimpleNamespace(ncon=None, contact=None),
                                                       touch_qpos=lambda mask=None: self.voided.append(mask))
        self.step_timestep, self.step_xfrc, self.voided = [], [], []      # (voided: the cache rows the stack asks the simulation to void -- with every geom_scale write)

    def _emit(self):
        obs = super()._emit()
        sim, B = self.mujoco_simulation, self.batch_size
        sim.qpos = obs["qpos"]
        c = self._contacts[self.t]
        pad = np.zeros((8, 3)); pad[:len(c)] = c
        rep = lambda a, dt: torch.as_tensor(np.repeat(a[None], B, 0), dtype=dt, device=self.device)
        sim.data.ncon = torch.full((B,), len(c), dtype=torch.int32, device=self.device)
        sim.data.contact = (rep(pad[:, 0], torch.int32), rep(pad[:, 1], torch.int32), rep(pad[:, 2], torch.float64))
        return obs

    def reset(self, mask=None):
        return self._emit()

    def step(self, a):
        self.step_timestep.append(float(self.params["timestep"][0, 0])); self.step_xfrc.append(self.params["xfrc_applied"][0].cpu().numpy().copy())
        return super().step(a)


def test_randomized_wrapper_stack_replays_the_reference_stack(locked_model):
    _randomized_golden_replay(locked_model)


@pytest.mark.gpu
def test_randomized_wrapper_stack_replays_the_reference_stack_gpu(locked_model):
    """The randomize=True golden replay (612 reference draws, 44 observation keys, model rows at both resets) on cuda:0."""
    DEV[0] = torch.device("cuda:0")
    try:
        _randomized_golden_replay(locked_model)
    finally:
        DEV[0] = torch.device("cpu")


def _randomized_golden_replay(locked_model):
    """randomize=True (the reference's default): BacklashWrapper, the thirteen pre-noise randomizations of LockedEnv, observation
    noise, occluded / freezing phasespace markers, action noise.  On the reference's own draws the vectorised stack must
    (a) ask for the same draws in the same order, (b) write the same values into the model rows at both resets, (c) return the
    same 44 observation keys / values, rewards and dones, (d) hand the same actions to the env, (e) run every env.step with
    the same timestep and wind force."""
    from robogym_amd.wrappers.dactyl_cube import BatchedDactylCubeWrappers

    g = np.load(os.path.join(G, "wrappers_randomized.npz"))
    inner = RandomizedScriptedBatchedEnv(g, locked_model)
    draws = ReplayDraws(g, inner.batch_size)
    env = BatchedDactylCubeWrappers(inner, randomize=True, draws=draws)
    keys = [str(k) for k in g["obs_keys"]]
    resets_at = [int(t) for t in g["resets_at"]]
    P, A, N = inner.params, locked_model.arrays, locked_model.names
    row = 0

    def check_obs(obs, what):
        nonlocal row
        assert list(obs.keys()) == keys, (list(obs.keys()), keys)
        for k in keys:
            np.testing.assert_allclose(obs[k][0].double().cpu().numpy().ravel(), g["wobs_" + k][row], atol=2e-6, rtol=2e-6, err_msg="%s at %s" % (k, what))
            assert (obs[k] == obs[k][0]).all()
        row += 1

    for t in range(len(g["actions"])):
        if t in resets_at:
            inner.t = t
            check_obs(env.reset(), "reset before step %d" % t)
            r = resets_at.index(t)
            assert len(inner.voided) >= r + 1      # a new cube size voids the cached pair distance bounds (include/rgstep.h, rg_batch_field_ptr)
            cube = N["geom"].index("cube:middle")
            for name, got in (("body_inertia", P["body_inertia"][0]), ("geom_friction", P["geom_friction"][0]), ("gravity", P["gravity"][0]), ("dof_damping", P["dof_damping"][0]),
                              ("actuator_kp", P["actuator_gainprm"][0, :, 0]), ("jnt_range", P["jnt_range"][0]), ("actuator_ctrlrange", P["actuator_ctrlrange"][0]),
                              ("tendon_range", P["tendon_range"][0]), ("site_pos", P["site_pos"][0]), ("cube_size", P["geom_scale"][0] * torch.as_tensor(A["geom_size"][cube], device=DEV[0]))):
                np.testing.assert_allclose(got.cpu().numpy(), g["model%d_%s" % (r, name)], rtol=1e-9, atol=1e-12, err_msg="model field %s after reset %d" % (name, r))
        obs, reward, done, info = env.step(torch.as_tensor(np.repeat(g["actions"][t][None], inner.batch_size, 0), device=DEV[0]))
        np.testing.assert_allclose(reward[0].cpu().numpy(), g["wreward"][t], atol=1e-6, err_msg="reward at step %d" % t)
        assert bool(done[0]) == bool(g["wdone"][t]), t
        for k in ("fell_down", "drops_so_far", "first_drop"):
            assert int(info[k][0]) == int(g["winfo_" + k][t]), (k, t)
        check_obs(obs, "step %d" % t)
    assert draws.i == len(draws.names), "the reference drew %d more times" % (len(draws.names) - draws.i)
    np.testing.assert_allclose(np.stack(inner.received), g["received_actions"], atol=2e-6)     # per-env wrapper state is fp32
    np.testing.assert_allclose(inner.step_timestep, g["step_timestep"], rtol=1e-12)
    cube_body = N["body"].index("cube:middle")
    np.testing.assert_allclose(np.stack(inner.step_xfrc)[:, cube_body, :3], g["step_xfrc"], rtol=1e-9, atol=1e-15)
    assert np.abs(g["received_actions"] - np.clip(np.linspace(-1, 1, 11)[g["actions"]], -1, 1)).max() > 0.05   # noise / latency / backlash did act


@pytest.mark.gpu
def test_informative_obs_gpu(locked_model):
    """Port of the reference's test_informative_obs (envs/dactyl/tests/test_locked.py:100-143): an episode of random actions
    through make_env(constants=dict(randomize=False, max_timesteps_per_goal=50)) plus one more reset; no observation key may
    be constant over the episode, except the reference's own whitelist.  And the default make_env() (randomize=True) runs."""
    from robogym_amd.envs.dactyl.locked import make_env

    WHITELIST = ["relative_goal_pos", "noisy_relative_goal_pos", "goal_pos", "fell_down", "is_goal_achieved"]
    env = make_env(constants=dict(randomize=False, max_timesteps_per_goal=50), batch_size=4, model=locked_model, starting_seed=3)
    obs = env.reset()
    all_obs = [obs]
    gen = torch.Generator(); gen.manual_seed(0)
    done0 = False
    while not done0:
        obs, reward, done, info = env.step(torch.randint(0, 11, (4, 20), generator=gen))
        all_obs.append(obs); done0 = bool(done[0])
    assert 1 < len(all_obs) <= 52
    all_obs.append(env.reset())
    keys = list(all_obs[0].keys())
    for o in all_obs:
        assert list(o.keys()) == keys
    for k in keys:
        if k in WHITELIST:
            continue
        first = all_obs[0][k][0]
        assert not all(torch.equal(first, o[k][0]) for o in all_obs), "observations for %s are all equal to %s" % (k, first)
    # the reference's default configuration: everything on
    env = make_env(batch_size=64, model=locked_model, starting_seed=4)
    obs = env.reset()
    assert len(obs) == 44 and obs["friction"].shape == (64, 195) and obs["joint_limit"].shape == (64, 64) and obs["randomized_phasespace_fingers"].shape == (64, 24)
    P = env.unwrapped.mujoco_simulation.params
    assert float((P["geom_scale"] - 1).abs().max()) > 0.01 and float((P["geom_scale"] - 1).abs().max()) <= 0.05
    for _ in range(30):
        obs, reward, done, info = env.step(torch.randint(0, 11, (64, 20), generator=gen))
    assert all(torch.isfinite(v.float()).all() for v in obs.values()) and int(env.unwrapped.sim_status().max()) == 0
    assert float(P["timestep"].min()) >= 0.004 - 1e-9 and float(P["timestep"].std()) > 0       # RandomizedTimestepWrapper at work, clipped at h/2
    assert float(info["fell_down"].float().mean()) < 0.5


def test_auto_reset_around_the_pipelined_env_emul(locked_model, emul_lib):
    """make_env(pipelined_reset=True): finished episodes restart inside the following steps; the wrappers redraw the env's
    randomizations when its episode ends (before the recipe runs) and reset their per-episode state when the new one starts."""
    from robogym_amd.envs.dactyl.locked import make_env

    env = make_env(constants={"mujoco_substeps": 2, "reset_initial_steps": 1, "n_random_initial_steps": 1, "max_timesteps_per_goal": 3}, batch_size=2, model=locked_model,
                   lib=emul_lib, starting_seed=5, pipelined_reset=True)
    assert env.auto_reset
    obs = env.reset()
    P = env.unwrapped.mujoco_simulation.params
    g0, kp0 = P["gravity"].clone(), obs["actuator_kp"].clone()
    a = torch.randint(0, 11, (2, 20))
    seen_done = seen_start = False
    for t in range(12):
        obs, reward, done, info = env.step(a)
        if bool(done[0]) and not seen_done:
            seen_done = True
            assert not torch.equal(P["gravity"][0], g0[0])               # new physics drawn on the step the episode ended ...
            assert torch.equal(obs["actuator_kp"][0], kp0[0])            # ... while the observation still describes the episode that just ended
            g1 = P["gravity"][0].clone()
        if seen_done and bool(info["episode_started"][0]) and not seen_start:
            seen_start = True
            assert torch.equal(P["gravity"][0], g1) and not torch.equal(obs["actuator_kp"][0], kp0[0])
            assert float(obs["action_ema"][0].abs().max()) == 0.0 and float(obs["previous_action"][0].abs().max()) == 0.0
            assert int(env._steps[0]) == 0
        assert all(torch.isfinite(v.float()).all() for v in obs.values())
    assert seen_done and seen_start
    # a thrown cube: drop penalty and done on the step it is seen, no penalty while the env re-initialises itself
    sim = env.unwrapped.mujoco_simulation
    while bool(info["resetting"].any()):
        obs, reward, done, info = env.step(a)
    q = sim.view(0); q[1, 2] = -0.5; sim.touch_qpos()
    obs, reward, done, info = env.step(a)
    assert bool(done[1]) and float(reward[1, 3]) == -20.0 and bool(info["fell_down"][1]) and float(reward[0, 3]) == 0.0
    obs, reward, done, info = env.step(a)
    assert bool(info["resetting"][1]) and float(reward[1, 3]) == 0.0 and not bool(info["fell_down"][1])


@pytest.mark.gpu
def test_auto_reset_rollout_gpu(locked_model):
    """The default randomized env with in-step resets on the MI355X: 200 steps at B = 512 with goals timing out after 25
    steps — episodes end and restart without any reset() call, every restart redraws that env's physics, the drop penalty is
    paid at most once per episode, nothing non-finite, no status bit."""
    from robogym_amd.envs.dactyl.locked import make_env

    B = 512
    env = make_env(constants={"max_timesteps_per_goal": 25}, batch_size=B, model=locked_model, starting_seed=11, pipelined_reset=True)
    obs = env.reset()
    P = env.unwrapped.mujoco_simulation.params
    g0 = P["gravity"].clone()
    gen = torch.Generator(device="cuda:0"); gen.manual_seed(2)
    ends = torch.zeros(B, dtype=torch.int32, device="cuda:0"); starts = ends.clone(); drops = ends.clone(); bad = 0
    since_start_drops = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    for t in range(200):
        obs, reward, done, info = env.step(torch.randint(0, 11, (B, 20), generator=gen, device="cuda:0"))
        ends += done.to(torch.int32); starts += info["episode_started"].to(torch.int32)
        d = (reward[:, 3] < 0).to(torch.int32)
        since_start_drops = torch.where(info["episode_started"].bool(), torch.zeros_like(d), since_start_drops + d)
        drops += d
        assert int(since_start_drops.max()) <= 1
        bad += int(sum((~torch.isfinite(v.float())).sum() for v in obs.values()))
    assert bad == 0 and int(env.unwrapped.sim_status().max()) == 0
    assert int(ends.sum()) > B and int(starts.sum()) > B // 2 and int(drops.sum()) > 0
    changed = (P["gravity"] != g0).any(dim=1)
    assert bool((changed | (ends == 0)).all())          # every env whose episode ended got new physics


def test_fixed_wrist_matches_the_reference_wrapper(locked_model):
    """constants.fixed_wrist: the reference's FixedWristWrapper, innermost in its stack, against the vectorised stack: the
    actions that reach the env (tests/golden/wrappers_fixed_wrist.npz, tools/gen_golden_wrappers.py)."""
    from robogym_amd.wrappers.dactyl_cube import BatchedDactylCubeWrappers

    g = dict(np.load(os.path.join(G, "wrappers_fixed_wrist.npz")))
    T = len(g["actions"])
    g["script_contacts"] = np.zeros((0, 4)); g["pos_to_ctrl"] = np.zeros((20, 24))
    inner = RandomizedScriptedBatchedEnv(g, locked_model)
    env = BatchedDactylCubeWrappers(inner, randomize=False, fixed_wrist=True)
    inner.t = 0
    env.reset()
    for t in range(T):
        env.step(torch.as_tensor(np.repeat(g["actions"][t][None], inner.batch_size, 0)))
    np.testing.assert_allclose(np.stack(inner.received), g["received_actions"], atol=2e-6)
    u = locked_model.names["actuator"].index("robot0:A_WRJ0")
    assert np.abs(g["received_actions"][:, u] - np.linspace(-1, 1, 11)[g["actions"][:, u]]).max() > 0.1     # the wrapper did override the policy


def _check_rows_went_through_setconst(env, model, envs):
    """Every listed env's dof / body / tendon `_invweight0` rows equal `setconst.set_constants` (host, double precision) of a
    model copy holding THAT env's mass / inertia / armature / site_pos rows.  Stated tolerance: 5e-5 relative (fp32
    tree-sparse factorisation of M at qpos0 on the device)."""
    from robogym_amd.mujoco import setconst

    P = env.unwrapped.mujoco_simulation.params
    worst = 0.0
    for e in envs:
        row = {k: P[k][e].cpu().numpy().astype(np.float64) for k in ("body_mass", "body_inertia", "dof_armature", "site_pos")}
        me = model.copy_with(**row)
        setconst.set_constants(me)
        for k in ("dof_invweight0", "body_invweight0", "tendon_invweight0"):
            got, want = P[k][e].cpu().numpy().astype(np.float64).ravel(), me.arrays[k].ravel()
            np.testing.assert_allclose(got, want, rtol=5e-5, atol=1e-12, err_msg="%s of env %d" % (k, e))
            worst = max(worst, float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-12))))
        # and they are NOT the model's own: the inertia randomisation (0.5-1.5 x per body) really moved them
        assert np.abs(P["dof_invweight0"][e].cpu().numpy() - model.arrays["dof_invweight0"]).max() > 1e-3 * np.abs(model.arrays["dof_invweight0"]).max()
    return worst


def test_default_make_env_recomputes_invweight0_at_reset_emul(locked_model, emul_lib):
    """VERDICT r02 weak 2 / ADVICE: RandomizedBodyInertiaWrapper scales body_inertia per episode, the reference then calls
    mujoco_simulation.set_constants() inside _reset (cube_env.py:346-349).  Here: reset() of the default make_env() runs
    rg_batch_set_constants for the reset envs (device-side mj_setConst); kernel source on the emulation harness."""
    from robogym_amd.envs.dactyl.locked import LockedEnvConstants, make_env

    env = make_env(batch_size=2, device="cpu", model=locked_model, starting_seed=5, lib=emul_lib,
                   constants=dict(mujoco_substeps=1, reset_initial_steps=1, n_random_initial_steps=1, max_pose_resets=1))
    env.reset()
    worst = _check_rows_went_through_setconst(env, locked_model, [0, 1])
    print("device mj_setConst vs host setconst (emulation): worst relative deviation %.2e" % worst)
    before = env.unwrapped.mujoco_simulation.params["dof_invweight0"].clone()
    env.reset(torch.tensor([True, False]))
    after = env.unwrapped.mujoco_simulation.params["dof_invweight0"]
    assert not torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])     # masked: only the reset env was redrawn and refreshed
    _check_rows_went_through_setconst(env, locked_model, [0])


@pytest.mark.gpu
def test_default_make_env_recomputes_invweight0_at_reset_gpu(locked_model):
    """The same on the MI355X at B = 256 (8 sampled envs), after reset() and after a masked reset; and with the pipelined reset
    (wrapper auto_reset): rows of envs whose episode ended are redrawn AND refreshed before their recipe runs."""
    from robogym_amd.envs.dactyl.locked import make_env

    env = make_env(batch_size=256, model=locked_model, starting_seed=6)
    env.reset()
    worst = _check_rows_went_through_setconst(env, locked_model, [0, 1, 37, 100, 255])
    m = torch.zeros(256, dtype=torch.bool); m[37] = True
    env.reset(m)
    worst = max(worst, _check_rows_went_through_setconst(env, locked_model, [37, 38]))
    print("device mj_setConst vs host setconst (MI355X): worst relative deviation %.2e" % worst)
    env = make_env(batch_size=64, model=locked_model, starting_seed=7, pipelined_reset=True, constants=dict(max_timesteps_per_goal=4))
    env.reset()
    gen = torch.Generator(); gen.manual_seed(0)
    ended = torch.zeros(64, dtype=torch.bool, device="cuda:0")
    for _ in range(12):
        obs, reward, done, info = env.step(torch.randint(0, 11, (64, 20), generator=gen))
        ended |= done
    idx = [int(i) for i in torch.nonzero(ended).flatten()[:4]]
    assert len(idx) >= 2
    _check_rows_went_through_setconst(env, locked_model, idx)
    assert int(env.unwrapped.sim_status().max()) == 0


# ------------------------------------------------------------------------------------------------ the quaternion helpers the stack leans on
def _quat_helpers_match_the_component_formulas(device):
    """`rotation.quat_mul` forms the Hamilton product from one outer product, one gather and three sums (six tensor kernels instead of 29: the wrapper stack is
    launch latency).  The products and the order of the sums are those of the reference's component formula (utils/rotation.py:234-257 `quat_mul`), so it is
    BIT-identical to it -- also with the conjugate folded into its sign table (`quat_difference`, rotation.py:271) and for signed zeros in `quat_normalize`
    (rotation.py:281-286)."""
    from robogym_amd.utils import rotation

    def formula(q0, q1):
        w0, x0, y0, z0 = q0.unbind(-1); w1, x1, y1, z1 = q1.unbind(-1)
        return torch.stack([w0 * w1 - x0 * x1 - y0 * y1 - z0 * z1, w0 * x1 + x0 * w1 + y0 * z1 - z0 * y1,
                            w0 * y1 + y0 * w1 + z0 * x1 - x0 * z1, w0 * z1 + z0 * w1 + x0 * y1 - y0 * x1], dim=-1)

    def normalize(q):
        return q * torch.where(q[..., :1] < 0, -torch.ones_like(q[..., :1]), torch.ones_like(q[..., :1]))

    gen = torch.Generator(device=device); gen.manual_seed(3)
    for dtype, bits in ((torch.float32, torch.int32), (torch.float64, torch.int64)):
        a = torch.randn((4096, 4), generator=gen, device=device, dtype=dtype)
        b = torch.randn((4096, 4), generator=gen, device=device, dtype=dtype)
        a[:8, 0] = 0.0; a[4:8, 0] = -0.0
        same = lambda x, y: torch.equal(x.contiguous().view(bits), y.contiguous().view(bits))
        assert same(rotation.quat_mul(a, b), formula(a, b))
        assert same(rotation.quat_mul(a[:3, None], b[None, :5]), formula(*torch.broadcast_tensors(a[:3, None], b[None, :5])))
        assert same(rotation.quat_difference(a, b), normalize(formula(a, rotation.quat_conjugate(b))))
        assert same(rotation.quat_normalize(a), normalize(a))


def test_quat_helpers_match_the_component_formulas():
    _quat_helpers_match_the_component_formulas("cpu")


@pytest.mark.gpu
def test_quat_helpers_match_the_component_formulas_gpu():
    _quat_helpers_match_the_component_formulas("cuda:0")


# ------------------------------------------------------------------------------------------------ the stack's launch count and its draw blocks
_VIEW_OPS = {"view", "select", "slice", "unsqueeze", "squeeze", "expand", "reshape", "_unsafe_view", "as_strided", "t", "transpose", "permute", "unbind", "alias",
             "detach", "_reshape_alias", "split", "split_with_sizes", "unfold"}


def test_default_wrapper_step_stays_under_its_kernel_budget_emul(locked_model, emul_lib):
    """On the GPU every tensor op of the wrapper stack is a ~4 us kernel queued behind the physics launch (profiles/r06_wrapped_breakdown.txt): round 6 brought the
    default make_env() step from ~370 to ~200 of them.  The count is a property of the Python code, so it is held here (aten ops that are not views, counted by a
    dispatch mode around one step on the CPU): a change that brings per-key loops back shows up as a failure, not as a slower bench line a round later."""
    from torch.utils._python_dispatch import TorchDispatchMode
    from robogym_amd.envs.dactyl.locked import make_env

    counts = {}

    class Count(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.__name__.split(".")[0]
            if name not in _VIEW_OPS:
                counts[name] = counts.get(name, 0) + 1
            return func(*args, **(kwargs or {}))

    quick = dict(mujoco_substeps=1, reset_initial_steps=1, n_random_initial_steps=1, max_pose_resets=1)      # (the physics is not what is counted)
    for kw, budget in ((dict(constants=dict(quick)), 215), (dict(constants=dict(quick, randomize=False)), 110)):
        env = make_env(batch_size=2, device="cpu", model=locked_model, starting_seed=1, lib=emul_lib, **kw)
        env.reset()
        gen = torch.Generator(); gen.manual_seed(0)
        env.step(torch.randint(0, 11, (2, 20), generator=gen))
        counts.clear()
        with Count():
            env.step(torch.randint(0, 11, (2, 20), generator=gen))
        total = sum(counts.values())
        print("tensor kernels per wrapped step (randomize %s): %d" % (kw["constants"].get("randomize", True), total), sorted(counts.items(), key=lambda kv: -kv[1])[:8])
        assert total <= budget, (total, counts)


def test_torch_draws_blocks():
    """TorchDraws inside a step: the small draws are disjoint column slices of one uniform and one normal block (exponentials: of the uniform block's image, on the
    same cursor, so no number is used twice); what does not fit, and everything outside a step, is drawn on its own."""
    from robogym_amd.wrappers.dactyl_cube import TorchDraws

    gen = torch.Generator(); gen.manual_seed(4)
    D = TorchDraws(gen, 6, "cpu")
    outside = D.uniform(0.0, 1.0, (3,))
    assert outside.shape == (6, 3) and outside.is_contiguous()
    D.begin_step()
    ublock, nblock = D._pool["u"][0], D._pool["n"][0]
    a = D.random_sample((5,)); e = D.exponential(2.0, (4,)); b = D.uniform(-1.0, 1.0, (3,)); n1 = D.randn((20,)); n2 = D.randn((3,)); c = D.uniform(0.0, 1.0)
    assert torch.equal(a, ublock[:, 0:5]) and torch.equal(e, -torch.log1p(-ublock[:, 5:9]) * 2.0) and torch.equal(b, -1.0 + 2.0 * ublock[:, 9:12]) and torch.equal(c, ublock[:, 12])
    assert torch.equal(n1, nblock[:, :20]) and torch.equal(n2, nblock[:, 20:23]) and (e > 0).all() and c.shape == (6,)
    big = D.randn((TorchDraws.N_POOL,))            # does not fit what is left of the block: drawn on its own, the cursor stays
    assert big.shape == (6, TorchDraws.N_POOL) and D._pool["n"][1] == 23
    D.end_step()
    assert D.randn((2,)).shape == (6, 2) and not D._pool
