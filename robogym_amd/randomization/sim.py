"""Batched simulation randomizers: the reference's `robogym/randomization/sim.py` (GravityRandomizer :115-133,
PidRandomizer :136-160, JointMarginRandomizer :163-180, GeomSolimpRandomizer :183-268, GeomSolrefRandomizer :271-315,
GenericSimRandomizer :317-589) and the dactyl physics wrappers
(`wrappers/randomizations.py`: RandomizedBodyInertiaWrapper :72-92, RandomizedFrictionBaseWrapper :95-173,
RandomizedGravityWrapper :176-191, RandomizedDampingWrapper :562-590, RandomizedKpWrapper :720-746) acting on the
per-env model parameter rows of the HIP stepper instead of on one `sim.model`.

The reference writes `sim.model.<field>` of ONE env before `reset()`; here `sim.params[<field>]` is a `[B, ...]` tensor view
into the rows the kernel reads (include/rgstep.h RG_F_ENVPRM), a randomizer draws for the envs selected by `mask` (the envs
being reset) and writes them with ordinary tensor ops: no host loop, no synchronisation.  The per-episode formulas are the
reference's; what is folded in is the ADR parameter plumbing (`_randomizer_param_values` is a constructor argument here).
Mass / inertia / armature changes need the mj_setConst outputs recomputed (`*_invweight0`: regulariser scales of the
constraint rows); `refresh_constants` does that on the device through the simulation's `set_constants(mask)` (rg_setconst_kernel on
the hand stepper, rb_setconst_kernel on `LargeModelSimulation` / `FullPerpendicularSimulation`): no host loop, no synchronisation.
"""
from typing import Optional, Sequence

import numpy as np
import torch

PID_GAIN_PARAMS = ["pid_kp", "pid_ti", "pid_imax_clamp", "pid_td", "pid_dsmooth", "pid_error_deadband"]   # mujoco/constants.py:35-52


class SimulationRandomizer:
    def __init__(self, name: str):
        self.name = name
        self._initial = None

    def prepare(self, sim):
        """Whatever `randomize` would have to upload from the host, made now: afterwards a call of `randomize` waits for nothing."""

    def _field(self, sim) -> torch.Tensor:
        raise NotImplementedError

    def _sample(self, init: torch.Tensor, gen: torch.Generator) -> torch.Tensor:
        raise NotImplementedError

    def randomize(self, sim, gen: torch.Generator, mask: Optional[torch.Tensor] = None, initial: Optional[torch.Tensor] = None):
        """Draw new values for the envs in `mask` (default: all) from the model's initial values -- or from `initial`, per-env values of the field's own shape
        (the rearrange envs' per-object materials: the rows of a world rebuilt with the episode's materials)."""
        f = self._field(sim)
        if self._initial is None:
            self._initial = f[0].clone()          # every row starts as the model's own values
        new = self._sample(self._initial.expand_as(f) if initial is None else initial, gen)
        if mask is None:
            f.copy_(new)
        else:
            f.copy_(torch.where(mask.reshape((-1,) + (1,) * (f.dim() - 1)), new, f))


class GravityRandomizer(SimulationRandomizer):
    """sim.py:115-133: gravity + (exp(p) - 1) * random unit vector."""

    def __init__(self, param: float = 0.0):
        super().__init__("gravity")
        self.param = param

    def _field(self, sim):
        return sim.params["gravity"]

    def _sample(self, init, gen):
        d = torch.randn(init.shape, generator=gen, device=init.device)
        d = d / d.norm(dim=-1, keepdim=True)
        return init + d * float(np.exp(self.param) - 1.0)


class PidRandomizer(SimulationRandomizer):
    """sim.py:136-160: actuator_gainprm[:, idx] * exp(N(mean, |std|)) per actuator."""

    def __init__(self, field_name: str, mean: float = 0.0, std: float = 0.0):
        super().__init__(field_name)
        self.idx, self.mean, self.std = PID_GAIN_PARAMS.index(field_name), mean, abs(std)

    def _field(self, sim):
        return sim.params["actuator_gainprm"][:, :, self.idx]

    def _sample(self, init, gen):
        return init * torch.exp(self.mean + self.std * torch.randn(init.shape, generator=gen, device=init.device))


class GenericSimRandomizer(SimulationRandomizer):
    """sim.py:317-589 for the modes the dactyl / rearrange randomizer lists use (base.py:1008-1092).  `ids` restricts the
    randomizer to a subset of rows (the reference's geom_ / body_ / dof_jnt_ / jnt_ prefixes, resolved by the caller with
    the model's name lists)."""

    def __init__(self, name: str, field_name: str, apply_mode: str = "uncoupled_mean_variance", param=(0.0, 0.0), coef: float = 1.0,
                 ids: Optional[Sequence[int]] = None, positive_only: bool = False):
        super().__init__(name)
        self.field_name, self.mode, self.coef, self.ids, self.positive_only = field_name, apply_mode, coef, ids, positive_only
        self.param = np.atleast_1d(np.asarray(param, dtype=np.float64)) * coef
        self._sel = None

    def _row_mask(self, f):
        """[rows] bool: the rows `ids` names, on f's device; made once (the upload of a host list waits for the device)"""
        if self._sel is None or self._sel.device != f.device or self._sel.shape[0] != f.shape[1]:
            sel = torch.zeros(f.shape[1], dtype=torch.bool, device=f.device)
            sel[torch.as_tensor(list(self.ids), device=f.device)] = True
            self._sel = sel
        return self._sel

    def prepare(self, sim):
        if self.ids is not None:
            self._row_mask(sim.params[self.field_name])

    def _field(self, sim):
        f = sim.params[self.field_name]
        return f if self.ids is None else _RowSubset(f, self.ids)

    def randomize(self, sim, gen, mask=None, initial=None):
        f = sim.params[self.field_name]
        if self._initial is None:
            self._initial = f[0].clone()
        init = self._initial.expand_as(f) if initial is None else initial
        new = self._sample(init, gen)
        if self.positive_only:
            new = new.clamp(min=0.0)
        if self.ids is not None:
            new = torch.where(self._row_mask(f).reshape((1, -1) + (1,) * (f.dim() - 2)), new, f)
        if mask is not None:
            new = torch.where(mask.reshape((-1,) + (1,) * (f.dim() - 1)), new, f)
        f.copy_(new)

    def _sample(self, init, gen):
        p, dev = self.param, init.device
        n = lambda: torch.randn(init.shape, generator=gen, device=dev)
        u = lambda: torch.rand(init.shape, generator=gen, device=dev)
        m = self.mode
        if m == "coupled":
            return init * float(np.exp(p[0]))
        if m == "uncoupled":
            return init * torch.exp((p[0] + n()) * abs(p[0]))
        if m == "ranges":
            lo, hi = min(0.0, -p[0]), max(0.0, p[1])
            return init * torch.exp(lo + (hi - lo) * u())
        if m == "variance":
            return init * torch.exp(n() * abs(p[0]))
        if m == "variance_additive":
            return init + n() * float(np.exp(abs(p[0])) - 1.0)
        if m == "variance_mean_additive":
            return init + (float(np.exp(p[0]) - 1.0) + n() * float(np.exp(abs(p[1])) - 1.0)).abs()
        if m == "coupled_mean_variance":
            return init * torch.exp(p[0] + abs(p[0]) * n())
        if m == "uncoupled_mean_variance":
            return init * torch.exp(p[0] + abs(p[1]) * n())
        if m == "max_additive":
            return init + u() * float(np.exp(abs(p[0])) - 1.0)
        raise ValueError("Invalid mode: {}".format(m))


class JointMarginRandomizer(SimulationRandomizer):
    """sim.py:163-180: jnt_margin + U(0, 1) * (exp(p) - 1) * 0.15 per joint."""

    def __init__(self, param: float = 0.0):
        super().__init__("jnt_margin")
        self.param = param

    def _field(self, sim):
        return sim.params["jnt_margin"]

    def _sample(self, init, gen):
        return init + torch.rand(init.shape, generator=gen, device=init.device) * float(np.exp(self.param) - 1.0) * 0.15


class GeomSolimpRandomizer(SimulationRandomizer):
    """sim.py:183-268: (dmin, dmax, width) of every geom.  dmax = 1 - (1 - dmax0) exp(N(dmax_mean, dmax_std)) clipped to `drange`;
    dmin = clip(dmax - (dmax0 - dmin0) exp(N(delta_mean, delta_std))); width = width0 exp(N(width_mean, width_std)).
    `param` = [dmax_mean, dmax_std, delta_mean, delta_std, width_mean, width_std]."""

    def __init__(self, param=(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), drange=(0.5, 0.99)):
        super().__init__("geom_solimp")
        self.param, self.drange = [float(v) for v in param], (float(drange[0]), float(drange[1]))
        assert len(self.param) == 6 and self.param[1] >= 0 and self.param[3] >= 0 and self.param[5] >= 0

    def _field(self, sim):
        return sim.params["geom_solimp"]

    def _sample(self, init, gen):
        p, (lo, hi) = self.param, self.drange
        n = lambda: torch.randn(init.shape[:-1], generator=gen, device=init.device)
        dmax = (1.0 - (1.0 - init[..., 1]) * torch.exp(p[0] + p[1] * n())).clamp(lo, hi)
        delta = (init[..., 1] - init[..., 0]) * torch.exp(p[2] + p[3] * n())
        dmin = (dmax - delta).clamp(lo, hi)
        width = init[..., 2] * torch.exp(p[4] + p[5] * n())
        out = init.clone()
        out[..., 0], out[..., 1], out[..., 2] = dmin, dmax, width
        return out


class GeomSolrefRandomizer(SimulationRandomizer):
    """sim.py:271-315: timeconst * exp(N(timeconst_mean, timeconst_std)), dampratio * exp(N(dampratio_mean, dampratio_std)) per geom."""

    def __init__(self, param=(0.0, 0.0, 0.0, 0.0)):
        super().__init__("geom_solref")
        self.param = [float(v) for v in param]
        assert len(self.param) == 4 and self.param[1] >= 0 and self.param[3] >= 0

    def _field(self, sim):
        return sim.params["geom_solref"]

    def _sample(self, init, gen):
        p = self.param
        n = lambda: torch.randn(init.shape[:-1], generator=gen, device=init.device)
        out = init.clone()
        out[..., 0] = init[..., 0] * torch.exp(p[0] + p[1] * n())
        out[..., 1] = init[..., 1] * torch.exp(p[2] + p[3] * n())
        return out


class _RowSubset:   # (placeholder type for _field(); GenericSimRandomizer.randomize handles subsets itself)
    def __init__(self, f, ids):
        self.f, self.ids = f, ids


def refresh_constants(sim, rows: Optional[Sequence[int]] = None):
    """mj_setConst for the envs whose mass / inertia / armature rows were changed (the reference calls
    `mujoco_simulation.set_constants()` in `_reset`, cube_env.py:349): dof / body / tendon `_invweight0` recomputed ON THE
    DEVICE from each env's own row (`sim.set_constants`: rg_setconst_kernel, or rb_setconst_kernel on the large-model stepper); no host loop, no
    synchronisation."""
    if rows is None:
        sim.set_constants()
        return
    mask = torch.zeros(sim.batch_size, dtype=torch.int32, device=sim.device)
    mask[torch.as_tensor(list(rows), dtype=torch.long, device=sim.device)] = 1
    sim.set_constants(mask)
