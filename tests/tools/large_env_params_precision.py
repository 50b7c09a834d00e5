"""dactyl/full_perpendicular with per-env rows: the comparison of tests/tools/large_precision_report.py (the oracle built in FLOAT against the same source in DOUBLE,
re-synchronised env.steps) on the variant models of tests/test_large_env_params.py -- the model's own values, timestep x 0.75 / 1.2, a wrench on the cube and a
fingertip, cube scale 0.95 / 1.05 with shifted sites -- over the 10 env.steps and the action stream of test_full_cube_rows_resync_env_steps_gpu.  Writes the spread
per variant to profiles/large_env_params_precision.txt and tests/golden/large_env_params_spread.json, which that test reads: a variant whose own spread exceeds the
default model's is held to 3 x its own spread (the rule of tests/golden/ycb_pair_spread.json), every other one to the bounds of test_large_model_resync_env_steps_gpu.
    python tests/tools/large_env_params_precision.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle.rg_oracle import OracleSim  # noqa: E402
from robogym_amd.envs.dactyl.full_perpendicular import FINGERTIP_SITE_NAMES, REFERENCE_SITE_NAMES, load_full_perpendicular_model  # noqa: E402
from robogym_amd.mujoco import setconst  # noqa: E402
from robogym_amd.mujoco.big_tables import derive_big_tables  # noqa: E402
from robogym_amd.mujoco.model_blob import pack_model  # noqa: E402
from tests import test_large_env_params as T  # noqa: E402
from tests.test_large_model import OracleFullCube  # noqa: E402

m = load_full_perpendicular_model(); setconst.set_constants(m); derive_big_tables(m)
A, names = m.arrays, m.names["joint"]
hand_j = [j for j, n in enumerate(names) if n.startswith("robot0:")]
hq = np.array([A["jnt_qposadr"][j] for j in hand_j])
P = np.zeros((20, len(hand_j)))
for u in range(20):
    if A["actuator_trntype"][u] == 0:
        P[u, hand_j.index(int(A["actuator_trnid"][u]))] = 1
    else:
        t = int(A["actuator_trnid"][u])
        for w in range(A["tendon_adr"][t], A["tendon_adr"][t] + A["tendon_num"][t]):
            P[u, hand_j.index(int(A["wrap_objid"][w]))] = 1
non_target = np.array([i for j, n in enumerate(names) if not n.startswith("target:") for i in range(A["jnt_qposadr"][j], A["jnt_qposadr"][j] + {0: 7, 1: 4, 2: 1, 3: 1}[int(A["jnt_type"][j])])])
ts0 = float(np.asarray(A["opt_timestep"]).reshape(-1)[0])


class _Sites:
    tip_sites = [m.names["site"].index("robot0:" + s) for s in FINGERTIP_SITE_NAMES]
    ref_sites = [m.names["site"].index("robot0:" + s) for s in REFERENCE_SITE_NAMES]


shift, wind = T._site_shift(m, _Sites), T._wind(m)
out, lines = {}, []
for ts_factor, scale in ((0.75, 0.95), (1.2, 1.05)):
    acts = np.random.RandomState(3).uniform(-1, 1, (10, 4, 20))          # the action stream of the GPU test: one draw of (4, 20) per step
    for e, kind in enumerate(T.FULL_ROWS):
        key = kind if kind in ("model", "wind") else "%s:%g" % (kind, ts_factor if kind == "timestep" else scale)
        if key in out:
            continue
        model = m.copy_with(opt_timestep=[ts0 * ts_factor]) if kind == "timestep" else (T._scaled_cube_model(m, scale, shift) if kind == "scale+sites" else m)
        o64, o32 = OracleFullCube(model, P, hq), OracleFullCube(model, P, hq)
        o32.sim = OracleSim(pack_model(model), f32=True)
        o64.hold_pose()
        for _ in range(60):
            o64.sim.step()
        if kind == "wind":
            o64.sim.xfrc_applied[:] = wind.reshape(-1); o32.sim.xfrc_applied[:] = wind.reshape(-1)
        E = []
        for step in range(10):
            st = o64.state_f32()
            s = o32.sim
            s.qpos[:] = st["qpos"]; s.qvel[:] = st["qvel"]; s.pid[:] = st["pid"]; s.qacc_warmstart[:] = st["warm"]; s.ctrl[:] = st["ctrl"]
            o32.env_step(acts[step, e]); o64.env_step(acts[step, e])
            d = np.abs(o32.sim.qpos.astype(np.float64) - o64.sim.qpos)
            E.append((d[non_target].max(), d[hq].max()))
        E = np.array(E)
        out[key] = dict(median=float(np.median(E[:, 0])), p90=float(np.percentile(E[:, 0], 90)), max=float(E[:, 0].max()), hand=float(np.median(E[:, 1])))
        lines.append("  %-18s non-target qpos median %.2e p90 %.2e max %.2e | hand joints median %.2e" % (key, out[key]["median"], out[key]["p90"], out[key]["max"], out[key]["hand"]))
        print(lines[-1], flush=True)
base = dict(median=1e-3, p90=1e-2, max=5e-2, hand=2e-5)
with open(os.path.join(ROOT, "profiles", "large_env_params_precision.txt"), "w") as f:
    f.write("dactyl/full_perpendicular with per-env rows: oracle FLOAT against oracle DOUBLE (tests/tools/large_env_params_precision.py), 10 re-synchronised env.steps of iid\n"
            "U(-1, 1) relative actions per variant model of tests/test_large_env_params.py (the protocol and actions of test_full_cube_rows_resync_env_steps_gpu).\n"
            "Rule: a variant whose own spread exceeds the default model's ('model') is held to 3 x its own spread in that test, every other figure to the bounds of\n"
            "test_large_model_resync_env_steps_gpu (median 1e-3, p90 1e-2, max 5e-2, hand joints median 2e-5).\n"
            "These figures are CPU-only (both sides are the oracle), from ONE action seed and 10 env.steps per variant: a thin basis, taken as the issue states the rule.\n\n" + "\n".join(lines) + "\n\nbounds that follow:\n")
    for key, v in out.items():
        f.write("  %-18s %s\n" % (key, {k: (3.0 * v[k] if v[k] > out["model"][k] else base[k]) for k in base}))
with open(os.path.join(ROOT, "tests", "golden", "large_env_params_spread.json"), "w") as f:
    json.dump({"what": "float-vs-double oracle spread per variant model, tests/tools/large_env_params_precision.py; bound = 3 x own spread where it exceeds the default model's",
               "variants": out}, f, indent=1)
