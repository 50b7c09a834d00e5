"""bench.py's plain line and `--dump-outputs`, on CPU: the headline code path with the kernel source on the emulation harness (RG_BENCH_EMUL_LIB test
hook), one rank, a batch of 2.  A plain run carries the headline fields and nothing that `--full` adds; two runs with the same arguments write the same
arrays."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["RG_BENCH_EMUL_LIB"] = os.path.join(ROOT, "tests", "emul", "librgstep_emul.so")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--dump-outputs", str(out_dir), *extra]
    out = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.split("\n") if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_bench_plain_line_and_dumped_outputs_are_reproducible(emul_lib, tmp_path):
    r = _bench(tmp_path / "a")
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0
    assert r["unit"] == "env-steps/s" and r["higher_is_better"] is True and r["dtype"] == "f32" and "dactyl/locked" in r["metric"]
    assert "cpu_baseline" not in r and "secondary" not in r and r["config"]["long_window"] is None
    _bench(tmp_path / "b")
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"obs_qpos.npy", "obs_cube_quat.npy", "reward.npy", "done.npy", "info_goal_dist_cube_quat.npy"} <= set(names), names
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.shape[0] == 2, (n, a.dtype, a.shape)
        np.testing.assert_array_equal(a, b, err_msg=n)
    assert np.abs(np.load(tmp_path / "a" / "obs_qpos.npy")).max() > 0
