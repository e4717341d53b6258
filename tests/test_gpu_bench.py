"""bench.py on one GPU: a plain run times --steps steps and carries the headline fields only, --dump-outputs writes what the last timed
step computed - in the engine's reproducible mode, so that two runs with the same arguments write bit-identical outputs - and --full
adds the measurements beyond the headline without changing the timed steps."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "layouts", "batch_handover")


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "toy-tiny",
           "--dump-outputs", str(out_dir), *extra]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_dumps_the_last_timed_step_and_full_adds_the_rest(tmp_path):
    plain = _bench(tmp_path / "plain")
    assert all(k in plain for k in HEADLINE) and plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert plain["unit"] == "graph-tokens/s" and plain["higher_is_better"] is True and plain["dtype"] == "bf16"
    assert not any(k in plain for k in FULL_ONLY + ("cpu_baseline", "per_sample_kernels"))
    assert plain["config"]["reproducible_mode"] is True
    names = {"loss", "grad_norm", "master_weights", "grads"}
    files = {f[:-4]: np.load(tmp_path / "plain" / f) for f in os.listdir(tmp_path / "plain")}
    assert set(files) == names
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(os.path.getsize(tmp_path / "plain" / (n + ".npy")) for n in names) <= 64 << 20
    assert abs(float(files["loss"][0]) - plain["smtp_loss"]) <= 1e-6 * abs(plain["smtp_loss"])
    assert float(files["grad_norm"][0]) > 0 and np.abs(files["grads"]).max() > 0

    full = _bench(tmp_path / "full", "--full", "--no-cpu-baseline")
    assert all(k in full for k in HEADLINE + FULL_ONLY) and full["steps"] == 3
    again = {n: np.load(tmp_path / "full" / (n + ".npy")) for n in names}
    # another process, the same timed steps on the same inputs (the extra measurements of --full all run after the dump): bit-identical
    for n in names:
        assert np.array_equal(again[n], files[n]), f"{n}.npy differs between two runs with the same arguments"
