"""GPU: bench.py's plain run (no --full) on a small MSM -- the line holds the headline fields and nothing that needs runs
of its own, --steps sets the number of timed steps, and --dump-outputs writes the last timed result.  The same arguments
with --full check that result against the oracle inside bench.py; its hash must be the dumped result's, and the dump must
be the same in both runs (inputs depend on the arguments only)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--lg", "16", "--warmup", "1"] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dump(libs, tmp_path):
    d = _run(["--steps", "3", "--dump-outputs", str(tmp_path / "plain")])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["unit"] == "points/s" and d["higher_is_better"] is True and d["dtype"] == "u32"
    assert d["ms_per_step"] > 0 and abs(d["value"] - (1 << 16) / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    for k in ("parity", "ntt", "extras", "cpu_baseline"):
        assert d[k] is None, k
    xy = np.load(tmp_path / "plain" / "msm_affine.npy")
    assert xy.dtype == np.float64 and xy.shape == (2, 12)
    assert (xy == np.floor(xy)).all() and (xy >= 0).all() and (xy < 2.0 ** 32).all() and xy.any()

    f = _run(["--steps", "2", "--full", "--no-ntt", "--no-extras", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full")])
    assert f["steps"] == 2 and f["parity"]["timed_msm_equals_oracle"] is True
    xy_full = np.load(tmp_path / "full" / "msm_affine.npy")
    assert (xy_full == xy).all()
    assert f["parity"]["result_affine_sha256"] == hashlib.sha256(xy.astype("<u4").tobytes()).hexdigest()
