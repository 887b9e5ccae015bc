"""bench.py end to end on one GPU (run with -m gpu), at batch 16: a plain run reports the headline alone and still writes both
sample sets; --full adds the roofline.  The bf16 samples a plain run writes untimed equal the last timed step of a bf16 run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "16"]


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_and_full_run(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert plain["roofline"] is None and plain["cpu_baseline"] is None and "secondary" not in plain
    assert plain["steps"] == 2 and plain["warmup"] == 1 and plain["value"] > 0 and plain["ms_per_step"] > 0
    samples = {n: np.load(tmp_path / "plain" / f"{n}.npy") for n in ("samples", "samples_bf16")}
    for n, a in samples.items():
        assert a.dtype == np.float32 and a.shape == (16, 3, 32, 32) and np.isfinite(a).all(), n
    assert not np.array_equal(samples["samples"], samples["samples_bf16"])

    full = _bench("--full", "--dtype", "bf16", "--no-cpu-baseline", "--no-secondary", "--dump-outputs", str(tmp_path / "full"))
    assert full["dtype"] == "bf16" and full["cpu_baseline"] is None and "secondary" not in full
    roof = full["roofline"]
    assert isinstance(roof, dict) and roof["launches"] > 0 and roof["achieved"] > 0
    assert np.array_equal(np.load(tmp_path / "full" / "samples.npy"), samples["samples_bf16"])
