"""The plain bench.py line and --dump-outputs on hardware: the line carries the contract fields and nothing that needs runs of its
own (those are --full's), `steps` timed steps, and the arrays of the last timed step land as float32 .npy files within 64 MB."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["unit"] == "videos/s" and d["higher_is_better"] is True and d["dtype"] == "bf16" and d["steps"] == 7 and d["warmup"] == 2
    assert d["ms_per_step"] > 0 and math.isclose(d["value"], (128 + 74) / (d["ms_per_step"] * 1e-3), rel_tol=1e-6)
    assert d["config"]["finite"] is True
    assert not {"roofline", "cpu_baseline", "other_arithmetic", "configs", "variants", "value_fresh_batch"} & set(d)
    files = sorted(os.listdir(out))
    arrays = {f[:-4]: np.load(out / f) for f in files}
    assert all(f.endswith(".npy") for f in files) and all(a.dtype == np.float32 for a in arrays.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 10 ** 6
    assert arrays["out"].shape == (128 + 74, 12) and arrays["losses"].shape == (6,)
    assert arrays["param.fc_feature_shared_source.weight"].shape == (512, 2048)
    assert all(np.isfinite(a).all() for a in arrays.values())
