"""A plain `bench.py --gpus 1 --steps K --warmup W` run: it times exactly K steps, prints one JSON line
with the headline fields and none of the measurements that take runs of their own (those are behind
--full), and --dump-outputs writes the last timed step's loss, parameters and gradients."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--workload", "n2v", "--feed", "fixed", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "ray-samples/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and d["dtype"] == "fp32"
    assert abs(d["value"] - 4096 * 64 / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    # every timed step launched the fused forward once: the timed region is exactly --steps steps
    assert d["kernels"]["mlp_fused_fwd"]["launches_per_step"] == 1.0
    assert not {"cpu_baseline", "frame_render", "roofline_hbm_frame"} & set(d)
    files = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert np.float32(files["loss"][0]) == np.float32(d["final_loss"])
    params = [n for n in files if n.startswith("param.")]
    assert params and all("grad." + n[6:] in files for n in params)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
