"""GPU: a plain bench.py run (no --full) times its steps and prints the headline line only, and
--dump-outputs writes what the last timed step computed: logits and loss that belong together,
a gradient and an updated value for every parameter."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dump(cuda, tmp_path):
    import bench

    B = 8
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--graphs-per-gpu", str(B), "--dump-outputs",
                        str(tmp_path / "out")], capture_output=True, text=True, timeout=120,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["warmup"] == 1 and out["unit"] == "graphs/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement (both rounded in the line)
    assert out["value"] == pytest.approx(B / (out["ms_per_step"] * 1e-3), rel=1e-2)
    for key in ("roofline", "roofline_next", "entries", "knn_graph", "cpu_baseline"):
        assert key not in out  # --full only

    wl = bench.WORKLOADS["c2"]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    params = [n for n, _ in bench.build_model(wl).named_parameters()]
    assert set(got) == {"logits", "loss"} | {f"{k}.{n}" for k in ("grad", "param") for n in params}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["logits"].shape == (B, wl["classes"])
    # the loss of the dumped logits on the run's own (seeded) labels: fp32 CE over 5 classes
    y = bench.make_batch(wl, B, seed=100).y
    want = torch.nn.functional.cross_entropy(torch.from_numpy(got["logits"]).double(), y)
    assert abs(float(got["loss"]) - want.item()) <= 1e-5
    # four Adam steps (1 warmup + 3 timed; the capture's own warmups add more) moved the weights
    init = dict(bench.build_model(wl).named_parameters())
    assert any(not np.array_equal(got[f"param.{n}"], init[n].detach().numpy()) for n in params)
    assert any(np.abs(got[f"grad.{n}"]).max() > 0 for n in params)
