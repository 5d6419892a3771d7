"""bench.py on the GPU at a small size: a plain run times --steps steps and carries the headline fields only, --full
adds the secondary figures, and --dump-outputs writes what the last timed step computed -- the same arrays in both
runs (same seeds, same timed path).  -m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, K, W = 4, 5, 2
ARGS = ["--gpus", "1", "--batch", str(B), "--prompt", "40", "--context", "160", "--steps", str(K), "--warmup", str(W)]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
SECONDARY = ("roofline", "kv_pack", "kernels")


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_and_full_runs_and_their_dumped_outputs(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-codec", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for r in (plain, full):
        assert all(k in r for k in HEADLINE), r
        assert r["steps"] == K and r["warmup"] == W and r["unit"] == "codec_tokens/s" and r["dtype"] == "bf16"
        assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(B * 8 * 1e3 / r["ms_per_step"], rel=1e-9)
    assert not any(k in plain for k in SECONDARY)
    assert all(k in full for k in SECONDARY) and full["kernels"]["attn_scores_kernel"]["launches"] > 0

    shapes = {"ids": (B, 8), "logits_ch0": (B, 152697), "logits_ch1_7": (7, B, 1025)}
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(n + ".npy" for n in shapes)
    total = 0
    for name, shape in shapes.items():
        a, b = (np.load(tmp_path / d / (name + ".npy")) for d in ("plain", "full"))
        assert a.dtype in (np.float32, np.float64) and a.shape == shape, (name, a.dtype, a.shape)
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    ids = np.load(tmp_path / "plain" / "ids.npy")
    assert np.array_equal(ids, np.round(ids)) and (ids >= 0).all()
    l0 = np.load(tmp_path / "plain" / "logits_ch0.npy")
    assert np.isfinite(l0).any(axis=1).all()
