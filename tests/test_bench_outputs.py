"""bench.py --dump-outputs and the plain / --full split: the dump holds the last timed step's results
as float32 .npy files within its size budget (a larger array as the same seeded sample every run), a
plain run reports the timed steps alone, and two runs with the same arguments start from identical
inputs and end at the same results."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_samples_large_arrays_the_same_way_every_run(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 3 * 4 * 100)      # 3 arrays: 100 elements each
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    named = [("small", torch.tensor([[1, 2], [3, 4]])), ("big", big), ("half", torch.ones(7, dtype=torch.bfloat16))]
    bench.dump_outputs(str(tmp_path / "a"), named)
    bench.dump_outputs(str(tmp_path / "b"), named)
    a = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    b = {f: np.load(tmp_path / "b" / f) for f in sorted(os.listdir(tmp_path / "b"))}
    assert list(a) == ["big.npy", "half.npy", "small.npy"] == list(b)
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["small.npy"].tolist() == [[1, 2], [3, 4]] and a["half.npy"].tolist() == [1] * 7
    s = a["big.npy"]
    assert s.shape == (100,) and np.array_equal(s, b["big.npy"])
    assert np.all(np.diff(s) > 0) and s.min() >= 0 and s.max() <= 999 and np.all(s == np.round(s))
    assert sum(v.nbytes for v in a.values()) <= 3 * 4 * 100


def _run_bench(monkeypatch, capsys, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path, monkeypatch, capsys):
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--n-patches", "300"]
    outs = []
    for tag in ("a", "b"):
        d = _run_bench(monkeypatch, capsys, argv + ["--dump-outputs", str(tmp_path / tag)])
        assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["unit"] == "slides/sec" and d["dtype"] == "bf16"
        assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-3)
        # a plain run measures nothing beside its steps
        assert d["full"] is False and "cpu_baseline" not in d
        assert all(d[k] is None for k in ("roofline", "roofline_pinv_bwd", "hbm_roofline", "gemm_roofline", "optimizer_ms"))
        outs.append({f: np.load(tmp_path / tag / f) for f in sorted(os.listdir(tmp_path / tag))})
    a, b = outs
    assert list(a) == list(b) and {"loss.npy", "y_prob.npy", "y_hat.npy"} <= set(a)
    assert any(f.startswith("param.") for f in a) and any(f.startswith("grad.") for f in a)
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    for f in a:
        assert a[f].dtype == np.float32 and a[f].shape == b[f].shape and np.isfinite(a[f]).all(), f
    assert a["y_prob.npy"].shape == (1, 2) and a["y_prob.npy"].sum() == pytest.approx(1.0, abs=1e-5)
    assert any(np.abs(a[f]).max() > 0 for f in a if f.startswith("grad."))
    # the same seeded weights, bags and dropout seeds: the runs differ by the order of atomic sums at
    # most, far inside bf16's 2^-8 relative step on the O(1) logits behind these probabilities
    assert np.abs(a["y_prob.npy"] - b["y_prob.npy"]).max() <= 2.0 ** -8
