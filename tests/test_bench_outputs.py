"""bench.py --dump-outputs / --full: the sampling of the dumped arrays (CPU), and on the GPU a plain
run's result line and its dumped outputs, which two runs with the same arguments must reproduce."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_outputs_whole_or_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    g = torch.Generator().manual_seed(0)
    Y = torch.randn(6, 7, 5, 16, 1, generator=g)             # 3360 elements: sampled; Y[-1] 560: whole
    hyp = torch.rand(5, 4, 1, generator=g).double()
    bench.dump_outputs(str(tmp_path / "a"), Y, hyp)
    bench.dump_outputs(str(tmp_path / "b"), Y.clone(), hyp)
    got = {f: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["Y.npy", "Y_final.npy", "hyp.npy"]
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["Y.npy"].shape == (1000,)
    assert np.isin(got["Y.npy"], Y.numpy()).all()            # elements of Y, at the same places
    assert np.array_equal(got["Y_final.npy"], Y[-1].numpy())  # in both dumps
    assert np.array_equal(got["hyp.npy"], hyp.float().numpy())
    for f, v in got.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / f))
    Y2 = Y.clone()
    Y2[3] += 1.0                                             # a changed iterate shows in the sample
    bench.dump_outputs(str(tmp_path / "c"), Y2, hyp)
    assert not np.array_equal(got["Y.npy"], np.load(tmp_path / "c" / "Y.npy"))


def _plain_runs(out_dirs):
    """One plain run per directory, side by side (most of a run is the start of its process)."""
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                               "--steps", "3", "--warmup", "1", "--min-warmup-s", "0",
                               "--dump-outputs", str(d)], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for d in out_dirs]
    done = [p.communicate(timeout=120) for p in procs]        # both have ended before any check
    results = []
    for p, (out, err) in zip(procs, done):
        assert p.returncode == 0, err[-2000:]
        lines = out.strip().splitlines()
        assert len(lines) == 1                                # one JSON result line
        results.append(json.loads(lines[0]))
    return results


@pytest.mark.gpu
def test_plain_run_is_lean_and_its_outputs_repeat(tmp_path, cuda):
    for r in _plain_runs([tmp_path / "d1", tmp_path / "d2"]):
        assert r["steps"] == 3 and r["warmup_steps_run"] == 1 and r["full"] is False
        assert r["parity"] is None and r["cpu_baseline"] is None and r["extras"] is None
        assert r["unit"] == "ADMM-iters/s" and r["higher_is_better"] is True and r["dtype"] == "f32"
        assert r["status"] == {"headline_forward": 0}
        # value and ms_per_step describe the same timed steps: B K / value = seconds per step
        assert r["ms_per_step"] > 0
        assert r["value"] == pytest.approx(4096 * 25 / (r["ms_per_step"] * 1e-3), rel=1e-9)
    shapes = {"Y.npy": (25, 4096, 5, 256, 1), "Y_final.npy": (4096, 5, 256, 1), "hyp.npy": (5, 4, 1)}
    total = 0
    for f, shape in shapes.items():
        a, b = np.load(tmp_path / "d1" / f), np.load(tmp_path / "d2" / f)
        # the headline's Y has 131 M elements: its 6 M-element sample; the others (5.2 M, 20) whole
        assert a.shape == ((6_000_000,) if f == "Y.npy" else shape) and a.dtype == np.float32
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a, b), f
        total += a.nbytes
    assert total <= 64e6
