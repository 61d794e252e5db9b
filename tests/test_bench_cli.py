"""bench.py's command line: a plain run does the headline only, --full adds the rest, --dump-outputs
writes what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import gpu_available

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _result(n=1000, kk=5):
    g = torch.Generator().manual_seed(1)
    return dict(tau=torch.rand(n, dtype=torch.float64, generator=g),
                Y=torch.rand((n, kk), dtype=torch.float64, generator=g),
                stats=torch.randint(0, 1000, (n, 8), dtype=torch.int32, generator=g),
                _inputs=[torch.zeros(3)])


def test_dump_outputs_writes_every_array_as_float64(tmp_path):
    import bench

    res = _result()
    bench.dump_outputs(str(tmp_path / "d"), res)
    assert sorted(os.listdir(tmp_path / "d")) == ["Y.npy", "stats.npy", "tau.npy"]
    for k in ("tau", "Y", "stats"):
        a = np.load(tmp_path / "d" / (k + ".npy"))
        assert a.dtype == np.float64 and a.shape == tuple(res[k].shape)
        assert np.array_equal(a, res[k].numpy().astype(np.float64))


def test_dump_outputs_samples_a_large_result_the_same_way_every_time(tmp_path, monkeypatch):
    import bench

    res = _result()
    row_bytes = 8 * (1 + 5 + 8) + 8
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * row_bytes)
    bench.dump_outputs(str(tmp_path / "a"), res)
    bench.dump_outputs(str(tmp_path / "b"), res)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and rows.size == 100 and np.all(np.diff(rows) > 0)
    total = 0
    for k in ("tau", "Y", "stats", "rows"):
        a, b = np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy"))
        assert np.array_equal(a, b)
        total += a.nbytes
        if k != "rows":
            assert np.array_equal(a, res[k].numpy()[rows.astype(np.int64)].astype(np.float64))
    assert total <= 100 * row_bytes


@pytest.mark.gpu
@pytest.mark.skipif(not gpu_available(), reason="needs an MI355X")
def test_plain_run_times_the_requested_steps_and_dumps_its_outputs(tmp_path):
    """A plain run on a 64-reactor slice of the headline sweep: --steps sets the number of timed steps,
    ms_per_step is the time of one of them, nothing that belongs to --full has run, and the dump holds
    the arrays of the last step, consistent with the counts of the result line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup",
                          "1", "--reactors", "64", "--dump-outputs", str(tmp_path / "d")], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    rep = json.loads(out.stdout.strip().splitlines()[-1])
    assert rep["steps"] == 2 and rep["warmup"] == 1 and rep["full"] is False
    assert rep["unit"] == "reactors/s" and rep["higher_is_better"] is True and rep["dtype"] == "f64"
    assert rep["ms_per_step"] > 0
    assert abs(rep["value"] * rep["ms_per_step"] / 1e3 / 64 - 1) < 1e-9
    for k in ("cpu_baseline", "pcie_inclusive", "c1", "c4", "c5", "rop", "lu", "rop_161sp", "rop_ext161", "pfr",
              "hcci"):
        assert rep[k] is None, k
    shapes = dict(tau=(64,), T=(64,), P=(64,), V=(64,), Y=(64, 53), stats=(64, 8), t_stop=(64,))
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in shapes)
    d = {k: np.load(tmp_path / "d" / (k + ".npy")) for k in shapes}
    for k, s in shapes.items():
        assert d[k].dtype == np.float64 and d[k].shape == s and np.all(np.isfinite(d[k])), k
    assert rep["failed_reactors"] == 0 == int((d["stats"][:, 6] != 0).sum())
    assert rep["not_ignited"] == int((d["tau"] <= 0).sum())
    # mass fractions still sum to one (a linear invariant of the integrator; 1e-8 is the run's rtol)
    assert np.all(np.abs(d["Y"].sum(axis=1) - 1) < 1e-8) and np.all(d["t_stop"] > 0)
