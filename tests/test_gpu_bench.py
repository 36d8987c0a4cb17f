"""bench.py on the GPU, in this process on a small batch: a plain run times the headline
steps only (the side legs need --full), --steps sets the number of timed steps, and
--dump-outputs writes the timed path's results, identical from run to run."""
import json
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_LEGS = ("cpu_baseline", "parity_sample", "per_step_launch", "config5")


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, ROOT)
    import bench as b
    return b


def _run(bench, monkeypatch, capsys, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", *argv])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_reproducible_outputs(bench, monkeypatch, capsys, tmp_path):
    B, K, W = 96, 3, 1
    args = ("--steps", str(K), "--warmup", str(W), "--batch", str(B))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _run(bench, monkeypatch, capsys, *args, "--dump-outputs", a)
    assert not any(k in res for k in SIDE_LEGS)
    assert res["steps"] == K and res["warmup"] == W and res["steps_done"] == B * K
    assert res["metric"] == bench.METRIC and res["unit"] == "MPC steps/s" and res["dtype"] == "f64"
    assert res["higher_is_better"] is True and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(B * K / (res["ms_per_step"] * K / 1e3))
    _run(bench, monkeypatch, capsys, *args, "--dump-outputs", b)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b)) and {"u.npy", "f.npy", "status.npy", "w_final.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float64 and x.shape == y.shape
        np.testing.assert_array_equal(x, y)
        total += os.path.getsize(os.path.join(a, n))
    assert total <= bench.DUMP_MAX_BYTES
    u, st = np.load(os.path.join(a, "u.npy")), np.load(os.path.join(a, "status.npy"))
    assert u.shape == (K, B, 6) and st.shape == (K, B) and np.isin(st, (0, 1)).any()
    assert np.isfinite(u[st == 0]).all() and np.abs(u[st == 0]).max() > 0


def test_full_run_keeps_the_side_legs(bench, monkeypatch, capsys):
    res = _run(bench, monkeypatch, capsys, "--full", "--steps", "2", "--warmup", "1", "--batch", "64",
               "--config5-batch", "64", "--config5-cpu-scenarios", "16", "--cpu-budget", "5",
               "--config5-cpu-budget", "5")
    assert all(k in res for k in SIDE_LEGS)
    assert res["steps"] == 2 and res["config5"]["steps"] == 2 and res["per_step_launch"]["value"] > 0
    assert res["parity_sample"]["steps_compared"] > 0 and res["cpu_baseline"]["value"] > 0
