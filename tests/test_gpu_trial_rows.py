"""The line-search trials of the LDS-row class form their row values inside their row pass
(Solver::row_scaled) instead of stage-parallel before it (eval_fg / eval_fg2), and a
speculative pair's second trial forms them from its parked X straight into dt.  Every test
runs the same inputs on two handles -- one created with NMPC_STAGE_ROWS=1 (Params::stagerows:
the stage-parallel order, the pair's rows parked in dms and copied on acceptance) -- and
asserts bitwise equal results."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SWITCH = "NMPC_STAGE_ROWS"


def _solver(spec):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)


def _both(monkeypatch, run):
    """run() on a handle of the product's order and on one created under the switch"""
    monkeypatch.delenv(SWITCH, raising=False)
    new = run()
    monkeypatch.setenv(SWITCH, "1")
    old = run()
    monkeypatch.delenv(SWITCH, raising=False)
    return new, old


def _solve(spec, x0, bounds, P, trace=False):
    lbx, ubx, lbg, ubg = bounds
    s = _solver(spec)
    if trace:
        s.set_trace(True)
    sol = s(x0=x0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    out = {k: np.array(sol[k]) for k in ("x", "f", "g", "lam_g", "lam_x")}
    out["status"] = np.array(s.stats()["status_code"])
    out["iters"] = np.array(s.stats()["iter_count"])
    if trace:
        out["trace"] = np.array(s.read_trace(P.shape[0]))
    return out


def _assert_same(new, old):
    assert new.keys() == old.keys()
    for k in new:
        np.testing.assert_array_equal(new[k], old[k], err_msg=k)


def test_restoration_fixtures_are_bitwise_equal(monkeypatch):
    """The 16 restoration fixtures (N = 20, 10 obstacles: m = 15, ng = 315 -- rows straddle
    stage boundaries inside a 64-lane trip and the fifth trip is partial), trace on: the whole
    trace and x, f, g, lam_g, lam_x, status, iterations.  The stage-parallel run must contain
    restoration iterations accepted after backtracking (trace column 7 <= -2), i.e. a pair's
    second trial was taken."""
    from nmpc_amd import make_spec

    G = np.load(os.path.join(GOLD, "resto_cases.npz"))
    spec = make_spec("race_track_2", N=20, T=0.2)
    assert (spec.m, spec.ng) == (15, 315)
    new, old = _both(monkeypatch, lambda: _solve(spec, G["w"].T, spec.bounds(), G["p"], trace=True))
    ls = old["trace"][:, :, 7]
    print(f"restoration iterations {int((ls < 0).sum())}, of them backtracked {int((ls <= -2).sum())}, "
          f"iterations {int(old['iters'].sum())}")
    assert int((ls <= -2).sum()) > 0, "no backtracked restoration acceptance in the fixtures"
    _assert_same(new, old)


@pytest.mark.parametrize("nospec", [False, True])
def test_bounding_chains_are_bitwise_equal(monkeypatch, nospec):
    """The three restoration-heavy chains that bound the benchmark launch (scenarios 2284,
    2685, 3646 of config 3's seed-1003 draw) with their neighbours, B = 8, K = 20 closed-loop
    steps from u = 0: histories and the final p and w.  nospec: NMPC_NO_SPEC=1 on both sides,
    so the restoration trials are all formed alone (spec 0)."""
    import torch
    from nmpc_amd import config_spec, draw_scenarios

    spec = config_spec(3)
    rows = [2283, 2284, 2285, 2685, 2686, 3645, 3646, 3647]
    B, K = len(rows), 20
    P = draw_scenarios(spec, 4096, seed=1003)[rows]
    f64 = dict(dtype=torch.float64, device="cuda")
    bnd = [torch.tensor(v, **f64) for v in spec.bounds()]
    vt, wt = torch.full((B,), 12.0, **f64), torch.full((B,), 0.01, **f64)
    if nospec:
        monkeypatch.setenv("NMPC_NO_SPEC", "1")

    def run():
        s = _solver(spec)
        hist = {"u": torch.empty(K, B, 6, **f64), "f": torch.empty(K, B, **f64),
                "status": torch.empty(K, B, dtype=torch.int32, device="cuda"),
                "iters": torch.empty(K, B, dtype=torch.int32, device="cuda")}
        p, w = torch.tensor(P, **f64), torch.zeros(B, spec.nw, **f64)
        s.closed_loop_device(K, *bnd, p, w, vt, wt, hist)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in hist.items()}
        out["p"], out["w"] = p.cpu().numpy(), w.cpu().numpy()
        return out

    new, old = _both(monkeypatch, run)
    st = old["status"]
    print(f"iterations {int(old['iters'].sum())}, max_iter steps {int((st == -1).sum())}")
    assert int((st == -1).sum()) > 0, "no max_iter step on the bounding chains"
    _assert_same(new, old)


def _edge_specs():
    from nmpc_amd import config_spec, make_spec
    from nmpc_amd import spec as S

    rng = np.random.default_rng(0)
    xy = rng.uniform(-300, 1500, (16, 2))
    obs16 = tuple(S.Obstacle(float(x), float(y), 40.0) for x, y in xy)
    return {
        "no_obstacles": (make_spec(None, N=20, T=0.2), 16),              # m = nb
        "16_obstacles": (S.ProblemSpec(N=10, T=0.2, obstacles=obs16).validate(), 16),  # m = 21
        "N1": (make_spec("race_track_2", N=1, T=0.2), 16),
        "N20_pairs": (make_spec("race_track_2", N=20, T=0.2), 16),       # the largest N with pairs
        "N21_no_pairs": (make_spec("race_track_2", N=21, T=0.2), 16),    # the next class: no pairs
        "no_gimbal": (make_spec("race_track_2", N=20, T=0.2, model="uav5"), 16),  # nb = 2, m = 12
        # the LDS-row class's row maximum without the gimbal rows: 2 + 13 rows per stage
        "no_gimbal_13_obstacles": (make_spec(None, N=20, T=0.2, obstacles=obs16[:13], model="uav5"), 16),
        "config5_N50": (config_spec(5), 8),                              # global rows: the switch changes nothing
    }


@pytest.mark.parametrize("case", ["no_obstacles", "16_obstacles", "N1", "N20_pairs", "N21_no_pairs", "no_gimbal",
                                  "no_gimbal_13_obstacles", "config5_N50"])
def test_row_map_shape_edges_are_bitwise_equal(monkeypatch, case):
    """Cold solves from u = 0 at the shapes where the map from a row to its stage and kind
    changes: x, f, g, status, iterations (and the multipliers)."""
    from nmpc_amd import draw_scenarios

    spec, B = _edge_specs()[case]
    P = draw_scenarios(spec, B, seed=1003)
    new, old = _both(monkeypatch, lambda: _solve(spec, np.zeros(spec.nw), spec.bounds(), P))
    print(f"{case}: m {spec.m}, ng {spec.ng}, iterations {int(old['iters'].sum())}, status {old['status'].tolist()}")
    assert np.all(np.isfinite(old["x"]))
    _assert_same(new, old)
