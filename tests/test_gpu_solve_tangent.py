"""nmpc_solve_tangent_batch / nmpc_solve_tangent_batch_dev (Solver.sensitivity_fused,
sensitivity_device, feedback_gain_device, the jvp of nmpc_amd.autograd.solve): the forward-mode
sensitivity of a solution as one launch -- barrier weights, delta ladder, parameter products and
solves on the device -- against the dense checker of tests/solve_tangent_ref.py, against the
adjoint identity with the fused reverse-mode launch, and against the host route it fuses
(Solver.sensitivity(tangent="exact"))."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import adjoint_ref as ar
from tests import eval_ref as er
from tests import kkt_ref as kr
from tests import param_ref as qr
from tests import solve_adjoint_ref as sr
from tests import solve_tangent_ref as tr
from tests.test_gpu_solve_adjoint import _bnd, _g, _solved, _solver, _ulps  # the solved cases are shared

pytestmark = pytest.mark.gpu

OUT = ("dx", "dlam_g", "dX")
SEEDS = ("x_bar", "lam_g_bar", "X_bar")
CASES = tr.SOLVED


def _dirs(spec, B, nd, seed):
    """(np, nd, B), N(0, 1)."""
    return np.ascontiguousarray(np.transpose(tr.draw_directions(spec, B, nd, seed), (2, 1, 0)))


def _seeds(spec, B, na, seed):
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((n, na, B)) for k, n in zip(SEEDS, (spec.nw, spec.ng, spec.nX))}


def _fused(s, sol, bounds, P, dp, g=True):
    so = sol if g else {k: v for k, v in sol.items() if k != "g"}
    return s.sensitivity_fused(so, *bounds, P.T, dp)


def _prep(spec, sol, bounds, P, dp, B, nd, keys=OUT + ("info", "delta"), g=True, rep=True):
    """Device tensors for Solver.sensitivity_device from host data: dp (np, nd, B) or (np, nd)
    (shared); bounds (n,) shared (rep: replicated per scenario instead) or (n, B)."""
    import torch

    f64 = dict(dtype=torch.float64, device="cuda")

    def cols(a):  # (n,) or (n, B) -> device (n,) or (B, n)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = np.repeat(a[:, None], B, axis=1) if rep else a
        return torch.tensor(np.ascontiguousarray(a.T if a.ndim == 2 else a), **f64)

    dsol = {k: cols(sol[k]) for k in ("x", "lam_g", "lam_x")}
    if g:
        dsol["g"] = cols(sol["g"])
    db = [cols(v) for v in bounds]
    dd = torch.tensor(np.ascontiguousarray(np.transpose(dp, (2, 1, 0)) if dp.ndim == 3 else dp.T), **f64)
    shapes = {"dx": (B, nd, spec.nw), "dlam_g": (B, nd, spec.ng), "dX": (B, nd, spec.nX)}
    out = {k: torch.full(shapes[k], 7.0, **f64) for k in keys if k in shapes}
    if "info" in keys:
        out["info"] = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    if "delta" in keys:
        out["delta"] = torch.full((B,), 7.0, **f64)
    return dsol, db, cols(P.T), dd, out


def _host_layout(out):
    return {k: (np.transpose(v.cpu().numpy(), (2, 1, 0)) if v.dim() == 3 else v.cpu().numpy()) for k, v in out.items()}


def _device(s, spec, sol, bounds, P, dp, B, nd, **kw):
    """Solver.sensitivity_device on host data (see _prep), results in the host methods' layout."""
    import torch

    dsol, db, dP, dd, out = _prep(spec, sol, bounds, P, dp, B, nd, **kw)
    s.sensitivity_device(dsol, *db, dP, dd, out)
    torch.cuda.synchronize()
    return _host_layout(out)


def _same(a, b, what, keys=None):
    """Bitwise equality of two results (NaN equal to NaN)."""
    for k in (keys or a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _dpb(dp, b):
    """Scenario b's directions, (nd, np)."""
    return dp[:, :, b].T if dp.ndim == 3 else dp.T


def _check(name, prob, got, sol, bounds, P, dp, B, nd, g=None, brf=1e-8):
    """Gates (a) and (b) for every scenario with info 0, against the dense checker at the returned
    delta; returns the checker's per-scenario results."""
    res = []
    for b in range(B):
        if got["info"][b] != 0:
            res.append(None)
            continue
        d = _dpb(dp, b)
        ref = tr.dense_tangent(prob, sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b], P[b],
                               [_bnd(v, b) for v in bounds], d, delta=got["delta"][b],
                               g=None if g is None else g[:, b], brf=brf)
        free = ref["free"]
        dx = got["dx"][:, :, b].T
        assert np.all(dx[:, ~free] == 0.0), (name, b)
        rho = max(kr.rho(ref["M"], dx[j][free], ref["rhs"][j]) for j in range(nd))
        own = tr.products_on(ref, dx, d)
        fig = tr.check_against({k: got[k][:, :, b].T for k in tr.KEYS}, own, f"{name} scenario {b}")
        print(f"{name} scenario {b}: rho(dx) {rho:.2e} (bound {kr.TOL:.0e}), dlam_g error / bound {fig['dlam_g']:.2e}, "
              f"dX {fig['dX']:.2e}, delta {got['delta'][b]:.3g}, cond(M) {np.linalg.cond(ref['M']):.1e}")
        assert rho <= kr.TOL, (name, b, rho)
        res.append(ref)
    return res


def _identity_bound(ref, q, dx, j, xb, lb, Xb, d):
    """Gate (c), the bound of tests/test_gpu_solve_adjoint.py's (c): the two solves' gate (a) seen
    through each other's solution, and twice gate (b) of every product in either side."""
    dn, ss, free = ref["dn"], ref["ss"], ref["free"]
    J, Z, Cm, Jp, Xp = dn["J"], dn["Z"], dn["C"], dn["Jp"], dn["Xp"]
    aMf = np.abs(ref["M"])
    r_q = xb + Xb @ Z + (ss * lb) @ J
    den_q = float(np.max(aMf @ np.abs(q[free]))) + float(np.max(np.abs(r_q[free])))
    den_x = float(np.max(aMf @ np.abs(dx[free]))) + float(np.max(np.abs(ref["rhs"][j])))
    bound = kr.TOL * (np.sum(np.abs(q)) * den_x + np.sum(np.abs(dx)) * den_q)
    bound += 2 * (_g(q, Cm, d) + _g(ss * (np.abs(lb) + np.abs(J) @ np.abs(q)), Jp, d)
                  + _g(ss * lb, J, dx) + _g(Xb, Z, dx) + _g(Xb, Xp, d))
    return bound


def _against_host(name, got, host, refs, B, nd, dp):
    """(d): info and delta equal, dx bitwise (the right-hand side is formed by the same
    operations: hp as it stands, one product sigma_s jp per row), dlam_g within gate (b)."""
    np.testing.assert_array_equal(got["info"], host["info"])
    np.testing.assert_array_equal(got["delta"], host["delta"])
    print(f"{name} against sensitivity(tangent='exact'), largest difference in ulps: "
          + ", ".join(f"{k} {_ulps(got[k], host[k]):.1f}" for k in ("dx", "dlam_g")))
    np.testing.assert_array_equal(got["dx"], host["dx"], err_msg=f"{name}: dx against the host route")
    for b in range(B):
        if refs[b] is None:
            continue
        own = tr.products_on(refs[b], got["dx"][:, :, b].T, _dpb(dp, b))
        err, sc = np.abs(got["dlam_g"][:, :, b].T - host["dlam_g"][:, :, b].T), own["scale"]["dlam_g"]
        assert np.all(err[sc == 0] == 0.0), (name, b)
        fig = float(np.max(err[sc > 0] / (tr.TOL * sc[sc > 0]), initial=0.0))
        print(f"{name} scenario {b}: dlam_g against the host route, difference / gate (b) {fig:.2e}")
        assert fig <= 1.0, (name, b, fig)


@pytest.mark.parametrize("name,unit", [(n, False) for n in CASES] + [("race_track_2", True)])
def test_fused_tangent_matches_the_checker_the_adjoint_and_the_host_route(name, unit):
    """Solved cases (every scenario converges), nd = 2 directions dp ~ N(0, 1), and dp = I
    (nd = np) on race_track_2.

    (a) dx against the dense M at the returned delta: rho(M, dx, rhs) <= kkt_ref.TOL with
        rhs = -C dp - J' Sigma_s Jp dp on the free variables; dx = 0 exactly on fixed ones.
    (b) dlam_g and dX against the checker's dense Sigma_s (J dx + Jp dp) and Z dx + Xp dp on the
        GPU's own dx, within TOL x the per-entry sum of the absolute terms.
    (c) The adjoint identity <pbar, dp> = <x_bar, dx> + <lam_g_bar, dlam_g> + <X_bar, dX> against
        Solver.sensitivity_adjoint_fused for N(0, 1) seeds (na = 2), within _identity_bound.
    (d) Against Solver.sensitivity(tangent="exact"), the launches this one fuses: _against_host."""
    spec, s, B, P, bounds, sol = _solved(name)
    lbx, ubx, lbg, ubg = bounds
    prob = er.problem_of(spec)
    nd = spec.np if unit else 2
    dp = np.repeat(np.eye(spec.np)[:, :, None], B, axis=2) if unit else _dirs(spec, B, nd, 81)
    got = _fused(s, sol, bounds, P, dp)
    assert got["dx"].shape == (spec.nw, nd, B) and got["dlam_g"].shape == (spec.ng, nd, B)
    assert got["dX"].shape == (spec.nX, nd, B) and got["info"].shape == (B,) and got["delta"].shape == (B,)
    print(f"{name}: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    refs = _check(name, prob, got, sol, bounds, P, dp, B, nd, g=sol["g"])
    # (c)
    na = 2
    seeds = _seeds(spec, B, na, 82)
    adj = s.sensitivity_adjoint_fused(sol, lbx, ubx, lbg, ubg, P.T, **seeds)
    np.testing.assert_array_equal(adj["delta"], got["delta"])
    for b in range(B):
        worst = 0.0
        for a in range(na):
            xb, lb, Xb = (seeds[k][:, a, b] for k in SEEDS)
            q = adj["q"][:, a, b]
            for j in range(nd):
                d = dp[:, j, b]
                dx = got["dx"][:, j, b]
                D = xb @ dx + lb @ got["dlam_g"][:, j, b] + Xb @ got["dX"][:, j, b] - adj["pbar"][:, a, b] @ d
                bound = _identity_bound(refs[b], q, dx, j, xb, lb, Xb, d)
                if bound == 0.0:  # an entry of p that nothing reads
                    assert D == 0.0, (name, b, a, j, D)
                    continue
                worst = max(worst, abs(D) / bound)
                assert abs(D) <= bound, (name, b, a, j, D, bound)
        print(f"{name} scenario {b}: adjoint identity defect / bound {worst:.2e}")
    # (d)
    host = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="exact")
    _against_host(name, got, host, refs, B, nd, dp)


@pytest.mark.parametrize("name", ["n1", "n63_16obs"])
def test_synthetic_points_on_the_smallest_and_largest_shape(name):
    """Random x inside the bounds and random signed multipliers (tests/eval_ref.draw_point), N = 1
    and N = 63 with 16 obstacles (every lane, every row slot), nd = 2, g NULL: every point
    factorises along the ladder (n63_16obs climbs it), gates (a), (b) hold against the dense
    checker and (d) against the host route."""
    spec = er.case_spec(name)
    prob = er.problem_of(spec)
    s = _solver(spec)
    B, nd = er.CASES[name], 2
    d = er.draw_point(spec, B, seed=31)
    bounds = (d["lbx"], d["ubx"], d["lbg"], d["ubg"])
    P = d["p"]
    sol = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    sol["g"] = s.evaluate(sol["x"], P.T)["g"]
    dp = _dirs(spec, B, nd, 83)
    got = _fused(s, sol, bounds, P, dp, g=False)
    print(f"{name}: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0), got["info"]
    if name == "n63_16obs":
        assert np.max(got["delta"]) > 1e-4  # the ladder climbed
    refs = _check(name, prob, got, sol, bounds, P, dp, B, nd, g=None)
    host = s.sensitivity(sol, *bounds, P.T, dp, tangent="exact")
    _against_host(name, got, host, refs, B, nd, dp)


def test_fixed_controls_equality_rows_and_invalid_bounds():
    """A third of the controls fixed through lbx == ubx, a whole stage among them: dx is exactly 0
    there, gates (a) and (b) hold on the free ones, and the host route gives the same info, delta
    and dx.  An equality row (lbg == ubg) in one scenario, lbx > ubx in another and a NaN multiplier
    in a third give info -11, delta 0 and NaN for those scenarios; the remaining one is bitwise
    what it is without them.  The host wrapper raises on equality rows."""
    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    lbx, ubx, lbg, ubg = bounds
    nd = 2
    dp = _dirs(spec, B, nd, 84)
    rng = np.random.default_rng(78)
    fx = rng.uniform(size=(spec.nw, B)) < 1.0 / 3.0
    nu = spec.nw // spec.N
    fx[:nu, 0] = True  # a whole stage
    lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb2[fx], ub2[fx] = sol["x"][fx], sol["x"][fx]
    b2 = (lb2, ub2, lbg, ubg)
    got = _fused(s, sol, b2, P, dp)
    print(f"fixed controls: {fx.sum(axis=0)} of {spec.nw}, info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    for b in range(B):
        assert np.all(got["dx"][fx[:, b], :, b] == 0.0), b
    refs = _check("fixed controls", prob, got, sol, b2, P, dp, B, nd, g=sol["g"])
    assert all(np.array_equal(r["free"], ~fx[:, b]) for b, r in enumerate(refs))
    host = s.sensitivity(sol, lb2, ub2, lbg, ubg, P.T, dp, tangent="exact")
    _against_host("fixed controls", got, host, refs, B, nd, dp)
    # invalid scenarios
    full = _device(s, spec, sol, bounds, P, dp, B, nd)
    lg2, ug2 = (np.repeat(v[:, None], B, axis=1) for v in (lbg, ubg))
    lg2[spec.ng // 2, 0] = ug2[spec.ng // 2, 0]
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb3[5, 1] = ub3[5, 1] + 1.0
    sol3 = dict(sol, lam_g=sol["lam_g"].copy())
    sol3["lam_g"][3, 2] = np.nan
    got = _device(s, spec, sol3, (lb3, ub3, lg2, ug2), P, dp, B, nd)
    print(f"invalid scenarios: info {got['info']}, delta {got['delta']}")
    np.testing.assert_array_equal(got["info"], [-11, -11, -11, 0])
    np.testing.assert_array_equal(got["delta"][:3], 0.0)
    for k in OUT:
        assert np.all(np.isnan(got[k][:, :, :3])), k
        np.testing.assert_array_equal(got[k][:, :, 3], full[k][:, :, 3], err_msg=k)
    assert got["delta"][3] == full["delta"][3]
    with pytest.raises(ValueError):
        s.sensitivity_fused(sol, lbx, ubx, lg2, ug2, P.T, dp)


def test_the_ladder_runs_in_the_kernel():
    """With first_hessian_perturbation = 1e-12 on the handle: at the solved points M is singular
    rather than indefinite at delta = 0, so the first rung already factorises -- delta = 1e-12 in
    the kernel and on the host; at synthetic points (random multipliers: M indefinite) many rungs
    are needed, and delta equals the host ladder's exactly, scenario by scenario, with dx the
    host's bits.  With max_hessian_perturbation below the first rung a scenario whose M does not
    factorise at delta = 0 keeps info = 1, the delta it was last tried at and NaN in dx, dlam_g,
    dX; a scenario that factorises at 0 (here: one whose undetermined last stage is fixed through
    its bounds) is bitwise what it is under the default ladder."""
    spec, s0, B, P, bounds, sol = _solved("race_track_2")
    lbx, ubx, lbg, ubg = bounds
    nd = 2
    dp = _dirs(spec, B, nd, 85)
    s = _solver(spec, first_hessian_perturbation=1e-12)
    rungs = [1e-12, 100.0 * 1e-12]
    for _ in range(60):
        rungs.append(8.0 * rungs[-1])
    got = _fused(s, sol, bounds, P, dp)
    host = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="exact")
    print(f"ladder from 1e-12, solved points: info {got['info']}, delta {got['delta']}, host delta {host['delta']}")
    _same(got, host, "ladder from 1e-12", ("info", "delta", "dx"))
    assert np.all(got["info"] == 0) and all(d in rungs for d in got["delta"]), got["delta"]
    Bs = er.CASES["race_track_2"]
    d = er.draw_point(spec, Bs, seed=33)
    syn = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    syn["g"] = s.evaluate(syn["x"], d["p"].T)["g"]
    dps = _dirs(spec, Bs, nd, 86)
    got = _fused(s, syn, bounds, d["p"], dps)
    host = s.sensitivity(syn, lbx, ubx, lbg, ubg, d["p"].T, dps, tangent="exact")
    print(f"ladder from 1e-12, synthetic points: info {got['info']}, delta {got['delta']}, host delta {host['delta']}")
    _same(got, host, "ladder from 1e-12, synthetic points", ("info", "delta", "dx"))
    assert np.all(got["info"] == 0) and all(dl in rungs for dl in got["delta"]), got["delta"]
    climbed = [rungs.index(dl) + 1 for dl in got["delta"]]
    print(f"rungs climbed: {climbed}")
    assert max(climbed) >= 3
    # no rung allowed: per-scenario bounds, scenario 0 with its last stage fixed at the solution
    nu = spec.nw // spec.N
    lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb2[-nu:, 0] = ub2[-nu:, 0] = sol["x"][-nu:, 0]
    b2 = (lb2, ub2, lbg, ubg)
    ref = _fused(s0, sol, b2, P, dp)
    cut = _solver(spec, max_hessian_perturbation=1e-6)
    got = _fused(cut, sol, b2, P, dp)
    hst = cut.sensitivity(sol, lb2, ub2, lbg, ubg, P.T, dp, tangent="exact")
    print(f"max_hessian_perturbation 1e-6: info {got['info']}, delta {got['delta']}; default ladder: info "
          f"{ref['info']}, delta {ref['delta']}")
    np.testing.assert_array_equal(got["info"], hst["info"])
    np.testing.assert_array_equal(got["delta"], hst["delta"])
    stuck = ref["delta"] > 1e-6
    assert np.any(stuck)
    np.testing.assert_array_equal(got["info"], np.where(stuck, 1, 0))
    for k in OUT:
        assert np.all(np.isnan(got[k][:, :, stuck])), k
        np.testing.assert_array_equal(got[k][:, :, ~stuck], ref[k][:, :, ~stuck], err_msg=k)


def test_batch_plumbing():
    """All bitwise: nd = 3 equals three nd = 1 calls; leading dimension 0 for the bounds, p and the
    directions equals the replicated call; the host and the device entry point agree, for every
    subset of the outputs; a NaN in one direction leaves the other directions' bits unchanged; a
    direction along an entry of p that nothing reads gives zeros, whatever stands there.  With g
    NULL the weights come from the kernel's own g(x, p): info and delta are equal and the result
    (difference printed) passes the same gates."""
    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    nd = 3
    dp = _dirs(spec, B, nd, 87)
    full = _fused(s, sol, bounds, P, dp)
    assert np.all(full["info"] == 0)
    _same(_device(s, spec, sol, bounds, P, dp, B, nd), full, "device against host entry point")
    for j in range(nd):
        one = _fused(s, sol, bounds, P, dp[:, j:j + 1])
        for k in OUT:
            np.testing.assert_array_equal(one[k][:, 0], full[k][:, j], err_msg=f"{k} direction {j}")
        _same(one, full, f"direction {j}", ("info", "delta"))
    # leading dimension 0: shared bounds, p and directions against replicated ones
    sh = np.ascontiguousarray(dp[:, :, 0])
    P1 = np.repeat(P[:1], B, axis=0)
    sol1 = {k: np.repeat(v[:, :1], B, axis=1) for k, v in sol.items()}
    rep = _device(s, spec, sol1, bounds, P1, np.repeat(sh[:, :, None], B, axis=2), B, nd, rep=True)
    import torch

    dsol, db, dP, dd, out = _prep(spec, sol1, bounds, P1, sh, B, nd, rep=False)
    s.sensitivity_device(dsol, *db, dP[0].contiguous(), dd, out)
    torch.cuda.synchronize()
    shared = _host_layout(out)
    _same(shared, rep, "ld = 0")
    _same(shared, _fused(s, sol1, bounds, P1, sh), "ld = 0, host entry point")
    for b in range(1, B):
        for k in OUT:
            np.testing.assert_array_equal(shared[k][:, :, b], shared[k][:, :, 0], err_msg=k)
    # subsets of the outputs
    for n in (1, 2, 3):
        for keys in itertools.combinations(OUT, n):
            part = _device(s, spec, sol, bounds, P, dp, B, nd, keys=keys + (("info",) if n == 2 else ()))
            _same(part, full, f"outputs {keys}")
    # a NaN entry poisons its own direction only
    bad = dp.copy()
    bad[3, 1, :] = np.nan
    poisoned = _fused(s, sol, bounds, P, bad)
    for k in OUT:
        np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=f"{k}, NaN in a direction")
        assert np.all(np.any(np.isnan(poisoned[k][:, 1]), axis=0)), k
    _same(poisoned, full, "NaN in a direction", ("info", "delta"))
    # an entry of p that nothing reads
    unread = [i for i, kd in enumerate(qr.entry_kinds(prob)) if kd is None]
    assert unread, "race_track_2 reads every entry of p"
    un = np.zeros((spec.np, 2, B))
    un[unread[0], 0], un[unread[-1], 1] = 3.0, np.nan
    zero = _fused(s, sol, bounds, P, un)
    for k in OUT:
        assert np.all(zero[k] == 0.0), k
    # g NULL
    own = _fused(s, sol, bounds, P, dp, g=False)
    _same(own, full, "g NULL", ("info", "delta"))
    print("g NULL against the solve's g_out, largest difference in ulps: "
          + ", ".join(f"{k} {_ulps(own[k], full[k]):.1f}" for k in OUT))
    _check("race_track_2, g NULL", prob, own, sol, bounds, P, dp, B, nd, g=None)


def test_sensitivity_device_does_not_synchronise():
    """nmpc_solve_tangent_batch_dev only enqueues (the pattern of tests/test_gpu_solve_adjoint.py::
    test_sensitivity_adjoint_device_does_not_synchronise): behind a spinning kernel on a side
    stream the call returns while the stream is still busy, and the results equal an unobstructed
    run's.  After a solve of the same B it allocates nothing."""
    import time
    import torch

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    nd = 2
    dp = _dirs(spec, B, nd, 88)
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    ref = _device(s, spec, sol, bounds, P, dp, B, nd)
    assert s.memory_info() == mem  # the solve's workspace covers the launch
    dsol, db, dP, dd, o = _prep(spec, sol, bounds, P, dp, B, nd)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    per_cycle_ms = float("inf")  # the least of three: a busy host or a cold clock only ever inflates one
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(st):
            e0.record(st); torch.cuda._sleep(1 << 22); e1.record(st)
        torch.cuda.synchronize()
        per_cycle_ms = min(per_cycle_ms, e0.elapsed_time(e1) / (1 << 22))
    cycles = int(min(max(400.0 / max(per_cycle_ms, 1e-12), float(1 << 22)), float(1 << 34)))  # ~0.4 s
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        torch.cuda._sleep(cycles)
        e1.record(st)
    t0 = time.perf_counter()
    s.sensitivity_device(dsol, *db, dP, dd, o, stream=st)
    call_ms = (time.perf_counter() - t0) * 1e3
    busy = not st.query()
    torch.cuda.synchronize()
    spin_ms = e0.elapsed_time(e1)
    print(f"sensitivity_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info() == mem
    _same(_host_layout(o), ref, "behind the spinning kernel")


def test_argument_validation_on_a_live_handle():
    """B <= 0, nd <= 0, a NULL required pointer, every output NULL and a leading dimension that is
    neither 0 nor >= the vector length return NMPC_E_INVALID from both entry points before any
    device call: nothing is written, and the handle still works."""
    from nmpc_amd import _lib

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    L = _lib.lib()
    nd = 2
    nw, ng, npp, nX = spec.nw, spec.ng, spec.np, spec.nX
    arr = {"x": sol["x"].T, "p": P, "lam_g": sol["lam_g"].T, "lam_x": sol["lam_x"].T, "g": sol["g"].T,
           "lbx": np.repeat(bounds[0][None], B, 0), "ubx": np.repeat(bounds[1][None], B, 0),
           "lbg": np.repeat(bounds[2][None], B, 0), "ubg": np.repeat(bounds[3][None], B, 0),
           "dp": np.transpose(_dirs(spec, B, nd, 89), (2, 1, 0))}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    arr.update(dx=np.full((B, nd, nw), 7.0), dlam_g=np.full((B, nd, ng), 7.0), dX=np.full((B, nd, nX), 7.0),
               delta=np.full(B, 7.0))
    info = np.full(B, 99, dtype=np.int32)
    names = ("x", "p", "lam_g", "lam_x", "g", "lbx", "ubx", "lbg", "ubg", "dp")
    lens = dict(zip(names, (nw, npp, ng, nw, ng, nw, nw, ng, ng, npp * nd)))
    dpt, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)

    def call(B_=B, nd_=nd, null=(), ld=None, dev=False):
        ld = dict(lens, **(ld or {}))
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k not in null else vp(0)  # noqa: E731
            gi = vp(info.ctypes.data)
        else:
            g = lambda k: arr[k].ctypes.data_as(dpt) if k not in null else None  # noqa: E731
            gi = info.ctypes.data_as(ip)
        args = [s._h, B_, nd_]
        for k in names:
            args += [g(k), ld[k]]
        args += [g("dx"), g("dlam_g"), g("dX"), gi, g("delta")]
        return L.nmpc_solve_tangent_batch_dev(*args, vp(0)) if dev else L.nmpc_solve_tangent_batch(*args)

    # each with the full message of its rule; the last four break two rules at once: the earlier
    # one in the order of the checks answers
    req, ldm = "required pointer is null (x, p, lam_g, lam_x, lbx, ubx, lbg, ubg, dp)", "leading dimension smaller than the vector length"
    outs = "dx_out, dlam_g_out and dX_out are all null"
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("nd = 0", dict(nd_=0), "nd <= 0"),
                 ("nd < 0", dict(nd_=-1), "nd <= 0"), ("every output NULL", dict(null=OUT), outs),
                 ("ld_x negative", dict(ld={"x": -nw}), ldm), ("ld_dp one direction", dict(ld={"dp": npp}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in names if k != "g"]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and nd = 0", dict(B_=0, nd_=0), "B <= 0"), ("nd = 0 and x NULL", dict(nd_=0, null=("x",)), "nd <= 0"),
                  ("dp NULL and no output", dict(null=("dp",) + tuple(OUT)), req),
                  ("no output and ld_p short", dict(null=OUT, ld={"p": npp - 1}), outs)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error(), what
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    call(null=OUT)
    assert "dx_out" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(nd_=0))
    assert all(np.all(arr[k] == 7.0) for k in OUT + ("delta",)) and np.all(info == 99)  # nothing ran
    # and the handle still works: g NULL, dX alone; leading dimension 0 shares everything
    assert call(null=("g", "dx", "dlam_g", "delta")) == 0
    assert np.all(np.isfinite(arr["dX"])) and np.all(info == 0) and np.all(arr["dx"] == 7.0) and np.all(arr["dlam_g"] == 7.0)
    assert call(ld={k: 0 for k in names}) == 0
    for k in OUT:
        assert np.all(np.isfinite(arr[k]))
        for b in range(1, B):
            np.testing.assert_array_equal(arr[k][0], arr[k][b])


def test_feedback_gain_device(monkeypatch):
    """K = d u0* / d x0 equals the first nu rows of sensitivity_fused's dx for the nx unit directions
    of p's x0 block, bitwise, with the same info; with torch.Tensor.cpu made to raise the call
    still completes: it reads nothing back."""
    import torch

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    nu, nx = spec.nw // spec.N, spec.nX // (spec.N + 1)
    ref = _fused(s, sol, bounds, P, np.eye(spec.np)[:, :nx])
    dsol, db, dP, _, _ = _prep(spec, sol, bounds, P, np.zeros((spec.np, 1)), B, 1, rep=False)

    def boom(*a, **k):
        raise AssertionError("a host round trip in feedback_gain_device")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        K, info = s.feedback_gain_device(dsol, *db, dP)
    torch.cuda.synchronize()
    assert tuple(K.shape) == (B, nu, nx) and K.is_contiguous() and info.dtype == torch.int32
    np.testing.assert_array_equal(info.cpu().numpy(), ref["info"])
    np.testing.assert_array_equal(np.transpose(K.cpu().numpy(), (1, 2, 0)), ref["dx"][:nu])
    pre = {"K": torch.full((B, nu, nx), 7.0, dtype=torch.float64, device="cuda"),
           "info": torch.full((B,), 99, dtype=torch.int32, device="cuda")}
    K2, info2 = s.feedback_gain_device(dsol, *db, dP, out=pre)
    assert K2 is pre["K"] and info2 is pre["info"] and torch.equal(K2, K) and torch.equal(info2, info)
    # NaN where info != 0
    lx = dsol["lam_x"].clone()
    lx[1, 2] = float("nan")
    K3, info3 = s.feedback_gain_device(dict(dsol, lam_x=lx), *db, dP)
    assert info3.cpu().numpy().tolist() == [0, -11] + [0] * (B - 2)
    assert bool(torch.all(torch.isnan(K3[1]))) and torch.equal(K3[0], K[0]) and torch.equal(K3[2:], K[2:])


def test_autograd_forward_mode():
    """torch.autograd.forward_ad through nmpc_amd.autograd.solve: with backward="device" the
    tangents on x and X are sensitivity_device's dx and dX for the same direction, bitwise, and
    backward="host" (sensitivity_fused) gives the same bits; <p.grad, t> of a random linear loss
    equals <x_bar, jvp_x> + <X_bar, jvp_X> within gate (c)'s bound; with max_iter = 1 every
    tangent row is NaN."""
    import torch
    import torch.autograd.forward_ad as fwAD
    from nmpc_amd import autograd

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    lbx, ubx, lbg, ubg = bounds
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(90)
    t = rng.standard_normal((B, spec.np))
    cx, cX = rng.standard_normal((B, spec.nw)), rng.standard_normal((B, spec.nX))
    tan = {}
    for mode in ("device", "host"):
        with fwAD.dual_level():
            pd = fwAD.make_dual(torch.tensor(P, **f64), torch.tensor(t, **f64))
            x, X = autograd.solve(s, pd, lbx, ubx, lbg, ubg, backward=mode)
            tx, tX = fwAD.unpack_dual(x).tangent, fwAD.unpack_dual(X).tangent
            assert tx is not None and tX is not None
            tan[mode] = (tx.cpu().numpy(), tX.cpu().numpy())
            np.testing.assert_array_equal(fwAD.unpack_dual(x).primal.cpu().numpy().T, sol["x"])
    dp = np.ascontiguousarray(t.T[:, None, :])  # (np, 1, B)
    ref = _device(s, spec, sol, bounds, P, dp, B, 1, keys=("dx", "dX", "info"))
    assert np.all(ref["info"] == 0)
    for mode in ("device", "host"):
        np.testing.assert_array_equal(tan[mode][0], ref["dx"][:, 0, :].T, err_msg=mode)
        np.testing.assert_array_equal(tan[mode][1], ref["dX"][:, 0, :].T, err_msg=mode)
    # backward against forward
    p = torch.tensor(P, requires_grad=True, **f64)
    x, X = autograd.solve(s, p, lbx, ubx, lbg, ubg, backward="device")
    (g,) = torch.autograd.grad((torch.tensor(cx, **f64) * x).sum() + (torch.tensor(cX, **f64) * X).sum(), p)
    g = g.cpu().numpy()
    adj = s.sensitivity_adjoint_fused(sol, lbx, ubx, lbg, ubg, P.T, x_bar=cx.T[:, None, :], X_bar=cX.T[:, None, :])
    full = _fused(s, sol, bounds, P, dp)
    refs = _check("autograd", prob, full, sol, bounds, P, dp, B, 1, g=sol["g"])
    worst = 0.0
    for b in range(B):
        D = cx[b] @ tan["device"][0][b] + cX[b] @ tan["device"][1][b] - g[b] @ t[b]
        bound = _identity_bound(refs[b], adj["q"][:, 0, b], tan["device"][0][b], 0, cx[b], np.zeros(spec.ng), cX[b], t[b])
        worst = max(worst, abs(D) / bound)
        assert abs(D) <= bound, (b, D, bound)
    print(f"autograd: <p.grad, t> against <x_bar, jvp_x> + <X_bar, jvp_X>, defect / bound {worst:.2e}")
    # no scenario converges in one iteration: NaN rows, never zeros
    s1 = _solver(spec, max_iter=1)
    for mode in ("device", "host"):
        with fwAD.dual_level():
            pd = fwAD.make_dual(torch.tensor(P, **f64), torch.tensor(t, **f64))
            x1, X1 = autograd.solve(s1, pd, lbx, ubx, lbg, ubg, backward=mode)
            assert bool(torch.all(torch.isnan(fwAD.unpack_dual(x1).tangent))), mode
            assert bool(torch.all(torch.isnan(fwAD.unpack_dual(X1).tangent))), mode
