"""nmpc_solve_adjoint_batch / nmpc_solve_adjoint_batch_dev (Solver.sensitivity_adjoint_fused,
sensitivity_adjoint_device, nmpc_amd.autograd.solve(backward="device")): the reverse-mode
sensitivity of a solution as one launch -- barrier weights, delta ladder, solves and pullback on
the device -- against the dense checker of tests/solve_adjoint_ref.py, against the adjoint
identity with the forward sensitivity, and against the three-launch host route it fuses
(Solver.sensitivity_adjoint)."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import adjoint_ref as ar
from tests import eval_ref as er
from tests import kkt_ref as kr
from tests import solve_adjoint_ref as sr

pytestmark = pytest.mark.gpu

SEEDS = ("x_bar", "lam_g_bar", "X_bar")
OUT = ("pbar", "q", "jq")
SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(SEEDS, n)]
# the solved cases: those of the CPU checker (tests/solve_adjoint_ref.SOLVED, where the oracle
# converges on every scenario: tests/test_solve_adjoint_capi.py asserts it); the GPU's convergence
# is asserted below
CASES = sr.SOLVED


def _solver(spec, opts=None, **ipopt):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    if ipopt:
        opts = dict(REFERENCE_OPTS, ipopt=dict(REFERENCE_OPTS["ipopt"], **ipopt))
    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS if opts is None else opts)


@functools.lru_cache(maxsize=None)
def _solved(name):
    """(spec, solver, B, P, bounds, solution): computed once, shared and left unchanged."""
    spec, P = sr.scenarios(name)
    B = P.shape[0]
    s = _solver(spec)
    bounds = spec.bounds()
    sol = s(x0=np.zeros(spec.nw), lbx=bounds[0], ubx=bounds[1], lbg=bounds[2], ubg=bounds[3], p=P.T)
    st = s.stats()["status_code"]
    assert np.all(np.isin(st, (0, 1))), (name, st)
    sol = {k: np.array(sol[k], dtype=np.float64).reshape(-1, B) for k in ("x", "g", "lam_x", "lam_g")}
    return spec, s, B, P, bounds, sol


def _seeds(spec, B, na, seed):
    """(n, na, B) arrays, N(0, 1)."""
    rng = np.random.default_rng(seed)
    return {k: rng.standard_normal((n, na, B)) for k, n in zip(SEEDS, (spec.nw, spec.ng, spec.nX))}


def _prep(spec, sol, bounds, P, seeds, B, na, keys=OUT + ("info", "delta"), g=True, rep=True):
    """Device tensors for Solver.sensitivity_adjoint_device from host data: seeds (n, na, B) or
    (n, na) (shared); bounds (n,) shared (rep: replicated per scenario instead) or (n, B)."""
    import torch

    f64 = dict(dtype=torch.float64, device="cuda")

    def cols(a, n):  # (n,) or (n, B) -> device (n,) or (B, n)
        a = np.asarray(a, dtype=np.float64)
        if a.ndim == 1:
            a = np.repeat(a[:, None], B, axis=1) if rep else a
        return torch.tensor(np.ascontiguousarray(a.T if a.ndim == 2 else a), **f64)

    dsol = {k: cols(sol[k], 0) for k in ("x", "lam_g", "lam_x")}
    if g:
        dsol["g"] = cols(sol["g"], 0)
    db = [cols(v, 0) for v in bounds]
    ds = {k: torch.tensor(np.ascontiguousarray(np.transpose(v, (2, 1, 0)) if v.ndim == 3 else v.T), **f64)
          for k, v in seeds.items()}
    shapes = {"pbar": (B, na, spec.np), "q": (B, na, spec.nw), "jq": (B, na, spec.ng)}
    out = {k: torch.full(shapes[k], 7.0, **f64) for k in keys if k in shapes}
    if "info" in keys:
        out["info"] = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    if "delta" in keys:
        out["delta"] = torch.full((B,), 7.0, **f64)
    return dsol, db, cols(P.T, 0), ds, out


def _device(s, spec, sol, bounds, P, seeds, B, na, **kw):
    """Solver.sensitivity_adjoint_device on host data (see _prep).  Returns numpy arrays in the
    host methods' layout, (n, na, B), and info / delta (B,)."""
    import torch

    dsol, db, dP, ds, out = _prep(spec, sol, bounds, P, seeds, B, na, **kw)
    s.sensitivity_adjoint_device(dsol, *db, dP, out, **ds)
    torch.cuda.synchronize()
    return {k: (np.transpose(v.cpu().numpy(), (2, 1, 0)) if v.dim() == 3 else v.cpu().numpy()) for k, v in out.items()}


def _fused(s, sol, bounds, P, seeds, g=True):
    so = sol if g else {k: v for k, v in sol.items() if k != "g"}
    return s.sensitivity_adjoint_fused(so, *bounds, P.T, **seeds)


def _same(a, b, what, keys=None):
    """Bitwise equality of two results (NaN equal to NaN)."""
    for k in (keys or a):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _ulps(a, b):
    """Largest difference of two arrays in units of the last place of the larger entry."""
    a, b = np.asarray(a, float), np.asarray(b, float)
    m = np.isfinite(a) & np.isfinite(b) & (a != b)
    if not np.any(m):
        return 0.0
    return float(np.max(np.abs(a[m] - b[m]) / np.spacing(np.maximum(np.abs(a[m]), np.abs(b[m])))))


def _against_host(name, got, host, refs, B, na):
    """pbar against the three-launch route's within gate (b): TOL x the sum of the absolute terms
    of pbar (the checker's, at its own q).  Prints the largest difference over the gate per
    scenario before asserting."""
    for b in range(B):
        if refs[b] is None:
            continue
        fig = 0.0
        for a in range(na):
            err = np.abs(got["pbar"][:, a, b] - host["pbar"][:, a, b])
            sc = refs[b]["scale"]["pbar"][a]
            assert np.all(err[sc == 0] == 0.0), (name, b, a)
            fig = max(fig, float(np.max(err[sc > 0] / (ar.TOL * sc[sc > 0]), initial=0.0)))
        print(f"{name} scenario {b}: pbar against the host route, difference / gate (b) {fig:.2e}")
        assert fig <= 1.0, (name, b, fig)


def _g(a, K, b):
    """The gate of one GPU product inside <a, K b>: TOL |a|_1 max_i (|K| |b|)_i."""
    return ar.TOL * float(np.sum(np.abs(a))) * float(np.max(np.abs(K) @ np.abs(b), initial=0.0))


def _bnd(v, b):
    v = np.asarray(v, dtype=np.float64)
    return v if v.ndim == 1 else v[:, b]


def _check(name, prob, got, sol, bounds, P, seeds, B, na, g=None, brf=1e-8):
    """Gates (a) and (b) for every scenario with info 0, against the dense checker at the returned
    delta; returns the checker's per-scenario results."""
    res = []
    for b in range(B):
        if got["info"][b] != 0:
            res.append(None)
            continue
        sd = {k: (seeds[k][:, :, b].T if seeds[k].ndim == 3 else seeds[k].T) for k in seeds}
        ref = sr.dense_adjoint(prob, sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b], P[b],
                               [_bnd(v, b) for v in bounds], delta=got["delta"][b], g=None if g is None else g[:, b],
                               brf=brf, **sd)
        free, ss, dn = ref["free"], ref["ss"], ref["dn"]
        for a in range(na):
            q, jq = got["q"][:, a, b], got["jq"][:, a, b]
            assert np.all(q[~free] == 0.0), (name, b, a)
            rho = kr.rho(ref["M"], q[free], ref["rhs"][a])
            lb = sd["lam_g_bar"][a] if "lam_g_bar" in sd else np.zeros_like(jq)
            own = ar.products_of(dn, y=(ss * (lb - jq))[None], z=-q[None],
                                 Xb=sd["X_bar"][a][None] if "X_bar" in sd else None)
            fig = ar.check_against({"pbar": got["pbar"][:, a, b][None]}, own, f"{name} pbar, scenario {b} seed {a}")
            print(f"{name} scenario {b} seed {a}: rho(q) {rho:.2e} (bound {kr.TOL:.0e}), pbar error / bound "
                  f"{fig['pbar']:.2e}, delta {got['delta'][b]:.3g}, cond(M) {np.linalg.cond(ref['M']):.1e}")
            assert rho <= kr.TOL, (name, b, a, rho)
        res.append(ref)
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_fused_sensitivity_matches_the_checker_and_the_host_route(name):
    """Solved cases (every scenario converges), random x_bar, lam_g_bar, X_bar ~ N(0, 1), na = 2.

    (a) q against the dense M at the returned delta: rho(M, q, r) <= kkt_ref.TOL with
        r = x_bar + Z' X_bar + J' Sigma_s lam_g_bar on the free variables; q = 0 exactly on fixed ones.
    (b) pbar against the checker's dense C' (-q) + Jp' Sigma_s (lam_g_bar - J q) + Xp' X_bar on the
        GPU's own q and J q, within the pbar gate of tests/adjoint_ref.py.
    (c) The adjoint identity against sensitivity(tangent="exact") with dp = I[:, :8], with the bound
        derived in tests/test_gpu_adjoint.py::test_reverse_mode_sensitivity_of_a_solution.
    Against Solver.sensitivity_adjoint, the three launches this one fuses: info and delta are equal;
    q and jq are the same operations on the same weights, right-hand side and factorisation and
    are bitwise equal; pbar takes its tangent from the forward sweep instead of a second prefix
    sum and forms y difference first, and stays within gate (b) of the host's.  The largest
    differences are printed, over the gate per scenario and in ulps."""
    spec, s, B, P, bounds, sol = _solved(name)
    lbx, ubx, lbg, ubg = bounds
    prob = er.problem_of(spec)
    na, nd = 2, 8
    seeds = _seeds(spec, B, na, 71)
    xb, lb, Xb = (seeds[k] for k in SEEDS)
    got = _fused(s, sol, bounds, P, seeds)
    assert got["pbar"].shape == (spec.np, na, B) and got["info"].shape == (B,) and got["delta"].shape == (B,)
    print(f"{name}: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    refs = _check(name, prob, got, sol, bounds, P, seeds, B, na, g=sol["g"])
    # (c)
    dp = np.eye(spec.np)[:, :nd]
    fwd = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="exact")
    np.testing.assert_array_equal(fwd["delta"], got["delta"])
    dXs = (s.products(sol["x"], P.T, fwd["dx"], lam_g=sol["lam_g"])["dX"]
           + s.param_products(sol["x"], P.T, dp, lam_g=sol["lam_g"])["dXp"])
    for b in range(B):
        ref = refs[b]
        dn, ss, free = ref["dn"], ref["ss"], ref["free"]
        J, Z, Cm, Jp, Xp = dn["J"], dn["Z"], dn["C"], dn["Jp"], dn["Xp"]
        aMf = np.abs(ref["M"])
        T = -(Cm @ dp) - J.T @ (ss[:, None] * (Jp @ dp))
        for a in range(na):
            q = got["q"][:, a, b]
            den_q = float(np.max(aMf @ np.abs(q[free]))) + float(np.max(np.abs(ref["rhs"][a])))
            worst = 0.0
            for j in range(nd):
                dx, dl = fwd["dx"][:, j, b], fwd["dlam_g"][:, j, b]
                D = (xb[:, a, b] @ dx + lb[:, a, b] @ dl + Xb[:, a, b] @ dXs[:, j, b]) - got["pbar"][:, a, b] @ dp[:, j]
                den_x = float(np.max(aMf @ np.abs(dx[free]))) + float(np.max(np.abs(T[free, j])))
                bound = kr.TOL * (np.sum(np.abs(q)) * den_x + np.sum(np.abs(dx)) * den_q)
                bound += 2 * (_g(q, Cm, dp[:, j]) + _g(ss * (np.abs(lb[:, a, b]) + np.abs(J) @ np.abs(q)), Jp, dp[:, j])
                              + _g(ss * lb[:, a, b], J, dx) + _g(Xb[:, a, b], Z, dx) + _g(Xb[:, a, b], Xp, dp[:, j]))
                if bound == 0.0:  # an entry of p that nothing reads
                    assert D == 0.0, (name, b, a, j, D)
                    continue
                worst = max(worst, abs(D) / bound)
                assert abs(D) <= bound, (name, b, a, j, D, bound)
            print(f"{name} scenario {b} seed {a}: adjoint identity defect / bound {worst:.2e}")
    # the parent's route
    host = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, **seeds)
    np.testing.assert_array_equal(got["info"], host["info"])
    np.testing.assert_array_equal(got["delta"], host["delta"])
    print(f"{name} against sensitivity_adjoint, largest difference in ulps: "
          + ", ".join(f"{k} {_ulps(got[k], host[k]):.1f}" for k in OUT))
    _same(got, host, f"{name} against the host route", ("q", "jq"))
    _against_host(name, got, host, refs, B, na)


def test_the_ladder_runs_in_the_kernel():
    """With first_hessian_perturbation = 1e-12 on the handle: at the solved points M is singular
    rather than indefinite at delta = 0 (the last heading-rate control has no cost, row or active
    bound), so the first rung already factorises -- delta = 1e-12 in the kernel and on the host;
    at synthetic points (random multipliers: M indefinite) many rungs are needed (1e-12, 1e-10,
    8e-10, ...), and delta equals the host ladder's exactly, scenario by scenario, with q, jq the
    host's bits.  With max_hessian_perturbation below the first rung a scenario whose M does not
    factorise at delta = 0 keeps info = 1, the delta it was last tried at and NaN in pbar, q, jq;
    a scenario that factorises at 0 (here: one whose undetermined last stage is fixed through its
    bounds) is bitwise what it is under the default ladder."""
    spec, s0, B, P, bounds, sol = _solved("race_track_2")
    lbx, ubx, lbg, ubg = bounds
    na = 2
    seeds = _seeds(spec, B, na, 73)
    s = _solver(spec, first_hessian_perturbation=1e-12)
    rungs = [1e-12, 100.0 * 1e-12]
    for _ in range(60):
        rungs.append(8.0 * rungs[-1])
    got = _fused(s, sol, bounds, P, seeds)
    host = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, **seeds)
    print(f"ladder from 1e-12, solved points: info {got['info']}, delta {got['delta']}, host delta {host['delta']}")
    _same(got, host, "ladder from 1e-12", ("info", "delta", "q", "jq"))
    assert np.all(got["info"] == 0) and all(d in rungs for d in got["delta"]), got["delta"]
    Bs = er.CASES["race_track_2"]
    d = er.draw_point(spec, Bs, seed=33)
    syn = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    syn["g"] = s.evaluate(syn["x"], d["p"].T)["g"]
    sds = _seeds(spec, Bs, na, 74)
    got = _fused(s, syn, bounds, d["p"], sds)
    host = s.sensitivity_adjoint(syn, lbx, ubx, lbg, ubg, d["p"].T, **sds)
    print(f"ladder from 1e-12, synthetic points: info {got['info']}, delta {got['delta']}, host delta {host['delta']}")
    _same(got, host, "ladder from 1e-12, synthetic points", ("info", "delta", "q", "jq"))
    assert np.all(got["info"] == 0) and all(dl in rungs for dl in got["delta"]), got["delta"]  # the same products
    climbed = [rungs.index(dl) + 1 for dl in got["delta"]]
    print(f"rungs climbed: {climbed}")
    assert max(climbed) >= 3
    # no rung allowed: per-scenario bounds, scenario 0 with its last stage fixed at the solution
    nu = spec.nw // spec.N
    lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb2[-nu:, 0] = ub2[-nu:, 0] = sol["x"][-nu:, 0]
    b2 = (lb2, ub2, lbg, ubg)
    ref = _fused(s0, sol, b2, P, seeds)
    cut = _solver(spec, max_hessian_perturbation=1e-6)
    got = _fused(cut, sol, b2, P, seeds)
    hst = cut.sensitivity_adjoint(sol, lb2, ub2, lbg, ubg, P.T, **seeds)
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
    print(f"scenarios that factorise at delta = 0: {int(np.sum(~stuck))} of {B}")


def test_batch_plumbing():
    """All bitwise unless said: every subset of the seeds equals all three with zeros in place of
    the absent ones (as numbers: a zero may change its sign); na = 3 equals three na = 1 calls;
    leading dimension 0 for the bounds and the seeds equals the replicated call; the host and the
    device entry point agree, for every subset of the outputs; a NaN in one seed leaves the other
    seeds' bits unchanged; with g NULL the weights come from the kernel's own g(x, p), and the
    result (difference printed: active slacks are floored, so it is at rounding level) passes the
    same gates."""
    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    na = 3
    seeds = _seeds(spec, B, na, 75)
    full = _fused(s, sol, bounds, P, seeds)
    assert np.all(full["info"] == 0)
    dev = _device(s, spec, sol, bounds, P, seeds, B, na)
    _same(dev, full, "device against host entry point")
    for sub in SUBSETS:
        part = _fused(s, sol, bounds, P, {k: seeds[k] for k in sub})
        zero = _fused(s, sol, bounds, P, {k: (seeds[k] if k in sub else np.zeros_like(seeds[k])) for k in SEEDS})
        _same(part, zero, f"seeds {sub} against zeros for the rest")
        _same(_device(s, spec, sol, bounds, P, {k: seeds[k] for k in sub}, B, na), part, f"device, seeds {sub}")
    for a in range(na):
        one = _fused(s, sol, bounds, P, {k: v[:, a:a + 1] for k, v in seeds.items()})
        for k in OUT:
            np.testing.assert_array_equal(one[k][:, 0], full[k][:, a], err_msg=f"{k} seed {a}")
        _same(one, full, f"seed {a}", ("info", "delta"))
    # leading dimension 0: shared seeds and bounds against replicated ones
    sh = {k: np.ascontiguousarray(v[:, :, 0]) for k, v in seeds.items()}
    rep = {k: np.repeat(v[:, :, None], B, axis=2) for k, v in sh.items()}
    shared = _device(s, spec, sol, bounds, P, sh, B, na, rep=False)
    _same(shared, _device(s, spec, sol, bounds, P, rep, B, na, rep=True), "ld = 0")
    _same(shared, _fused(s, sol, bounds, P, sh), "ld = 0, host entry point")
    # subsets of the outputs
    for keys in (("pbar",), ("q",), ("q", "jq", "info"), ("pbar", "delta")):
        part = _device(s, spec, sol, bounds, P, seeds, B, na, keys=keys)
        _same(part, full, f"outputs {keys}")
    # a NaN entry poisons its own seed only
    for sk, idx in (("x_bar", 6), ("lam_g_bar", 7), ("X_bar", 11)):
        bad = dict(seeds, **{sk: seeds[sk].copy()})
        bad[sk][idx, 1, :] = np.nan
        poisoned = _fused(s, sol, bounds, P, bad)
        for k in OUT:
            np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=f"{k}, NaN in {sk}")
        assert np.all(np.any(np.isnan(poisoned["pbar"][:, 1]), axis=0)), sk
        _same(poisoned, full, f"NaN in {sk}", ("info", "delta"))
    # g NULL
    own = _fused(s, sol, bounds, P, seeds, g=False)
    _same(own, full, "g NULL", ("info", "delta"))
    print("g NULL against the solve's g_out, largest difference in ulps: "
          + ", ".join(f"{k} {_ulps(own[k], full[k]):.1f}" for k in OUT)
          + ", relative: " + ", ".join(f"{k} {float(np.max(np.abs(own[k] - full[k])) / np.max(np.abs(full[k]))):.1e}" for k in OUT))
    _check("race_track_2, g NULL", prob, own, sol, bounds, P, seeds, B, na, g=None)


def test_fixed_controls_equality_rows_and_invalid_bounds():
    """A third of the controls fixed through lbx == ubx, a whole stage among them: q is exactly 0
    there, gates (a) and (b) hold on the free ones, and the host route gives the same info, delta,
    q and jq.  An equality row (lbg == ubg) in one scenario, lbx > ubx in another and a NaN
    multiplier in a third give info -11, delta 0 and NaN for those scenarios; the remaining one is
    bitwise what it is without them.  The host wrapper raises on equality rows."""
    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    lbx, ubx, lbg, ubg = bounds
    na = 2
    seeds = _seeds(spec, B, na, 77)
    rng = np.random.default_rng(78)
    fx = rng.uniform(size=(spec.nw, B)) < 1.0 / 3.0
    nu = spec.nw // spec.N
    fx[:nu, 0] = True  # a whole stage
    lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb2[fx], ub2[fx] = sol["x"][fx], sol["x"][fx]
    b2 = (lb2, ub2, lbg, ubg)
    got = _fused(s, sol, b2, P, seeds)
    print(f"fixed controls: {fx.sum(axis=0)} of {spec.nw}, info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    for b in range(B):
        assert np.all(got["q"][fx[:, b], :, b] == 0.0), b
    refs = _check("fixed controls", prob, got, sol, b2, P, seeds, B, na, g=sol["g"])
    assert all(np.array_equal(r["free"], ~fx[:, b]) for b, r in enumerate(refs))
    host = s.sensitivity_adjoint(sol, lb2, ub2, lbg, ubg, P.T, **seeds)
    _same(got, host, "fixed controls against the host route", ("info", "delta", "q", "jq"))
    # invalid scenarios
    full = _device(s, spec, sol, bounds, P, seeds, B, na)
    lg2, ug2 = (np.repeat(v[:, None], B, axis=1) for v in (lbg, ubg))
    lg2[spec.ng // 2, 0] = ug2[spec.ng // 2, 0]
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb3[5, 1] = ub3[5, 1] + 1.0
    sol3 = dict(sol, lam_g=sol["lam_g"].copy())
    sol3["lam_g"][3, 2] = np.nan
    got = _device(s, spec, sol3, (lb3, ub3, lg2, ug2), P, seeds, B, na)
    print(f"invalid scenarios: info {got['info']}, delta {got['delta']}")
    np.testing.assert_array_equal(got["info"], [-11, -11, -11, 0])
    np.testing.assert_array_equal(got["delta"][:3], 0.0)
    for k in OUT:
        assert np.all(np.isnan(got[k][:, :, :3])), k
        np.testing.assert_array_equal(got[k][:, :, 3], full[k][:, :, 3], err_msg=k)
    assert got["delta"][3] == full["delta"][3]
    with pytest.raises(ValueError):
        s.sensitivity_adjoint_fused(sol, lbx, ubx, lg2, ug2, P.T, **seeds)
    with pytest.raises(ValueError):
        s.sensitivity_adjoint_fused(sol, lbx, ubx, lbg, ubg, P.T)


@pytest.mark.parametrize("name", ["n1", "n63_16obs"])
def test_synthetic_points_on_the_smallest_and_largest_shape(name):
    """Random x inside the bounds and random signed multipliers (tests/eval_ref.draw_point), N = 1
    and N = 63 with 16 obstacles (every lane, every row slot): info, delta, q and jq equal the
    three-launch route's exactly, pbar within gate (b) of it, every point factorises along the
    ladder (n63_16obs climbs to delta = 327.68 and 2,621.44), and gates (a), (b) hold against the
    dense checker."""
    spec = er.case_spec(name)
    prob = er.problem_of(spec)
    s = _solver(spec)
    B, na = er.CASES[name], 2
    d = er.draw_point(spec, B, seed=31)
    bounds = (d["lbx"], d["ubx"], d["lbg"], d["ubg"])
    P = d["p"]
    sol = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    sol["g"] = s.evaluate(sol["x"], P.T)["g"]
    seeds = _seeds(spec, B, na, 32)
    got = _fused(s, sol, bounds, P, seeds, g=False)
    host = s.sensitivity_adjoint(sol, *bounds, P.T, **seeds)
    print(f"{name}: info {got['info']}, delta {got['delta']}; largest difference in ulps: "
          + ", ".join(f"{k} {_ulps(got[k], host[k]):.1f}" for k in OUT))
    _same(got, host, f"{name} against the host route", ("info", "delta", "q", "jq"))
    assert np.all(got["info"] == 0), got["info"]  # every point factorises along the ladder
    refs = _check(name, prob, got, sol, bounds, P, seeds, B, na, g=None)
    _against_host(name, got, host, refs, B, na)


def test_sensitivity_adjoint_device_does_not_synchronise():
    """nmpc_solve_adjoint_batch_dev only enqueues (the pattern of tests/test_gpu_adjoint.py::
    test_adjoint_products_device_does_not_synchronise): behind a spinning kernel on a side stream
    the call returns while the stream is still busy, and the results equal an unobstructed run's.
    After a solve of the same B it allocates nothing."""
    import time
    import torch

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    na = 2
    seeds = _seeds(spec, B, na, 79)
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    ref = _device(s, spec, sol, bounds, P, seeds, B, na)
    assert s.memory_info() == mem  # the solve's workspace covers the launch
    dsol, db, dP, ds, o = _prep(spec, sol, bounds, P, seeds, B, na)
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
    s.sensitivity_adjoint_device(dsol, *db, dP, o, stream=st, **ds)
    call_ms = (time.perf_counter() - t0) * 1e3
    busy = not st.query()
    torch.cuda.synchronize()
    spin_ms = e0.elapsed_time(e1)
    print(f"sensitivity_adjoint_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info() == mem
    for k in OUT:
        np.testing.assert_array_equal(np.transpose(o[k].cpu().numpy(), (2, 1, 0)), ref[k], err_msg=k)
    np.testing.assert_array_equal(o["info"].cpu().numpy(), ref["info"])
    np.testing.assert_array_equal(o["delta"].cpu().numpy(), ref["delta"])


def test_argument_validation_on_a_live_handle():
    """B <= 0, na <= 0, a NULL required pointer, every seed NULL, pbar_out and q_out both NULL and
    a leading dimension that is neither 0 nor >= the vector length return NMPC_E_INVALID from both
    entry points before any device call: nothing is written, and the handle still works."""
    from nmpc_amd import _lib

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    L = _lib.lib()
    na = 2
    nw, ng, npp, nX = spec.nw, spec.ng, spec.np, spec.nX
    sd = _seeds(spec, B, na, 80)
    arr = {"x": sol["x"].T, "p": P, "lam_g": sol["lam_g"].T, "lam_x": sol["lam_x"].T, "g": sol["g"].T,
           "lbx": np.repeat(bounds[0][None], B, 0), "ubx": np.repeat(bounds[1][None], B, 0),
           "lbg": np.repeat(bounds[2][None], B, 0), "ubg": np.repeat(bounds[3][None], B, 0),
           "x_bar": np.transpose(sd["x_bar"], (2, 1, 0)), "lam_g_bar": np.transpose(sd["lam_g_bar"], (2, 1, 0)),
           "X_bar": np.transpose(sd["X_bar"], (2, 1, 0))}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    arr.update(pbar=np.full((B, na, npp), 7.0), q=np.full((B, na, nw), 7.0), jq=np.full((B, na, ng), 7.0),
               delta=np.full(B, 7.0))
    info = np.full(B, 99, dtype=np.int32)
    names = ("x", "p", "lam_g", "lam_x", "g", "lbx", "ubx", "lbg", "ubg", "x_bar", "lam_g_bar", "X_bar")
    lens = dict(zip(names, (nw, npp, ng, nw, ng, nw, nw, ng, ng, nw * na, ng * na, nX * na)))
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)

    def call(B_=B, na_=na, null=(), ld=None, dev=False):
        ld = dict(lens, **(ld or {}))
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k not in null else vp(0)  # noqa: E731
            gi = vp(info.ctypes.data)
        else:
            g = lambda k: arr[k].ctypes.data_as(dp) if k not in null else None  # noqa: E731
            gi = info.ctypes.data_as(ip)
        args = [s._h, B_, na_]
        for k in names:
            args += [g(k), ld[k]]
        args += [g("pbar"), g("q"), g("jq"), gi, g("delta")]
        return L.nmpc_solve_adjoint_batch_dev(*args, vp(0)) if dev else L.nmpc_solve_adjoint_batch(*args)

    # each with the full message of its rule; the last four break two rules at once: the earlier
    # one in the order of the checks answers
    req, ldm = "required pointer is null (x, p, lam_g, lam_x, lbx, ubx, lbg, ubg)", "leading dimension smaller than the vector length"
    seeds, outs = "every seed pointer is null (x_bar, lam_g_bar, X_bar)", "both pbar_out and q_out are null"
    no_seed = ("x_bar", "lam_g_bar", "X_bar")
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("na = 0", dict(na_=0), "na <= 0"),
                 ("na < 0", dict(na_=-1), "na <= 0"), ("every seed NULL", dict(null=no_seed), seeds),
                 ("pbar and q NULL", dict(null=("pbar", "q")), outs), ("ld_x negative", dict(ld={"x": -nw}), ldm),
                 ("ld_x_bar one seed", dict(ld={"x_bar": nw}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in names[:9] if k != "g"]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and na = 0", dict(B_=0, na_=0), "B <= 0"), ("na = 0 and x NULL", dict(na_=0, null=("x",)), "na <= 0"),
                  ("ubg NULL and no seed", dict(null=("ubg",) + no_seed), req),
                  ("no seed and no output", dict(null=no_seed + ("pbar", "q")), seeds),
                  ("no output and ld_p short", dict(null=("pbar", "q"), ld={"p": npp - 1}), outs)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error(), what
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    call(null=("x_bar", "lam_g_bar", "X_bar"))
    assert "seed" in L.nmpc_last_error().decode()
    call(null=("pbar", "q"))
    assert "pbar_out" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(na_=0))
    assert all(np.all(arr[k] == 7.0) for k in OUT + ("delta",)) and np.all(info == 99)  # nothing ran
    # and the handle still works: one seed, g NULL, q alone; leading dimension 0 shares everything
    assert call(null=("lam_g_bar", "X_bar", "g", "pbar", "jq", "delta")) == 0
    assert np.all(np.isfinite(arr["q"])) and np.all(info == 0) and np.all(arr["pbar"] == 7.0) and np.all(arr["jq"] == 7.0)
    assert call(ld={k: 0 for k in names}) == 0
    for k in OUT:
        assert np.all(np.isfinite(arr[k]))
        for b in range(1, B):
            np.testing.assert_array_equal(arr[k][0], arr[k][b])


def test_autograd_with_the_backward_pass_on_the_device(monkeypatch):
    """nmpc_amd.autograd.solve(backward="device"): the gradient of a random linear loss on (x, X)
    agrees with backward="host" within gate (b) (TOL x the sum of the absolute terms of pbar at
    the host route's q); a loss on x alone seeds nothing on X; with max_iter = 1 every
    row is NaN; and with Solver.sensitivity_adjoint and torch.Tensor.cpu made to raise, forward
    plus backward still complete: nothing in them reads a value back."""
    import torch
    from nmpc_amd import autograd
    from nmpc_amd.nlpsol import Solver
    from oracle import nmpc_oracle as orc

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    prob = er.problem_of(spec)
    lbx, ubx, lbg, ubg = bounds
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(72)
    cx, cX = rng.standard_normal((B, spec.nw)), rng.standard_normal((B, spec.nX))
    tcx, tcX = torch.tensor(cx, **f64), torch.tensor(cX, **f64)
    grads = {}
    for mode in ("host", "device"):
        p = torch.tensor(P, requires_grad=True, **f64)
        x, X = autograd.solve(s, p, lbx, ubx, lbg, ubg, backward=mode)
        (g,) = torch.autograd.grad((tcx * x).sum() + (tcX * X).sum(), p)
        grads[mode] = g.cpu().numpy()
        np.testing.assert_array_equal(x.detach().cpu().numpy().T, sol["x"])
    assert np.all(np.isfinite(grads["host"]))
    r = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=cx.T[:, None, :], X_bar=cX.T[:, None, :])
    np.testing.assert_array_equal(grads["host"], r["pbar"][:, 0, :].T)

    def gate(gdev, rh, Xbar):
        """|gdev - host| over gate (b): TOL x the scale at the host route's q, jq."""
        worst = 0.0
        for b in range(B):
            ev = orc.SSEval(prob, sol["x"][:, b], P[b])
            dn = ar.dense(ev, 1.0, sol["lam_g"][:, b])
            ss = kr.barrier_weights(sol["g"][:, b], sol["lam_g"][:, b], lbg, ubg)
            sc = ar.products_of(dn, y=-(ss * rh["jq"][:, 0, b])[None], z=-rh["q"][:, 0, b][None],
                                Xb=None if Xbar is None else Xbar[b][None])["scale"]["pbar"][0]
            err = np.abs(gdev[b] - rh["pbar"][:, 0, b])
            assert np.all(err[sc == 0] == 0.0)
            worst = max(worst, float(np.max(err[sc > 0] / (ar.TOL * sc[sc > 0]))))
        return worst

    worst = gate(grads["device"], r, cX)
    print(f"autograd, backward on the device against the host route: error / bound {worst:.2e}, "
          f"{_ulps(grads['device'], grads['host']):.1f} ulps")
    assert worst <= 1.0
    with pytest.raises(ValueError):
        autograd.solve(s, torch.tensor(P, **f64), lbx, ubx, lbg, ubg, backward="fused")
    # no scenario converges in one iteration: NaN rows, never zeros
    s1 = _solver(spec, max_iter=1)
    p1 = torch.tensor(P, requires_grad=True, **f64)
    x1, X1 = autograd.solve(s1, p1, lbx, ubx, lbg, ubg, backward="device")
    (g1,) = torch.autograd.grad((tcx * x1).sum() + (tcX * X1).sum(), p1)
    assert np.all(np.isnan(g1.cpu().numpy()))
    # nothing is read back
    def boom(*a, **k):
        raise AssertionError("a host round trip in the device route")

    p2 = torch.tensor(P, requires_grad=True, **f64)
    with monkeypatch.context() as m:
        m.setattr(Solver, "sensitivity_adjoint", boom)
        m.setattr(torch.Tensor, "cpu", boom)
        x2, X2 = autograd.solve(s, p2, lbx, ubx, lbg, ubg, backward="device")
        (g2,) = torch.autograd.grad((tcx * x2).sum(), p2)
    gx = g2.cpu().numpy()
    assert np.all(np.isfinite(gx))
    rx = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=cx.T[:, None, :])
    worst = gate(gx, rx, None)
    print(f"autograd, loss on x alone: error / bound {worst:.2e}, {_ulps(gx, rx['pbar'][:, 0, :].T):.1f} ulps")
    assert worst <= 1.0
