"""The fp32 leg's linear algebra at given points, on the GPU: Solver::riccati -> resolve -> forward
-> refine -> refine of the kernel classes CapC (fp64 control), CapC32 (fp32 factors, global rows)
and CapA32 (fp32 factors, LDS rows, N <= 20, 15 rows per stage) through the probe
(tests/probe/nmpc_probe.hip: nmpc_probe_lq_step), against the dense condensed KKT matrix of
tests/kkt_ref.py.  The bounds come from the float32 restatement of tests/fp32_ref.py alone
(re-measured by tests/test_fp32_step.py), never from the kernel; every figure is printed before it
is asserted."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_ref as er
from tests import fp32_ref as fr
from tests import kkt_ref as kr

pytestmark = pytest.mark.gpu

FP32 = ("C32", "A32")
CAPACITY = {"C": (63, 21), "C32": (63, 21), "A32": (20, 15)}  # N, rows per stage (tests/probe/build.py)


def _fits(cls, name):
    spec = er.case_spec(name)
    return spec.N <= CAPACITY[cls][0] and spec.ng // (spec.N + 1) <= CAPACITY[cls][1]


# every case for CapC32 (n63_16obs at its capacity, n1), the cases within N <= 20 and 15 rows for CapA32
FP32_CASES = [(cls, name) for cls in FP32 for name in er.CASES if _fits(cls, name)]


def _desc(spec):
    """The problem description nlpsol hands to nmpc_create (nmpc_amd/nlpsol.py), default options."""
    from nmpc_amd import _lib

    d = _lib.Desc()
    d.model = 1 if spec.model == "uav5" else 0
    d.N, d.np, d.n_obs = spec.N, spec.np, spec.n_obs
    d.T, d.w1, d.w2, d.vfov, d.hfov = spec.T, spec.w1, spec.w2, spec.vfov, spec.hfov
    for j, ob in enumerate(spec.obstacles):
        d.obs_x[j], d.obs_y[j], d.obs_rsum[j] = ob.x, ob.y, ob.r
        d.obs_x_pidx[j], d.obs_y_pidx[j] = ob.x_pidx, ob.y_pidx
    d.w1_pidx, d.w2_pidx = spec.w1_pidx, spec.w2_pidx
    return d


def _step(cls, spec, inp, sel=slice(None), **over):
    """dw (3, B, NR, nw), dX (3, B, NR, nX), info (B): the step after forward, one and two
    refinements; the absent controls' entries of the kernel's own layout must be exactly 0."""
    from tests.probe import build as pb

    a = {k: inp[k][sel] for k in ("x", "p", "lam_g", "sigma_x", "sigma_s", "delta", "r_w", "r_g")}
    a.update(over)
    a = {k: np.ascontiguousarray(v, dtype=float) for k, v in a.items()}
    B, nr = a["x"].shape[0], a["r_w"].shape[1]
    assert a["x"].shape == (B, spec.nw) and a["p"].shape == (B, spec.np) and a["lam_g"].shape == (B, spec.ng)
    assert a["sigma_x"].shape == (B, spec.nw) and a["sigma_s"].shape == (B, spec.ng) and a["delta"].shape == (B,)
    assert a["r_w"].shape == (B, nr, spec.nw) and a["r_g"].shape == (B, nr, spec.ng)
    dw, dX = np.full((3, B, nr, spec.nw), 7.0), np.full((3, B, nr, spec.nX), 7.0)
    du = np.full((3, B, nr, spec.N, 6), 7.0)
    info = np.full(B, 9, dtype=np.int32)
    dp = C.POINTER(C.c_double)
    ptr = lambda v: v.ctypes.data_as(dp)  # noqa: E731
    d = _desc(spec)
    rc = pb.lib().nmpc_probe_lq_step(pb.LQ_CLASSES[cls], C.byref(d), B, nr, ptr(a["x"]), ptr(a["p"]), ptr(a["lam_g"]),
                                     float(inp["obj_factor"]), ptr(a["sigma_x"]), ptr(a["sigma_s"]), ptr(a["delta"]),
                                     ptr(a["r_w"]), ptr(a["r_g"]), ptr(dw), ptr(dX), ptr(du), info.ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, f"nmpc_probe_lq_step({cls}): HIP error {rc}"
    nu = spec.nw // spec.N
    fin = info == 0
    assert pb.LQ_CAPACITY == CAPACITY
    np.testing.assert_array_equal(du[:, fin, :, :, :nu].reshape(3, int(fin.sum()), nr, spec.nw), dw[:, fin])
    assert np.all(du[:, fin, :, :, nu:] == 0.0), f"{cls}: an absent control has a step"
    assert np.all(np.isnan(du[:, ~fin]))
    return dw, dX, info


def _kkt_solve(spec, inp):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    t = lambda a: np.ascontiguousarray(np.transpose(a, (2, 1, 0)))  # noqa: E731
    res = s.kkt_solve(inp["x"].T, inp["p"].T, r_w=t(inp["r_w"]), r_g=t(inp["r_g"]), lam_g=inp["lam_g"].T,
                      obj_factor=inp["obj_factor"], sigma_x=inp["sigma_x"].T, sigma_s=inp["sigma_s"].T, delta=inp["delta"])
    return np.transpose(res["dw"], (2, 1, 0)), np.transpose(res["dX"], (2, 1, 0)), res["info"]


def test_the_probe_refuses_a_shape_beyond_the_class():
    """CapA32 holds N <= 20 and 15 rows per stage: a larger problem is refused before any launch."""
    spec, inp, per, evs = kr.reference("n63_16obs", "mild", kr.COMBOS[0])
    from tests.probe import build as pb

    d = _desc(spec)
    z = np.zeros(8)
    p = z.ctypes.data_as(C.POINTER(C.c_double))
    rc = pb.lib().nmpc_probe_lq_step(pb.LQ_CLASSES["A32"], C.byref(d), 1, 1, p, p, p, 1.0, p, p, p, p, p, p, p, p,
                                     np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 1  # hipErrorInvalidValue
    assert np.all(z == 0.0)


@pytest.mark.parametrize("regime", kr.REGIMES)
@pytest.mark.parametrize("name", list(er.CASES))
def test_fp64_control(name, regime):
    """CapC through the probe's restated setup: rho <= 1e-10 against the dense M in both regimes,
    the forward error as kkt_ref.check_solution gates it, and the step equal to
    Solver.kkt_solve's.  refine compiles to nothing for an fp64 class: the three steps are bitwise
    equal.  Against kkt_solve the gate is 1e-12 relative; expected, and printed, is bitwise
    equality (the same expressions in the same order on the same device functions)."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, regime, combo)
        dw, dX, info = _step("C", spec, inp)
        assert np.all(info == 0), info
        np.testing.assert_array_equal(dw[0], dw[1])
        np.testing.assert_array_equal(dw[0], dw[2])
        np.testing.assert_array_equal(dX[0], dX[1])
        np.testing.assert_array_equal(dX[0], dX[2])
        kdw, kdX, kinfo = _kkt_solve(spec, inp)
        assert np.all(kinfo == 0)
        for b in range(er.CASES[name]):
            what = f"{name} {regime} obj {combo[0]} scenario {b} CapC"
            kr.check_solution(dw[0, b], per[b], regime, what)
            _check_dX(evs[b], dw[0, b], dX[0, b], what)
            rel = float(np.max(np.abs(dw[0, b] - kdw[b])) / np.max(np.abs(kdw[b])))
            relX = float(np.max(np.abs(dX[0, b] - kdX[b])) / max(np.max(np.abs(kdX[b])), 1e-300))
            print(f"{what}: against kkt_solve dw {rel:.2e}, dX {relX:.2e} (bound 1e-12), bitwise "
                  f"{np.array_equal(dw[0, b], kdw[b]) and np.array_equal(dX[0, b], kdX[b])}")
            assert rel <= 1e-12 and relX <= 1e-12, (what, rel, relX)


@pytest.mark.parametrize("regime", fr.GATED)
@pytest.mark.parametrize("cls,name", FP32_CASES)
def test_fp32_step_and_refinement(cls, name, regime):
    """Per case, at both combos: rho(dw0) <= 30 rho0_ref (the fp32 factorisation is sound),
    rho(dw1) <= bound1 and rho(dw2) <= bound2 (the refinement is exact to the restatement's
    level), and rho(dw1) < rho(dw0) on every column (the refinement did work).  dX is the
    oracle's Z applied to the GPU's own dw at every stage of the refinement.  uav5: the absent
    gimbal controls' steps are exactly 0 before and after each refinement (_step)."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, regime, combo)
        ref, bd = fr.bounds(name, regime, combo)
        dw, dX, info = _step(cls, spec, inp)
        assert np.all(info == 0), info
        worst = np.zeros(3)
        for b in range(er.CASES[name]):
            r = fr.rhos([dw[0, b], dw[1, b], dw[2, b]], per[b])
            worst = np.maximum(worst, np.max(r, axis=1))
            print(f"{cls} {name} {regime} obj {combo[0]} scenario {b}: rho {np.max(r[0]):.2e} / {np.max(r[1]):.2e} / "
                  f"{np.max(r[2]):.2e}, columns improved {np.sum(r[1] < r[0])} of {kr.NR}")
        print(f"{cls} {name} {regime} obj {combo[0]}: rho0/1/2 {worst[0]:.2e} {worst[1]:.2e} {worst[2]:.2e}; reference "
              f"{ref[0]:.2e} {ref[1]:.2e} {ref[2]:.2e}; bounds {bd[0]:.2e} {bd[1]:.2e} {bd[2]:.2e}; "
              f"of bound {worst[0] / bd[0]:.2f} {worst[1] / bd[1]:.2f} {worst[2] / bd[2]:.2f}")
        for b in range(er.CASES[name]):
            r = fr.rhos([dw[0, b], dw[1, b], dw[2, b]], per[b])
            assert np.all(r[0] <= bd[0]), (cls, name, regime, combo, b, "rho0", r[0], bd[0])
            assert np.all(r[1] <= bd[1]), (cls, name, regime, combo, b, "rho1", r[1], bd[1])
            assert np.all(r[2] <= bd[2]), (cls, name, regime, combo, b, "rho2", r[2], bd[2])
            assert np.all(r[1] < r[0]), (cls, name, regime, combo, b, "no gain", r[0], r[1])
            for t in range(3):
                _check_dX(evs[b], dw[t, b], dX[t, b], f"{cls} {name} {regime} scenario {b} step {t}")


def _check_dX(ev, dw, dX, what):
    """dX against Z dw of the oracle within 1e-10 of the absolute-product scale
    (kkt_ref.check_steps' dX gate; the refinement adds two fp64 sweeps, far below it)."""
    Z = kr.pr.stack_Z(ev)
    ref, scale = dw @ Z.T, np.max(np.abs(dw) @ np.abs(Z).T, axis=1)
    err = np.max(np.abs(dX - ref), axis=1)
    q = np.where(scale > 0, err / np.where(scale > 0, kr.TOL * scale, 1.0), np.where(err == 0, 0.0, np.inf))
    assert np.all(q <= 1.0), (what, q)


@pytest.mark.parametrize("cls,name", FP32_CASES)
def test_barrier_regime_is_recorded(cls, name):
    """cond(M) up to 1e15: recorded, not gated.  Where the restatement's float32 Cholesky and the
    kernel's verdict both succeed, rho0/1/2 of both are printed; where either fails, which.
    Asserted: a scenario whose verdict is not 0 returns NaN steps, and its neighbours are bitwise
    what the same batch gives without it."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, "barrier", combo)
        rr, ok = fr.case_figures(name, "barrier", combo)
        dw, dX, info = _step(cls, spec, inp)
        B = er.CASES[name]
        for b in range(B):
            what = f"{cls} {name} barrier obj {combo[0]} scenario {b} (cond {per[b]['cond']:.1e})"
            if info[b] == 0 and ok[b]:
                r = np.max(fr.rhos([dw[0, b], dw[1, b], dw[2, b]], per[b]), axis=1)
                print(f"{what}: kernel rho {r[0]:.1e} / {r[1]:.1e} / {r[2]:.1e}, restatement {rr[b, 0]:.1e} / "
                      f"{rr[b, 1]:.1e} / {rr[b, 2]:.1e}")
            else:
                print(f"{what}: kernel verdict {info[b]}, restatement's float32 Cholesky {'succeeds' if ok[b] else 'fails'}")
            assert info[b] in (0, 1)
            if info[b] != 0:
                assert np.all(np.isnan(dw[:, b])) and np.all(np.isnan(dX[:, b]))
        failed = np.flatnonzero(info != 0)
        if failed.size and failed.size < B:
            keep = np.flatnonzero(info == 0)
            dw2, dX2, info2 = _step(cls, spec, inp, keep)
            assert np.all(info2 == 0)
            np.testing.assert_array_equal(dw2, dw[:, keep])
            np.testing.assert_array_equal(dX2, dX[:, keep])


def test_a_failed_factorisation_ends_its_scenario_only():
    """The barrier regime need not produce a failed verdict on every class: here one scenario of
    a mild batch gets sigma = 0, delta = 0 and the multipliers of kkt_ref.indefinite_cases (dense
    M indefinite beyond the judged margin).  Verdict 1, NaN steps; the neighbours bitwise as in
    the batch without it -- for all three classes."""
    name = "race_track_2"
    spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[0])
    _, ind, ratio = kr.indefinite_cases(name)
    bad = int(np.flatnonzero(ratio < -kr.INDEF)[0])
    B = er.CASES[name]
    sx, ss, dl, lam = inp["sigma_x"].copy(), inp["sigma_s"].copy(), inp["delta"].copy(), inp["lam_g"].copy()
    sx[bad], ss[bad], dl[bad], lam[bad] = 0.0, 0.0, 0.0, ind["lam_g"][bad]
    x, p = inp["x"].copy(), inp["p"].copy()
    x[bad], p[bad] = ind["x"][bad], ind["p"][bad]
    keep = np.array([b for b in range(B) if b != bad])
    for cls in ("C",) + FP32:
        dw, dX, info = _step(cls, spec, inp, x=x, p=p, lam_g=lam, sigma_x=sx, sigma_s=ss, delta=dl)
        print(f"{cls}: lambda_min / max|M| of scenario {bad} {ratio[bad]:.2e}, verdicts {info}")
        assert info[bad] == 1 and np.all(np.isnan(dw[:, bad])) and np.all(np.isnan(dX[:, bad]))
        assert np.all(info[keep] == 0)
        dw2, dX2, info2 = _step(cls, spec, inp, keep)
        np.testing.assert_array_equal(dw2, dw[:, keep])
        np.testing.assert_array_equal(dX2, dX[:, keep])


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
@pytest.mark.parametrize("cls", FP32)
def test_fixed_and_absent_controls(cls, name):
    """sigma_x = +inf on a seeded third of the controls, all of one stage's among them (both
    models): the step is exactly 0 there before and after each refinement, and meets the case's
    bounds on the reduced system (rows and columns of the fixed variables removed from M).
    uav5 (three of the six controls absent): their steps are exactly 0 as well (_step), with
    every real control of a stage fixed besides."""
    spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
    ref, bd = fr.bounds(name, "mild", kr.COMBOS[1])
    B = er.CASES[name]
    fx = fr.draw_fixed(spec, B)
    sx = np.where(fx, np.inf, inp["sigma_x"])
    dw, dX, info = _step(cls, spec, inp, sigma_x=sx)
    assert np.all(info == 0), info
    for b in range(B):
        free = ~fx[b]
        for t in range(3):
            assert np.all(dw[t, b][:, fx[b]] == 0.0), (cls, name, b, t)
            _check_dX(evs[b], dw[t, b], dX[t, b], f"{cls} {name} fixed scenario {b} step {t}")
        r = fr.rhos([dw[0, b], dw[1, b], dw[2, b]], per[b], free)
        print(f"{cls} {name} fixed scenario {b}: {int(fx[b].sum())} of {spec.nw} fixed, rho {np.max(r[0]):.2e} / "
              f"{np.max(r[1]):.2e} / {np.max(r[2]):.2e} (bounds {bd[0]:.2e} {bd[1]:.2e} {bd[2]:.2e})")
        for t in range(3):
            assert np.all(r[t] <= bd[t]), (cls, name, b, t, r[t], bd[t])
        assert np.all(r[1] < r[0]), (cls, name, b, r[0], r[1])
