"""The fused forward-mode sensitivity entry points without a GPU: exported, argument checks
before any device call, part of the evaluation kernel's translation unit with their source under
the build hash -- and the checker of tests/test_gpu_solve_tangent.py (tests/solve_tangent_ref.py)
shown to satisfy the adjoint identity against the dense reverse-mode checker of
tests/solve_adjoint_ref.py, to agree with the difference-quotient sensitivity of tests/kkt_ref.py
within that reference's own error, and its gate shown to have teeth, all on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import kkt_ref as kr
from tests import solve_adjoint_ref as sr
from tests import solve_tangent_ref as tr
from tests import trace_cases as tc

NAMES = ("nmpc_solve_tangent_batch", "nmpc_solve_tangent_batch_dev")


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_solve_tangent_batch(" in text and "int nmpc_solve_tangent_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written.  A NULL handle is refused first,
    whatever else is wrong with the call: B <= 0, nd <= 0, every output NULL, a bad leading
    dimension.  Those need a live handle, which needs a device, to be reached on their own:
    tests/test_gpu_solve_tangent.py::test_argument_validation_on_a_live_handle runs every one of
    them on both entry points."""
    L = _lib.lib()
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_solve_tangent_batch(None, 1, 1, *([q, 0] * 10), q, q, q, C.cast(buf, ip), q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_solve_tangent_batch_dev(None, 1, 1, *([a, 0] * 10), a, a, a, a, a, vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    for B, nd, ins, outs in ((0, 1, [q, 0] * 10, (q, q, q)), (-2, 1, [q, 0] * 10, (q, q, q)),
                             (1, 0, [q, 0] * 10, (q, q, q)), (1, -1, [q, 0] * 10, (q, q, q)),
                             (1, 1, [q, 0] * 10, (None, None, None)), (1, 1, [q, -1] * 10, (q, q, q)),
                             (0, 0, [None, 0] * 10, (None, None, None))):
        rc = L.nmpc_solve_tangent_batch(None, B, nd, *ins, *outs, C.cast(buf, ip), q)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, nd)
    assert list(buf) == [0.0] * 8


def test_fused_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_solve_adjoint.hip (both on nmpc_point.hip's LDS carve-up and weights), and the library's
    build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_solve_tangent.hip"' in text
    assert text.index('#include "nmpc_solve_adjoint.hip"') < text.index('#include "nmpc_solve_tangent.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_solve_tangent.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


STEP = 1e-3
EPS = 2.2e-16


@pytest.mark.parametrize("name", list(tr.SOLVED))
def test_the_checker_satisfies_the_adjoint_identity(name):
    """On oracle solutions (every scenario converges: asserted), N(0, 1) directions (nd = 2) and
    N(0, 1) seeds on x*, lam_g* and X* (na = 2), at the same delta:
    D = <x_bar, dx> + <lam_g_bar, dlam_g> + <X_bar, dX> - <pbar, dp> with pbar of
    solve_adjoint_ref.dense_adjoint.  With M symmetric, M q = r and M dx = t the difference is
      the solves  <r, dx> - <q, t> = <q, e_x> - <e_q, dx> with the residuals e_q = M q - r and
                  e_x = M dx - t of the two dense solves, which are formed here:
                  |q|' |e_x| + |dx|' |e_q|;
      the terms   every inner product and matrix product on either side is a sum of at most
                  nw + ng + nX + np terms, nested three deep (seed, weight, matrix):
                  3 (nw + ng + nX + np) eps x the sum of the absolute terms of both sides,
                  |x_bar|' |dx| + |lam_g_bar|' Sigma_s (|J| |dx| + |Jp| |dp|) + |X_bar|' (|Z| |dx| + |Xp| |dp|)
                  + |q|' |C| |dp| + (Sigma_s (|lam_g_bar| + |J| |q|))' |Jp| |dp| + |X_bar|' |Xp| |dp|.
    The bound must itself stay below 1e-2 of the sum of the absolute terms (a wrong sign or a
    dropped term moves the sum by the order of its terms), or it would show nothing."""
    spec, prob, P, bounds, sols = sr.solved(name)
    B = len(sols)
    assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
    seeds = sr.draw_seeds(spec, B, sr.NA, 91)
    dp = tr.draw_directions(spec, B, tr.ND, 93)
    worst = loose = 0.0
    for b in range(B):
        fw = tr.tangent_of(name, b, dp)
        adj = sr.adjoint_of(name, b, seeds, delta=fw["delta"])
        dn, ss, free = fw["dn"], fw["ss"], fw["free"]
        aJ, aZ, aC, aJp, aXp = (np.abs(dn[k]) for k in ("J", "Z", "C", "Jp", "Xp"))
        for a in range(sr.NA):
            xb, lb, Xb = (seeds[k][b][a] for k in ("x_bar", "lam_g_bar", "X_bar"))
            q = adj["q"][a]
            e_q = adj["M"] @ q[free] - adj["rhs"][a]
            for j in range(tr.ND):
                dx, d = fw["dx"][j], dp[b][j]
                e_x = fw["M"] @ dx[free] - fw["rhs"][j]
                lhs = xb @ dx + lb @ fw["dlam_g"][j] + Xb @ fw["dX"][j]
                rhs = adj["pbar"][a] @ d
                terms = (np.abs(xb) @ np.abs(dx) + np.abs(lb) @ fw["scale"]["dlam_g"][j] + np.abs(Xb) @ fw["scale"]["dX"][j]
                         + np.abs(q) @ (aC @ np.abs(d)) + (ss * (np.abs(lb) + aJ @ np.abs(q))) @ (aJp @ np.abs(d))
                         + np.abs(Xb) @ (aXp @ np.abs(d)))
                bound = np.abs(q[free]) @ np.abs(e_x) + np.abs(dx[free]) @ np.abs(e_q)
                bound += 3 * (spec.nw + spec.ng + spec.nX + spec.np) * EPS * terms
                D = lhs - rhs
                worst, loose = max(worst, abs(D) / bound), max(loose, bound / terms)
                assert abs(D) <= bound, (name, b, a, j, D, bound)
    print(f"{name}: adjoint identity defect / bound {worst:.2e}, bound / sum of absolute terms at most {loose:.2e}")
    assert loose <= 1e-2, (name, loose)


@pytest.mark.parametrize("name", list(tr.SOLVED))
def test_the_checker_matches_the_difference_quotient_sensitivity(name):
    """kkt_ref.dense_sensitivity at the checker's delta: the same M and weights, the two parameter
    derivatives as central differences of step h = 1e-3.  Its own error, per entry of dx:
      truncation  c h^2 + O(h^4) in the right-hand side and so in dx; the same at h / 2 differs by
                  3/4 c h^2, so the bound takes 2 |dx(h) - dx(h/2)|;
      rounding    each difference quotient carries at most 4 eps |terms| / h: |grad f| + |J|' |lam_g|
                  for grad_l and |g| for g, the latter through J' Sigma_s; the perturbed argument
                  p +- h dp is itself rounded by eps |p|, so the step actually taken is off by up
                  to 4 eps (1 + |p|' |dp|) / h of itself, of |C| |dp| + |J|' Sigma_s |Jp| |dp|; all of
                  it through |M^-1|;
      the solves  |M^-1| (|e_fd| + |e_x|) with the residuals of the two dense solves.
    dlam_g = Sigma_s (J dx + dg): 2 |dlam_g(h) - dlam_g(h/2)| + Sigma_s (|J| x dx's rounding and
    solve terms + 4 eps / h (|g| + (1 + |p|' |dp|) |Jp| |dp|)).  At these solutions M is singular
    at delta = 0 (the last heading-rate control moves nothing that is read), delta = 1e-4 and
    |M^-1| reaches 1e4 along that control, so this reference's truncation is amplified there:
    on race_track_2 scenario 3 its own error reaches 0.43 on a dx of 9.5 (bound 0.65), where the
    adjoint identity above is sharp to 1e-12.  dx's bound must stay below the largest
    entry of the direction's dx, or it would show nothing; the largest ratios are printed."""
    spec, prob, P, bounds, sols = sr.solved(name)
    B = len(sols)
    assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
    dp = tr.draw_directions(spec, B, tr.ND, 93)
    worst = {"dx": 0.0, "dlam_g": 0.0}
    loose = {"dx": 0.0, "dlam_g": 0.0}
    for b, s in enumerate(sols):
        fw = tr.tangent_of(name, b, dp)
        dn, ev, ss, free = fw["dn"], fw["ev"], fw["ss"], fw["free"]
        fd = [kr.dense_sensitivity(prob, s["x"], s["lam_g"], s["lam_x"], P[b], dp[b], *bounds, h, fw["delta"])
              for h in (STEP, STEP / 2)]
        aMi = np.abs(np.linalg.inv(fw["M"]))
        aJ = np.abs(dn["J"])
        for j in range(tr.ND):
            d = dp[b][j]
            step_err = 4.0 * EPS / STEP * (1.0 + np.abs(P[b]) @ np.abs(d))
            ajp = np.abs(dn["Jp"]) @ np.abs(d)
            e_rhs = 4.0 * EPS / STEP * (np.abs(ev.gradF) + aJ.T @ np.abs(s["lam_g"]) + aJ.T @ (ss * np.abs(ev.g)))
            e_rhs += step_err * (np.abs(dn["C"]) @ np.abs(d) + aJ.T @ (ss * ajp))
            e_fd = fd[0]["M"] @ fd[0]["dx"][j][free] - fd[0]["rhs"][j]
            e_x = fw["M"] @ fw["dx"][j][free] - fw["rhs"][j]
            rnd = np.zeros(spec.nw)
            rnd[free] = aMi @ (e_rhs[free] + np.abs(e_fd) + np.abs(e_x))
            bound = {"dx": 2.0 * np.abs(fd[0]["dx"][j] - fd[1]["dx"][j]) + rnd,
                     "dlam_g": 2.0 * np.abs(fd[0]["dlam_g"][j] - fd[1]["dlam_g"][j])
                     + ss * (aJ @ rnd + 4.0 * EPS / STEP * np.abs(ev.g) + step_err * ajp)}
            for k in ("dx", "dlam_g"):
                err = np.abs(fw[k][j] - fd[0][k][j])
                big = float(np.max(np.abs(fw[k][j])))
                m = bound[k] > 0
                assert np.all(err[~m] == 0.0), (name, b, j, k)
                worst[k] = max(worst[k], float(np.max(err[m] / bound[k][m], initial=0.0)))
                loose[k] = max(loose[k], float(np.max(bound[k])) / big)
                assert np.all(err <= bound[k]), (name, b, j, k, float(np.max(err[m] / bound[k][m])))
    print(f"{name}: against the difference-quotient sensitivity, error / bound dx {worst['dx']:.2e}, dlam_g "
          f"{worst['dlam_g']:.2e}; bound / largest entry dx {loose['dx']:.2e}, dlam_g {loose['dlam_g']:.2e}")
    # (dlam_g's bound carries Sigma_s x the quotients' rounding: on `dynamic`, whose active rows have
    # Sigma_s up to 1e8, it exceeds the entries themselves and shows nothing there; it is printed)
    assert loose["dx"] <= 1.0, (name, loose)


# (mutant, case): the pairs on which the mutant misses the gate by MARGIN on every scenario.  Left
# out: the floor mutant on `race_track_2` (2.4e9 on scenario 0, exactly 0 on scenarios 1 to 3,
# which have no active row below the floor), on `weights_in_p` (exactly 0 on scenario 1) and on
# `uav5` (exactly 0 on all three): the mutant is the formula there (tests/solve_tangent_ref.py).
# `dynamic` (2 to 7 such rows in every scenario) remains for it.
LEFT_OUT = {("nofloor", "race_track_2"), ("nofloor", "uav5"), ("nofloor", "weights_in_p")}
TEETH = [(m, n) for m in tr.MUTANTS for n in tr.SOLVED if (m, n) not in LEFT_OUT]
# smallest figures over the scenarios of every remaining case: norhsjp 1.0e10, nojp 1.0e10, noXp 1.0e10,
# hpsign 2.0e10, nofloor 3.6e9 (dynamic)


@pytest.mark.parametrize("which,name", TEETH)
def test_the_gate_has_teeth_for_a_wrong_term(which, name):
    """A checker with one term wrong (tests/solve_tangent_ref.py: MUTANTS) misses gate (b) -- dlam_g
    and dX within 1e-10 of the per-entry sum of the absolute terms -- by at least
    trace_cases.MARGIN on every scenario of the case; the right checker passes against itself.
    Directions: the two N(0, 1) ones of the tests above and dp = I, as tests/test_gpu_solve_tangent.py
    uses them.  (A N(0, 1) direction moves every entry of p at once and its large terms set the
    scale; on those two alone the floor mutant reaches only 8.4 on `dynamic` scenario 2, with
    dp = I 1.6e9.)"""
    spec, prob, P, bounds, sols = sr.solved(name)
    B = len(sols)
    dp = np.concatenate([tr.draw_directions(spec, B, tr.ND, 93), np.repeat(np.eye(spec.np)[None], B, axis=0)], axis=1)
    for b in range(len(sols)):
        good = tr.tangent_of(name, b, dp)
        assert max(tr.figures(good, good).values()) == 0.0
        mut = tr.tangent_of(name, b, dp, mutant=which, delta=good["delta"])
        fig = max(tr.figures(mut, good).values())
        print(f"{name} scenario {b}, mutant {which}: error / bound {fig:.2e}")
        assert fig >= tc.MARGIN, (which, name, b, fig)
