"""The fused reverse-mode sensitivity entry points without a GPU: exported, argument checks
before any device call, part of the evaluation kernel's translation unit with their source under
the build hash -- and the checker of tests/test_gpu_solve_adjoint.py (tests/solve_adjoint_ref.py)
shown to satisfy the adjoint identity against the forward dense sensitivity of tests/kkt_ref.py
and its gate shown to have teeth, all on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import solve_adjoint_ref as sr
from tests import kkt_ref as kr
from tests import trace_cases as tc

NAMES = ("nmpc_solve_adjoint_batch", "nmpc_solve_adjoint_batch_dev")


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_solve_adjoint_batch(" in text and "int nmpc_solve_adjoint_batch_dev(" in text


def test_null_handle_is_invalid_for_both_entry_points():
    """NMPC_E_INVALID before anything is read or written.  The other invalid-argument cases need
    a live handle, which needs a device: tests/test_gpu_solve_adjoint.py::
    test_argument_validation_on_a_live_handle runs every one of them on both entry points."""
    L = _lib.lib()
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_solve_adjoint_batch(None, 1, 1, *([q, 0] * 12), q, q, q, C.cast(buf, ip), q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_solve_adjoint_batch_dev(None, 1, 1, *([a, 0] * 12), a, a, a, a, a, vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    # ... whatever else is wrong with the call
    rc = L.nmpc_solve_adjoint_batch(None, 0, 0, *([None, 0] * 12), None, None, None, None, None)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_fused_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_adjoint.hip and after nmpc_point.hip, the steps it shares with the tangent and policy
    kernels, and the library's build id covers both files."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_solve_adjoint.hip"' in text and '#include "nmpc_point.hip"' in text
    assert (text.index('#include "nmpc_adjoint.hip"') < text.index('#include "nmpc_point.hip"')
            < text.index('#include "nmpc_solve_adjoint.hip"'))
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_solve_adjoint.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    moved = ge.source_hash()
    assert moved != before
    with open(copy / "nmpc_point.hip", "ab") as fh:
        fh.write(b"x")
    assert ge.source_hash() not in (before, moved)


STEP = 1e-3
EPS = 2.2e-16


@pytest.mark.parametrize("name", list(sr.SOLVED))
def test_the_checker_satisfies_the_adjoint_identity(name):
    """On oracle solutions (every scenario converges: asserted), for dp = I[:, :8] and all three
    seeds: D = <x_bar, dx> + <lam_g_bar, dlam_g> + <X_bar, Z dx + Xp dp> - <pbar, dp> with
    (dx, dlam_g) of kkt_ref.dense_sensitivity at the checker's delta, whose two parameter
    derivatives are central differences of step h.  With M symmetric, M q = r and M dx = -dgl_h - J' Sigma_s dg_h the left
    side is -<q, dgl_h> + <Sigma_s (lam_g_bar - J q), dg_h> + <X_bar, Xp dp>: pbar' dp with C dp and
    Jp dp replaced by their differences.  So D is the differences' own error seen through q and y:
      truncation  c h^2 + O(h^4); the same sum at h / 2 differs from it by 3/4 c h^2, so the bound
                  takes 2 |LHS(h) - LHS(h/2)| (4/3 of it is the h^2 term, the rest is left to h^4);
      rounding    each difference quotient carries at most 4 eps |terms| / h (two evaluations, h and
                  h/2): |q|' (|grad f| + |J|' |lam_g|) and |y|' |g|; and the perturbed argument
                  p +- h dp is itself rounded by eps |p| (positions are hundreds of metres), as
                  are the differences against it inside the model, so the step actually taken is
                  off by up to eps |p| / h of itself: 4 eps (1 + |p|' |dp|) / h of
                  |q|' |C dp| + |y|' |Jp dp|;
      the solves  <r, dx> - <q, t> = <q, e_x> - <e_q, dx> with the residuals e_q = M q - r and
                  e_x = M dx - t of the two dense solves (tests/test_gpu_adjoint.py derives it), which
                  are formed here: |q|' |e_x| + |dx|' |e_q|;
      the sums    (nw + ng + nX) eps x the sum of the absolute terms, for the inner products.
    The bound must itself stay below 1e-2 of the sum of the absolute terms (a wrong sign or a
    dropped term moves the sum by the order of its terms), or it would show nothing."""
    spec, prob, P, bounds, sols = sr.solved(name)
    B = len(sols)
    assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
    seeds = sr.draw_seeds(spec, B, sr.NA, 91)
    nd = 8
    dp = np.eye(spec.np)[:nd]
    worst = loose = 0.0
    for b, s in enumerate(sols):
        adj = sr.adjoint_of(name, b, seeds)
        dn, ev, ss, free = adj["dn"], adj["ev"], adj["ss"], adj["free"]
        fw = [kr.dense_sensitivity(prob, s["x"], s["lam_g"], s["lam_x"], P[b], dp, *bounds, h, adj["delta"])
              for h in (STEP, STEP / 2)]
        for a in range(sr.NA):
            xb, lb, Xb = (seeds[k][b][a] for k in ("x_bar", "lam_g_bar", "X_bar"))
            q, jq = adj["q"][a], adj["jq"][a]
            y = ss * (lb - jq)
            e_q = adj["M"] @ q[free] - adj["rhs"][a]
            for j in range(nd):
                lhs = [xb @ f["dx"][j] + lb @ f["dlam_g"][j] + Xb @ (dn["Z"] @ f["dx"][j] + dn["Xp"] @ dp[j]) for f in fw]
                rhs = adj["pbar"][a] @ dp[j]
                dx = fw[0]["dx"][j]
                e_x = adj["M"] @ dx[free] - fw[0]["rhs"][j]
                bound = 2.0 * abs(lhs[0] - lhs[1])
                bound += 4.0 * EPS / STEP * (np.abs(q) @ (np.abs(ev.gradF) + np.abs(ev.J).T @ np.abs(s["lam_g"]))
                                             + np.abs(y) @ np.abs(ev.g))
                bound += (4.0 * EPS / STEP * (1.0 + np.abs(P[b]) @ np.abs(dp[j]))
                          * (np.abs(q) @ np.abs(dn["C"] @ dp[j]) + np.abs(y) @ np.abs(dn["Jp"] @ dp[j])))
                bound += np.abs(q[free]) @ np.abs(e_x) + np.abs(dx[free]) @ np.abs(e_q)
                terms = (np.abs(xb) @ np.abs(dx) + np.abs(lb) @ np.abs(fw[0]["dlam_g"][j])
                         + np.abs(Xb) @ np.abs(dn["Z"] @ dx + dn["Xp"] @ dp[j]) + np.abs(adj["pbar"][a]) @ np.abs(dp[j]))
                bound += (spec.nw + spec.ng + spec.nX) * EPS * terms
                D = lhs[0] - rhs
                if terms == 0.0:  # an entry of p that nothing reads: every term is exactly 0
                    assert D == 0.0 and lhs[1] == 0.0, (name, b, a, j, D)
                    continue
                worst, loose = max(worst, abs(D) / bound), max(loose, bound / terms)
                assert abs(D) <= bound, (name, b, a, j, D, bound)
    print(f"{name}: adjoint identity defect / bound {worst:.2e}, bound / sum of absolute terms at most {loose:.2e}")
    assert loose <= 1e-2, (name, loose)


# (mutant, case): the pairs on which the mutant misses the gate by MARGIN on every scenario.  Left
# out: the floor mutant on `race_track_2` (7.7e3 on scenario 0, exactly 0 on scenarios 1 to 3,
# which have no active row), on `weights_in_p` (2.8e3 on scenario 0, exactly 0 on the other two)
# and on `uav5` (exactly 0 on all three: its one active row keeps a slack of 1e-3, far above the
# floor): the mutant is the formula there (tests/solve_adjoint_ref.py).  `dynamic` is solved for
# this mutant's sake.
LEFT_OUT = {("nofloor", "race_track_2"), ("nofloor", "uav5"), ("nofloor", "weights_in_p")}
TEETH = [(m, n) for m in sr.MUTANTS for n in sr.SOLVED if (m, n) not in LEFT_OUT]
# smallest figures (race_track_2, uav5, dynamic, weights_in_p): nolam 1.2e2, 1.4e2, 1.3e16, 2.1e2;
# noX 5.7e8, 4.2e9, 8.0e9, 9.8e8; zplus 1.6e9, 1.8e10, 1.4e10, 1.6e10; nofloor 1.9e1 (dynamic)


@pytest.mark.parametrize("which,name", TEETH)
def test_the_gate_has_teeth_for_a_wrong_term(which, name):
    """A checker with one term wrong (tests/solve_adjoint_ref.py: MUTANTS) misses the pbar gate of
    tests/adjoint_ref.py -- 1e-10 of the sum of the absolute terms -- by at least
    trace_cases.MARGIN on every scenario of the case; the right checker passes against itself."""
    spec, prob, P, bounds, sols = sr.solved(name)
    seeds = sr.draw_seeds(spec, len(sols), sr.NA, 91)
    for b in range(len(sols)):
        good = sr.adjoint_of(name, b, seeds)
        assert sr.pbar_figure(good["pbar"], good) == 0.0
        mut = sr.adjoint_of(name, b, seeds, mutant=which, delta=good["delta"])
        fig = sr.pbar_figure(mut["pbar"], good)
        print(f"{name} scenario {b}, mutant {which}: pbar error / bound {fig:.2e}")
        assert fig >= tc.MARGIN, (which, name, b, fig)
