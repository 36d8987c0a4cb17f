"""The KKT-solve entry points without a GPU: exported, argument checks before any device call,
part of the evaluation kernel's translation unit with their source under the build hash -- and
the basis of the gate of tests/test_gpu_kkt.py re-measured on the CPU: the numpy restatement of
the stage-wise recursion against the dense matrix, and the gate's teeth on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import eval_ref as er
from tests import kkt_ref as kr

NAMES = ("nmpc_kkt_solve_batch", "nmpc_kkt_solve_batch_dev")


def test_both_symbols_are_declared_and_exported():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_kkt_solve_batch(" in text and "int nmpc_kkt_solve_batch_dev(" in text


def _call(L, dev, h, B, nr, x, p, rw, rg, dw, dX, jdw, lds=(0,) * 8):
    """Both entry points with the same argument list; lds = leading dimensions of x, p, lam_g,
    sigma_x, sigma_s, delta, r_w, r_g."""
    z = C.c_void_p(0) if dev else None
    args = [h, B, nr, x, lds[0], p, lds[1], z, lds[2], 1.0, z, lds[3], z, lds[4], z, lds[5], rw, lds[6], rg, lds[7],
            dw, dX, jdw, z]
    if dev:
        return L.nmpc_kkt_solve_batch_dev(*args, C.c_void_p(0))
    return L.nmpc_kkt_solve_batch(*args)


@pytest.mark.parametrize("dev", [False, True])
def test_null_handle_is_invalid(dev):
    L = _lib.lib()
    buf = (C.c_double * 8)()
    q = C.c_void_p(C.addressof(buf)) if dev else C.cast(buf, C.POINTER(C.c_double))
    rc = _call(L, dev, None, 1, 1, q, q, q, q, q, q, q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_kkt_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the KKT kernel's file is included by nmpc_eval.hip after
    the products kernel's, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_kkt.hip"' in text
    assert text.index('#include "nmpc_products.hip"') < text.index('#include "nmpc_kkt.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_kkt.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


def test_kkt_solve_raises_without_a_gpu():
    """No CPU path: without a device the handle cannot be created, so the entry point is
    unreachable -- as for every other entry point."""
    import torch

    from nmpc_amd import REFERENCE_OPTS, make_spec, nlpsol
    from nmpc_amd.nlpsol import Solver

    assert callable(Solver.kkt_solve) and callable(Solver.kkt_solve_device) and callable(Solver.sensitivity)
    if torch.cuda.is_available():
        return  # with a GPU the entry points run: tests/test_gpu_kkt.py
    spec = make_spec("race_track_2", N=6, T=0.2)
    with pytest.raises(_lib.NmpcError):
        s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
        s.kkt_solve(np.zeros(spec.nw), np.zeros(spec.np), r_w=np.ones(spec.nw))


def test_stage_terms_are_the_oracles_hessian():
    """The checker's stage-wise Hxx_k, Hxu_k assemble to SSEval.hessian exactly (same
    expressions): the restatement has no second definition of the derivatives."""
    for name in ("race_track_2", "uav5", "n1"):
        spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
        for b, ev in enumerate(evs):
            Hxx, Hxu = kr.stage_terms(ev, inp["obj_factor"], inp["lam_g"][b])
            nu, N = ev.prob.nu, ev.prob.N
            W = np.zeros_like(per[b]["W"])
            for k in range(1, N + 1):
                W += ev.Z[k].T @ Hxx[k] @ ev.Z[k]
                if k < N:
                    Cx = ev.Z[k].T @ Hxu[k]
                    W[:, nu * k:nu * k + nu] += Cx
                    W[nu * k:nu * k + nu, :] += Cx.T
            assert np.array_equal(W, per[b]["W"]), (name, b)


@pytest.mark.parametrize("regime", kr.REGIMES)
@pytest.mark.parametrize("name", list(er.CASES))
def test_the_bounds_basis_restatement_against_the_dense_matrix(name, regime):
    """The figures the bound rests on, re-measured here: the numpy fp64 restatement of the
    recursion and numpy's dense solve both meet rho <= nw * 2.2e-16 against the dense M on
    every scenario (the classical bound c n u of a backward-stable solve with c = 1; at most
    8.4e-14, three orders below the gate), the restatement's inertia verdict is 'positive
    definite' with the checker's delta, and it passes the gate itself, the mild regime's
    forward gate included."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, regime, combo)
        for b, ev in enumerate(evs):
            dw, ok = kr.riccati_np(ev, inp["obj_factor"], inp["lam_g"][b], inp["sigma_x"][b], inp["sigma_s"][b],
                                   inp["delta"][b], inp["r_w"][b], inp["r_g"][b])
            assert ok, (name, regime, combo, b)
            r, f = kr.figures(dw, per[b], regime)
            rd, _ = kr.figures(per[b]["ref"], per[b], regime)
            print(f"{name} {regime} obj {combo[0]} scenario {b}: delta {inp['delta'][b]:.3g}, cond {per[b]['cond']:.1e}, "
                  f"rho recursion {r:.2e}, rho dense solve {rd:.2e}, forward {f:.2e}")
            stable = spec.nw * np.finfo(float).eps
            assert r <= stable and rd <= stable, (name, regime, b, r, rd)
            kr.check_solution(dw, per[b], regime, f"{name} {regime} {b}")


def test_the_restatement_handles_fixed_variables_and_judges_inertia():
    spec, inp, per, evs = kr.reference("race_track_2", "mild", kr.COMBOS[0])
    rng = np.random.default_rng(5)
    for b, ev in enumerate(evs):
        fx = rng.uniform(size=spec.nw) < 0.2
        dw, ok = kr.riccati_np(ev, 1.0, inp["lam_g"][b], inp["sigma_x"][b], inp["sigma_s"][b], inp["delta"][b],
                               inp["r_w"][b], inp["r_g"][b], fixed=fx)
        assert ok and np.all(dw[:, fx] == 0.0)
        fr = ~fx
        M, rhs = per[b]["M"][np.ix_(fr, fr)], per[b]["rhs"][:, fr]
        assert max(kr.rho(M, dw[c, fr], rhs[c]) for c in range(kr.NR)) <= spec.nw * np.finfo(float).eps
    spec, inp, ratio = kr.indefinite_cases("race_track_2")
    _, _, evs = kr.pr.evals("race_track_2")
    z = np.zeros
    for b, ev in enumerate(evs):
        if ratio[b] < -kr.INDEF:
            _, ok = kr.riccati_np(ev, 1.0, inp["lam_g"][b], z(spec.nw), z(spec.ng), 0.0, z((1, spec.nw)) + 1.0,
                                  z((1, spec.ng)))
            assert not ok, b


@pytest.mark.parametrize("name", ["race_track_2", "nmpc_tt", "dynamic"])
def test_the_inertia_cases_have_indefinite_scenarios(name):
    """sigma = 0, delta = 0: the checker finds at least one scenario judged indefinite."""
    _, _, ratio = kr.indefinite_cases(name)
    print(f"{name}: lambda_min / max|M| = " + ", ".join(f"{v:.2e}" for v in ratio))
    assert np.any(ratio < -kr.INDEF)


# the cases each mutant is shown on: ones where the dropped term exists and is more than 1e-10
# of |M| -- a normwise residual sees an error E of M as |E dw| / (|M| |dw|), so a term far
# below the gate relative to M cannot be seen by it, whatever the solve (n63_16obs: below)
@pytest.mark.parametrize("which,name", [("dyn_hess", "race_track_2"), ("dyn_hess", "uav5"), ("Hg", "dynamic"),
                                        ("Hg", "n1"), ("Hxu", "nmpc_tt"), ("Hxu", "uav5")])
def test_the_gate_has_teeth_for_a_dropped_term(which, name):
    """A dense step computed with a Hessian that lacks one term -- the dynamics' second
    derivatives, the obstacle curvature, or the state-control cross term -- misses the rho gate
    against the true M on every scenario of the case (weights <= 1: a large barrier weight
    would hide the Hessian behind Sigma)."""
    spec, inp, per, evs = kr.reference(name, "teeth", kr.COMBOS[0])
    for b, ev in enumerate(evs):
        Wm = kr.mutant_W(ev, 1.0, inp["lam_g"][b], which)
        Mm = kr.dense_M(ev, Wm, inp["sigma_x"][b], inp["sigma_s"][b], inp["delta"][b])
        dw = np.linalg.solve(Mm, per[b]["rhs"].T).T
        r, _ = kr.figures(dw, per[b], "teeth")
        print(f"{name} scenario {b}, mutant {which}: rho {r:.2e} (bound {kr.TOL:.0e})")
        assert r > kr.TOL, (which, name, b, r)
        with pytest.raises(AssertionError):
            kr.check_solution(dw, per[b], "teeth", f"{name} mutant {which}")


def test_what_the_gate_cannot_see():
    """Recorded, not gated: on n63_16obs the obstacle curvature (|lam_g| ~ 10
    over distances of hundreds of metres) is 5e-9 to 3e-6 of max|M| (stage-cost Hessians seen
    through 63 stages of sensitivities, and the delta that makes M positive definite), so
    dropping it moves the normwise residual by 4e-12 to 2e-9: 0.04x, 0.5x and 22x the gate on
    the three scenarios (measured here), i.e. not on every scenario.  The products gate of
    tests/products_ref.py, whose scale is per direction, is the one that sees it (by 1e7)."""
    name = "n63_16obs"
    spec, inp, per, evs = kr.reference(name, "teeth", kr.COMBOS[0])
    for b, ev in enumerate(evs):
        Wm = kr.mutant_W(ev, 1.0, inp["lam_g"][b], "Hg")
        size = float(np.max(np.abs(Wm - per[b]["W"]))) / float(np.max(np.abs(per[b]["M"])))
        Mm = kr.dense_M(ev, Wm, inp["sigma_x"][b], inp["sigma_s"][b], inp["delta"][b])
        r, _ = kr.figures(np.linalg.solve(Mm, per[b]["rhs"].T).T, per[b], "teeth")
        print(f"{name} scenario {b}, mutant Hg: max|dW| / max|M| {size:.2e}, rho {r:.2e} = {r / kr.TOL:.2e} x bound")
        assert np.isfinite(r) and size > 0.0


@pytest.mark.parametrize("name", ["race_track_2", "nmpc_tt", "n63_16obs", "dynamic", "weights_in_p", "uav5"])
def test_what_one_entry_off_by_1e_7_does(name):
    """One stage-cost Hessian entry of one stage off by 1e-7 relative, seen through the step:
    the figure is printed and recorded in DESIGN.md 14; asserted is only that the mutant moves
    the residual at all (rho above the unmutated dense solve's)."""
    spec, inp, per, evs = kr.reference(name, "teeth", kr.COMBOS[0])
    for b, ev in enumerate(evs):
        Wm = kr.mutant_W(ev, 1.0, inp["lam_g"][b], "Hl")
        Mm = kr.dense_M(ev, Wm, inp["sigma_x"][b], inp["sigma_s"][b], inp["delta"][b])
        r, _ = kr.figures(np.linalg.solve(Mm, per[b]["rhs"].T).T, per[b], "teeth")
        r0, _ = kr.figures(per[b]["ref"], per[b], "teeth")
        print(f"{name} scenario {b}, Hl entry x (1 + 1e-7): rho {r:.2e} = {r / kr.TOL:.2e} x bound "
              f"(unmutated {r0:.2e})")
        assert r > r0
