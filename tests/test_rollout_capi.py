"""The policy-rollout entry points without a GPU: exported, declared, a NULL handle refused before
any device call, the kernel part of the evaluation unit with its source under the build hash -- and
the checker of tests/test_gpu_policy_rollout.py (tests/rollout_ref.py) shown to pass its own gates on
the oracle alone, with every mutant missing the gate named for it on every scenario:

  identity       e0 = 0, w = 0, K = the dense-oracle policy of tests/policy_ref.py: X is the oracle's
                 X* and J its objective, bitwise (the same operations in the same order), nsat = 0;
  linearisation  e0 = eps d, no clamp: r(eps) = |x_1 - X*_1 - (A_0 + B_0 K_0) eps d|_inf is second
                 order, r(eps) / r(eps / 2) = 4 within a factor of 2.  A first-order error gives a
                 ratio of 2 (1 + O(eps)), on the gate's edge, so the residual is also held to
                 r(eps) <= sqrt(eps) |(A_0 + B_0 K_0) eps d|_inf: relative to the linear term a
                 second-order residual scales as eps and a first-order one as eps^0, and sqrt(eps) is
                 their geometric mean.  Where every control of stage 0 is active K_0 is ~1e-7 and
                 x_1 cannot tell a wrong K_0 from a right one, so the same two bounds are also asked
                 of the whole trajectory against dX_{k+1} = (A_k + B_k K_k) dX_k, dX_0 = eps d;
  clamp          with disturbances that saturate, every applied control lies in the clamp box and
                 nsat counts exactly the entries on its faces (the mutant `noclamp` misses this one:
                 with e0 = 0 no clamp engages, so neither gate above can see it).

The measured figures are printed wherever the suite runs."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import policy_ref as pf
from tests import rollout_ref as rr
from tests import solve_adjoint_ref as sr

NAMES = ("nmpc_policy_rollout_batch", "nmpc_policy_rollout_batch_dev")
EPS = 1e-4                       # linearisation: |e0| = EPS and EPS / 2
SIGMA = (0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02)  # clamp gate: e0 ~ N(0, diag SIGMA^2) x SCALE
SCALE = 20.0


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 28 + (name.endswith("_dev"))
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_policy_rollout_batch(" in text and "int nmpc_policy_rollout_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever
    else is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_policy_rollout.py::test_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    buf = (C.c_double * 8)()
    q, qi = C.cast(buf, dp), C.cast(buf, ip)
    for B, M, ins, outs in ((1, 1, [q, 0] * 10, (q, q, qi, q, q)), (0, 1, [q, 0] * 10, (q, q, qi, q, q)),
                            (1, 0, [q, 0] * 10, (q, q, qi, q, q)), (1, 1, [q, -1] * 10, (q, q, qi, q, q)),
                            (1, 1, [None, 0] * 10, (None,) * 5)):
        rc = L.nmpc_policy_rollout_batch(None, B, M, *ins, *outs)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, M)
    a = vp(C.addressof(buf))
    rc = L.nmpc_policy_rollout_batch_dev(None, 1, 1, *([a, 0] * 10), *([a] * 5), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_rollout_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_solve_policy.hip, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_policy_rollout.hip"' in text
    assert text.index('#include "nmpc_solve_policy.hip"') < text.index('#include "nmpc_policy_rollout.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_policy_rollout.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


def _cases():
    """(name, b, prob, p, bounds, oracle solution, dense-oracle policy) of the 13 solved scenarios."""
    for name in pf.SOLVED:
        spec, prob, P, bounds, sols = sr.solved(name)
        assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
        dp = pf.directions(spec, len(sols), 95)[:, :1]
        for b in range(len(sols)):
            yield name, b, prob, P[b], bounds, sols[b], pf.policy_of(name, b, dp)


def _shaped(prob, sol, bounds):
    N, nu, m = prob.N, prob.nu, prob.m
    lo, hi = rr.widen(bounds[0], bounds[1])
    return sol["x"].reshape(N, nu), lo.reshape(N, nu), hi.reshape(N, nu), bounds[2].reshape(N + 1, m), bounds[3].reshape(N + 1, m)


def _identity(prob, p, bounds, sol, pol, mutant=None):
    from oracle import nmpc_oracle as orc

    ubar, lo, hi, lg, ug = _shaped(prob, sol, bounds)
    r = rr.rollout_one(prob, p, ubar, pol["X"], pol["K"], np.zeros(prob.nx), np.zeros((prob.N, prob.nx)), lo, hi, lg, ug,
                       mutant=mutant)
    g = orc.constraints(prob, sol["x"], p)
    viol = max(0.0, float(np.max(g - bounds[3])), float(np.max(bounds[2] - g)))
    return (np.array_equal(r["X"], pol["X"]) and np.array_equal(r["U"], ubar) and r["J"] == orc.objective(prob, sol["x"], p)
            and r["nsat"] == 0 and r["viol"] == viol)


def _linearisation(prob, p, sol, pol, d, mutant=None):
    """[(r(EPS) / r(EPS / 2), r(EPS) / |linear term|_inf)] at x_1 and over the stages 1 ... N, the
    linear term being dX_{k+1} = (A_k + B_k K_k) dX_k from dX_0 = eps d."""
    N = prob.N
    ubar = sol["x"].reshape(N, prob.nu)
    res, lin = [], None
    for eps in (EPS, EPS / 2):
        r = rr.rollout_one(prob, p, ubar, pol["X"], pol["K"], eps * d, mutant=mutant)
        dX = np.zeros((N + 1, prob.nx))
        dX[0] = eps * d
        for k in range(N):
            dX[k + 1] = (pol["A"][k] + pol["B"][k] @ pol["K"][k]) @ dX[k]
        err = np.max(np.abs(r["X"] - pol["X"] - dX), axis=1)
        res.append((float(err[1]), float(np.max(err[1:]))))
        lin = lin or (float(np.max(np.abs(dX[1]))), float(np.max(np.abs(dX[1:]))))
    return [(res[0][j] / res[1][j], res[0][j] / lin[j]) for j in (0, 1)]


def _lin_ok(figs):
    return all(2.0 <= ratio <= 8.0 and rel <= np.sqrt(EPS) for ratio, rel in figs)


def _clamp(prob, p, bounds, sol, pol, e0, mutant=None):
    """(the clamp property holds, largest nsat) over the samples e0 (M, nx)."""
    ubar, lo, hi, lg, ug = _shaped(prob, sol, bounds)
    ok, most = True, 0
    for e in e0:
        r = rr.rollout_one(prob, p, ubar, pol["X"], pol["K"], e, None, lo, hi, lg, ug, mutant=mutant)
        inside = bool(np.all(r["U"] >= lo) and np.all(r["U"] <= hi))
        ok &= inside and r["nsat"] == int(np.sum((r["U"] == lo) | (r["U"] == hi)))
        most = max(most, r["nsat"])
    return ok, most


def _direction(prob, seed):
    d = np.random.default_rng(seed).standard_normal(prob.nx)
    return d / np.max(np.abs(d))


def test_the_checker_passes_its_own_gates():
    """Identity, linearisation and the clamp property on the 13 solved scenarios."""
    for i, (name, b, prob, p, bounds, sol, pol) in enumerate(_cases()):
        assert _identity(prob, p, bounds, sol, pol), (name, b)
        figs = _linearisation(prob, p, sol, pol, _direction(prob, 300 + i))
        e0 = rr.draw_disturbances(prob, 1, 4, SIGMA, 400 + i, big=(1, 2, 3), scale=SCALE)[0][0]
        ok, most = _clamp(prob, p, bounds, sol, pol, e0)
        print(f"{name} scenario {b}: identity bitwise; r(eps) / r(eps / 2) = {figs[0][0]:.3f} at x_1, {figs[1][0]:.3f} over "
              f"the stages (2 to 8), r(eps) / |linear term| = {figs[0][1]:.2e}, {figs[1][1]:.2e} (bound {np.sqrt(EPS):.0e}); "
              f"clamp property over 4 samples, largest nsat {most}")
        assert _lin_ok(figs), (name, b, figs)
        assert ok and most > 0, (name, b, most)


@pytest.mark.parametrize("which", rr.MUTANTS)
def test_every_mutant_misses_the_gate_named_for_it(which):
    """`transpose` and `shift` miss the linearisation gate, `noclamp` the clamp property, on every
    one of the 13 scenarios (at e0 = 0 every K multiplies a zero state difference and no clamp engages,
    so all three pass the identity: asserted too)."""
    for i, (name, b, prob, p, bounds, sol, pol) in enumerate(_cases()):
        assert _identity(prob, p, bounds, sol, pol, mutant=which), (which, name, b)
        if which == "noclamp":
            e0 = rr.draw_disturbances(prob, 1, 4, SIGMA, 400 + i, big=(1, 2, 3), scale=SCALE)[0][0]
            ok, most = _clamp(prob, p, bounds, sol, pol, e0, mutant=which)
            print(f"{name} scenario {b}, mutant {which}: clamp property {ok}, nsat {most}")
            assert not ok, (which, name, b)
        else:
            figs = _linearisation(prob, p, sol, pol, _direction(prob, 300 + i), mutant=which)
            print(f"{name} scenario {b}, mutant {which}: r(eps) / r(eps / 2) = {figs[0][0]:.3f} at x_1, {figs[1][0]:.3f} over the "
                  f"stages, r(eps) / |linear term| = {figs[0][1]:.2e}, {figs[1][1]:.2e} (bound {np.sqrt(EPS):.0e})")
            assert not _lin_ok(figs), (which, name, b, figs)
