"""The policy-covariance entry points without a GPU: exported, declared, a NULL handle refused before
any device call, the kernel part of the evaluation unit with its source under the build hash -- and
the checker of tests/test_gpu_policy_covariance.py (tests/covariance_ref.py) held against the
nonlinear plant on the oracle alone:

  sigma points   the columns of the Cholesky factors of S0 and, at each stage, of W are fed as +-eps
                 pairs through tests/rollout_ref.rollout_one, unclamped; with delta = (X+ - X-) / 2 eps
                 the sum of delta delta' over the pairs is Sigma_k up to O(eps^2), and the same sum of
                 the U differences is sigma_u^2.  Gate: within GATE = 1e-6 of max |Sigma_k| per stage
                 (of the largest sigma_u^2) at eps = 1e-3.
  mutants        `transpose`, `shift`, `noW` and `openloop` each miss that gate on every scenario.

Scenarios: the 13 solved ones with the dense-oracle policy of tests/policy_ref.py, and n1 and two of
n63_16obs's at tests/eval_ref.draw_point(seed=31).  nmpc_amd.policy.tighten is checked on CPU tensors.
The measured figures are printed wherever the suite runs."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import covariance_ref as cr
from tests import eval_ref as er
from tests import policy_ref as pf
from tests import rollout_ref as rr
from tests import solve_adjoint_ref as sr

NAMES = ("nmpc_policy_covariance_batch", "nmpc_policy_covariance_batch_dev")
SIGMA = (0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02)  # the rollout tests'
EPS = 1e-3
GATE = 1e-6
SYNTHETIC = (("n1", (0, 1)), ("n63_16obs", (0, 1)))


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 20 + (name.endswith("_dev"))
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_policy_covariance_batch(" in text and "int nmpc_policy_covariance_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever
    else is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_policy_covariance.py::test_gate_f_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    for B, nc, ins, outs in ((1, 1, [q, 0] * 7, (q, q, q)), (0, 1, [q, 0] * 7, (q, q, q)), (1, 0, [q, 0] * 7, (q, q, q)),
                             (1, 1, [q, -1] * 7, (q, q, q)), (1, 1, [None, 0] * 7, (None,) * 3)):
        rc = L.nmpc_policy_covariance_batch(None, B, nc, *ins, *outs)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, nc)
    a = vp(C.addressof(buf))
    rc = L.nmpc_policy_covariance_batch_dev(None, 1, 1, *([a, 0] * 7), *([a] * 3), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_covariance_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included last by nmpc_eval.hip, and the
    library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    inc = '#include "nmpc_policy_covariance.hip"'
    assert inc in text and text.rindex("#include") == text.index(inc)
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_policy_covariance.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


@functools.lru_cache(maxsize=None)
def _cases():
    """(name, b, prob, p, ubar (N, nu), Xbar, K, S0, W) per scenario, computed once."""
    out = []
    for name in pf.SOLVED:
        spec, prob, P, bounds, sols = sr.solved(name)
        assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
        dp = pf.directions(spec, len(sols), 95)[:, :1]
        for b in range(len(sols)):
            pol = pf.policy_of(name, b, dp)
            out.append([name, b, prob, P[b], sols[b]["x"].reshape(prob.N, prob.nu), pol["X"], pol["K"]])
    for name, which in SYNTHETIC:
        spec = er.case_spec(name)
        prob = er.problem_of(spec)
        B = er.CASES[name]
        d = er.draw_point(spec, B, seed=31)
        bounds = (d["lbx"], d["ubx"], d["lbg"], d["ubg"])
        dp = pf.directions(spec, B, 95)[:, :1]
        for b in which:
            pol = pf.dense_policy(prob, d["w"][b], d["lam_g"][b], d["lam_x"][b], d["p"][b], bounds, dp[b])
            out.append([name, b, prob, d["p"][b], d["w"][b].reshape(prob.N, prob.nu), pol["X"], pol["K"]])
    for i, c in enumerate(out):
        S0, W = cr.draw_covariances(c[2], 1, SIGMA, seed=5 + i)
        c += [S0[0], W[0]]
    return tuple(tuple(c) for c in out)


def _sampled(prob, p, ubar, Xbar, K, S0, W, eps):
    """Sigma (N + 1, nx, nx) and var_u (N, nu) from the +-eps sigma-point pairs on the plant."""
    N, nx, nu = prob.N, prob.nx, prob.nu
    Sig, vu = np.zeros((N + 1, nx, nx)), np.zeros((N, nu))
    for j, d in cr.sigma_points(S0, W, N):
        r = []
        for sgn in (1.0, -1.0):
            e0, w = np.zeros(nx), np.zeros((N, nx))
            if j == 0:
                e0 = sgn * eps * d
            else:
                w[j - 1] = sgn * eps * d
            r.append(rr.rollout_one(prob, p, ubar, Xbar, K, e0, w))
        dX = (r[0]["X"] - r[1]["X"]) / (2.0 * eps)
        dU = (r[0]["U"] - r[1]["U"]) / (2.0 * eps)
        Sig += np.einsum("ki,kj->kij", dX, dX)
        vu += dU * dU
    return Sig, vu


@functools.lru_cache(maxsize=None)
def _plant(i, eps=EPS):
    """The sigma-point sums of scenario i, computed once."""
    name, b, prob, p, ubar, Xbar, K, S0, W = _cases()[i]
    return _sampled(prob, p, ubar, Xbar, K, S0, W, eps)


def _figures(i, mutant=None, eps=EPS):
    """(largest over the stages of |sampled - checker| / max |Sigma_k|, the same for sigma_u^2 over the
    largest of them), the checker under `mutant`."""
    name, b, prob, p, ubar, Xbar, K, S0, W = _cases()[i]
    ref = cr.covariance_one(prob, p, ubar, Xbar, K, S0, W, mutant=mutant)
    Sig, vu = _plant(i, eps)
    top = np.max(np.abs(Sig), axis=(1, 2))
    fS = float(np.max(np.max(np.abs(Sig - ref["Sigma"]), axis=(1, 2)) / top))
    fU = float(np.max(np.abs(vu - ref["var_u"])) / np.max(np.abs(vu)))
    return fS, fU


def test_the_checker_agrees_with_the_plant():
    """Sigma_k and sigma_u^2 of the checker against the sigma-point sums, every scenario."""
    for i, c in enumerate(_cases()):
        fS, fU = _figures(i)
        print(f"{c[0]} scenario {c[1]}: |sampled - checker| / max |Sigma_k| = {fS:.2e}, sigma_u^2 {fU:.2e} (gate {GATE:.0e}, "
              f"eps {EPS:.0e})")
        assert fS <= GATE and fU <= GATE, (c[0], c[1], fS, fU)


@pytest.mark.parametrize("which", cr.MUTANTS)
def test_every_mutant_misses_the_gate(which):
    """Each mutant's Sigma misses the gate against the plant's on every scenario.  (`shift` at N = 1
    is no mutant -- there is no K_1 to take K_0's place -- and is left out there.)"""
    worst = np.inf
    for i, c in enumerate(_cases()):
        if which == "shift" and c[2].N == 1:
            continue
        fS, fU = _figures(i, mutant=which)
        print(f"{c[0]} scenario {c[1]}, mutant {which}: |sampled - mutant| / max |Sigma_k| = {fS:.2e}, sigma_u^2 {fU:.2e}")
        assert fS > GATE, (which, c[0], c[1], fS)
        worst = min(worst, fS)
    print(f"mutant {which}: smallest miss {worst:.2e}")


def test_tighten_on_cpu_tensors():
    """Infinite bounds untouched, finite ones moved by exactly kappa sigma, crossing pairs at their
    midpoint, fixed variables and equality rows unchanged, lower <= upper throughout."""
    import torch
    from nmpc_amd import policy

    B, nc, N, nu, m = 2, 2, 3, 2, 2
    g = torch.Generator().manual_seed(3)
    su = torch.rand((B, nc, N, nu), dtype=torch.float64, generator=g) * 0.1
    sgm = torch.rand((B, nc, N + 1, m), dtype=torch.float64, generator=g) * 0.1
    inf = float("inf")
    lbx = torch.tensor([-1.0, -inf, -1e19, 0.5, -1.0, 0.0], dtype=torch.float64)         # shared (nw,)
    ubx = torch.tensor([1.0, 2.0, 1e19, 0.5, -0.99, inf], dtype=torch.float64)
    lbg = torch.tensor([[-2.0, -inf, 1.0, 0.0, -1e20, 3.0, -5.0, 0.0]] * B, dtype=torch.float64)  # (B, ng)
    ubg = torch.tensor([[2.0, 0.0, 1.0, 1e-3, 4.0, 1e19, 5.0, 0.0]] * B, dtype=torch.float64)
    su[:, :, 2, 0] = 0.05  # lbx[4], ubx[4]: room 0.01 < 2 kappa sigma
    sgm[:, :, 1, 1] = 0.02  # lbg[3], ubg[3]: room 1e-3
    kappa = 2.0
    for case in (0, 1):
        nlx, nux, nlg, nug = policy.tighten(lbx, ubx, lbg, ubg, {"sigma_u": su, "sigma_g": sgm}, kappa, case=case)
        bu, bg = kappa * su[:, case].reshape(B, -1), kappa * sgm[:, case].reshape(B, -1)
        assert nlx.shape == nux.shape == (B, N * nu) and nlg.shape == nug.shape == (B, (N + 1) * m)
        for nl, nh, lo, hi, back in ((nlx, nux, lbx.expand(B, -1), ubx.expand(B, -1), bu), (nlg, nug, lbg, ubg, bg)):
            assert torch.all(nl <= nh)
            absent_l, absent_h = lo.abs() >= 1e19, hi.abs() >= 1e19
            fixed = lo == hi
            cross = ~fixed & ~absent_l & ~absent_h & (lo + back > hi - back)
            assert torch.equal(nl[absent_l], lo[absent_l]) and torch.equal(nh[absent_h], hi[absent_h])
            assert torch.equal(nl[fixed], lo[fixed]) and torch.equal(nh[fixed], hi[fixed])
            mid = 0.5 * (lo + hi)
            assert torch.equal(nl[cross], mid[cross]) and torch.equal(nh[cross], mid[cross])
            move_l, move_h = ~absent_l & ~fixed & ~cross, ~absent_h & ~fixed & ~cross
            assert torch.equal(nl[move_l], (lo + back)[move_l]) and torch.equal(nh[move_h], (hi - back)[move_h])
            print(f"case {case}: {int(absent_l.sum() + absent_h.sum())} absent, {int(2 * fixed.sum())} fixed, "
                  f"{int(2 * cross.sum())} crossing, {int(move_l.sum() + move_h.sum())} moved bounds")
            assert cross.any() and fixed.any() and move_l.any() and move_h.any() and absent_l.any() and absent_h.any()
