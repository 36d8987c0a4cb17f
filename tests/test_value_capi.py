"""The policy-value entry points without a GPU: exported, declared, a NULL handle refused before any
device call, the kernel part of the evaluation unit with its source under the build hash -- and the
checker of tests/test_gpu_value.py (tests/value_ref.py) held against the nonlinear plant on the oracle
alone:

  sigma points   the columns d of the Cholesky factors of S0 (into e0) and, at each stage, of W (into
                 w) are fed as +-eps pairs through tests/rollout_ref.rollout_one, unclamped; then
                     sum over the pairs of (J+ + J- - 2 J0) / (2 eps^2)   is dJ   up to O(eps^2)
                     sum over the pairs of ((J+ - J-) / (2 eps))^2        is varJ up to O(eps^2)
                 Gate for dJ, at eps = 1e-2:  |sampled - dJ| <= 1e-4 A + 4 n_pairs |J0| 2^-52 / eps^2
                 with A the sum over the pairs of |1/2 d' P_j d| (dJ itself cancels: on n63_16obs it is
                 0.003 beside A = 0.27) and the second term the rounding floor of a second difference
                 of J.  Gate for varJ, at eps = 1e-3: relative 1e-6.
  mutants        `nodyn` and `shift` miss the dJ gate on every scenario with N > 1, `nocross` on both
                 n63_16obs scenarios (on the solved plans the speed control sits on its bound and its
                 gain row is ~0), `transpose` on every gimbal-model scenario with N > 1 (one uav5
                 scenario passes); all with feedback.  At N = 1 every mutant coincides with the checker.

Scenarios: tests/test_covariance_capi.py's (the 13 solved ones with the dense-oracle policy, n1 and two
of n63_16obs at draw_point(seed=31), covariances from draw_covariances(seed=5 + i)), with feedback and
open loop.  nmpc_amd.policy.expected_cost is checked on a stub solver with CPU tensors.  The measured
figures are printed wherever the suite runs."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import covariance_ref as cr
from tests import rollout_ref as rr
from tests import test_covariance_capi as tcc
from tests import value_ref as vr

NAMES = ("nmpc_policy_value_batch", "nmpc_policy_value_batch_dev")
EPS_DJ, EPS_VAR = 1e-2, 1e-3
GATE_DJ, GATE_VAR = 1e-4, 1e-6
_cases = tcc._cases  # (name, b, prob, p, ubar, Xbar, K, S0, W) per scenario, computed once per session


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        # (handle, B, nc), six (pointer, leading dimension) pairs, five outputs [, stream]
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 20 + (name.endswith("_dev"))
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_policy_value_batch(" in text and "int nmpc_policy_value_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever else
    is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_value.py::test_gate_f_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    for B, nc, ins, outs in ((1, 1, [q, 0] * 6, (q,) * 5), (0, 1, [q, 0] * 6, (q,) * 5), (1, -1, [q, 0] * 6, (q,) * 5),
                             (1, 0, [q, 0] * 6, (q,) * 5), (1, 1, [q, -1] * 6, (q,) * 5),
                             (1, 1, [None, 0] * 6, (None,) * 5)):
        rc = L.nmpc_policy_value_batch(None, B, nc, *ins, *outs)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, nc)
    a = vp(C.addressof(buf))
    rc = L.nmpc_policy_value_batch_dev(None, 1, 1, *([a, 0] * 6), *([a] * 5), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_value_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip right after the
    rollouts' reverse sweep, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        incs = [ln.strip() for ln in fh if ln.startswith("#include")]
    at = incs.index('#include "nmpc_policy_value.hip"')
    assert incs[at - 1] == '#include "nmpc_policy_rollout_adjoint.hip"'
    assert incs[at + 1] == '#include "nmpc_policy_covariance.hip"' and at + 2 == len(incs)
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_policy_value.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


def sampled_sums(roll, prob, S0, W, eps):
    """(second-difference sum, squared-first-difference sum, J0, number of pairs) of the +-eps sigma-
    point pairs; roll(e0 (nx,), w (N, nx)) returns J."""
    N, nx = prob.N, prob.nx
    J0 = roll(np.zeros(nx), np.zeros((N, nx)))
    d2, d1, n = 0.0, 0.0, 0
    for j, d in cr.sigma_points(S0, W, N):
        Jp = []
        for sgn in (1.0, -1.0):
            e0, w = np.zeros(nx), np.zeros((N, nx))
            if j == 0:
                e0 = sgn * eps * d
            else:
                w[j - 1] = sgn * eps * d
            Jp.append(roll(e0, w))
        d2 += (Jp[0] + Jp[1] - 2.0 * J0) / (2.0 * eps * eps)
        d1 += ((Jp[0] - Jp[1]) / (2.0 * eps)) ** 2
        n += 1
    return d2, d1, J0, n


@functools.lru_cache(maxsize=None)
def _plant(i, fb):
    """The sigma-point sums of scenario i with feedback (fb) or open loop, computed once: dJ's at EPS_DJ,
    varJ's at EPS_VAR."""
    name, b, prob, p, ubar, Xbar, K, S0, W = _cases()[i]

    def roll(e0, w):
        return rr.rollout_one(prob, p, ubar, Xbar, K if fb else None, e0, w)["J"]

    d2, _, J0, n = sampled_sums(roll, prob, S0, W, EPS_DJ)
    _, d1, _, _ = sampled_sums(roll, prob, S0, W, EPS_VAR)
    return d2, d1, J0, n


def dj_gate(A, n_pairs, J0, eps=EPS_DJ):
    return GATE_DJ * A + 4.0 * n_pairs * abs(J0) * 2.0 ** -52 / eps ** 2


def _figures(i, fb, mutant=None):
    """(|sampled - dJ| / gate, |sampled - varJ| / varJ) of the checker under `mutant`; the gate's A is
    the checker's own."""
    name, b, prob, p, ubar, Xbar, K, S0, W = _cases()[i]
    ref = vr.value_one(prob, p, ubar, Xbar, K if fb else None, mutant=mutant)
    mo = vr.moments(ref, S0, W)
    A, V, n = vr.pair_scales(ref, S0, W, prob.N)
    d2, d1, J0, npairs = _plant(i, fb)
    assert n == npairs
    return abs(d2 - mo["dJ"]) / dj_gate(A, npairs, J0), abs(d1 - mo["varJ"]) / abs(mo["varJ"]), mo, A


def test_the_checker_agrees_with_the_plant():
    """dJ and varJ of the checker against the sigma-point sums, every scenario, with feedback and open
    loop."""
    worst = [0.0, 0.0]
    for i, c in enumerate(_cases()):
        for fb in (True, False):
            fD, fV, mo, A = _figures(i, fb)
            print(f"{c[0]} scenario {c[1]} {'feedback' if fb else 'open loop'}: dJ {mo['dJ']:.3e} (A {A:.3e}), "
                  f"|sampled - dJ| / gate = {fD:.3f}; varJ {mo['varJ']:.3e}, relative error {fV:.2e} (gate {GATE_VAR:.0e})")
            assert fD <= 1.0 and fV <= GATE_VAR, (c[0], c[1], fb, fD, fV)
            worst = [max(worst[0], fD), max(worst[1], fV)]
    print(f"largest dJ error / gate {worst[0]:.3f}, largest varJ relative error {worst[1]:.2e}")


def _asserted(which, c):
    name, prob = c[0], c[2]
    if prob.N == 1:
        return False
    if which == "nocross":
        return name == "n63_16obs"
    if which == "transpose":
        return prob.model != "uav5"
    return True


@pytest.mark.parametrize("which", vr.MUTANTS)
def test_every_mutant_misses_the_gate(which):
    """Each mutant's dJ misses the gate against the plant's, with feedback, on the scenarios the module
    docstring names for it."""
    worst, seen = np.inf, 0
    for i, c in enumerate(_cases()):
        if c[2].N == 1:
            continue
        fD = _figures(i, True, mutant=which)[0]
        on = _asserted(which, c)
        print(f"{c[0]} scenario {c[1]}, mutant {which}: |sampled - mutant| / gate = {fD:.3e}{'' if on else ' (not asserted)'}")
        if on:
            assert fD > 1.0, (which, c[0], c[1], fD)
            worst, seen = min(worst, fD), seen + 1
    assert seen >= 2
    print(f"mutant {which}: smallest miss {worst:.3e} x the gate over {seen} scenarios")


def test_mutants_coincide_with_the_checker_at_n1():
    """N = 1: lam_1 = P_1 = 0, so P_0 is the stage cost's Hessian whatever K and the dynamics."""
    for c in _cases():
        name, b, prob, p, ubar, Xbar, K, S0, W = c
        if prob.N != 1:
            continue
        ref = vr.value_one(prob, p, ubar, Xbar, K)
        for which in vr.MUTANTS + (None,):
            for Kq in (K, None):
                got = vr.value_one(prob, p, ubar, Xbar, Kq, mutant=which)
                assert np.array_equal(got["P"], ref["P"]) and np.array_equal(got["lam"], ref["lam"]), which


def test_expected_cost_on_cpu_tensors():
    """policy.expected_cost passes pol["raw"] and sol["x"] on, drops the gains with feedback=False and
    adds EJ = J + dJ when both are there."""
    import torch
    from nmpc_amd import policy

    B, nc = 3, 2
    g = torch.Generator().manual_seed(4)
    J = torch.rand((B,), dtype=torch.float64, generator=g)
    dJ = torch.rand((B, nc), dtype=torch.float64, generator=g) - 0.5
    seen = {}

    class Stub:
        def policy_value_device(self, p, ubar, Xbar, K, S0=None, W=None, out=None, want=(), stream=None):
            seen.update(p=p, ubar=ubar, Xbar=Xbar, K=K, S0=S0, W=W, out=out, want=want, stream=stream)
            res = {"J": J, "dJ": dJ, "varJ": dJ * dJ}
            return {k: v for k, v in res.items() if k in want}

    raw = {"X": torch.zeros((B, 4, 5), dtype=torch.float64), "K": torch.ones((B, 3, 5, 3), dtype=torch.float64)}
    pol, sol = {"raw": raw}, {"x": torch.zeros((B, 9), dtype=torch.float64)}
    p, S0, W = torch.zeros((B, 7)), torch.zeros((nc, 5, 5)), torch.ones((nc, 5, 5))
    res = policy.expected_cost(Stub(), pol, sol, p, S0, W=W)
    assert seen["K"] is raw["K"] and seen["Xbar"] is raw["X"] and seen["S0"] is S0 and seen["W"] is W and seen["p"] is p
    assert torch.equal(seen["ubar"], sol["x"]) and seen["want"] == ("J", "dJ", "varJ")
    assert set(res) == {"J", "dJ", "varJ", "EJ"} and res["EJ"].shape == (B, nc)
    assert torch.equal(res["EJ"], J.unsqueeze(1) + dJ)
    res = policy.expected_cost(Stub(), pol, sol, p, S0, feedback=False, want=("dJ", "varJ"))
    assert seen["K"] is None and seen["W"] is None and set(res) == {"dJ", "varJ"}
    res = policy.expected_cost(Stub(), pol, sol, p, S0, want=("J",))
    assert set(res) == {"J"}
