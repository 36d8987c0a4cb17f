"""The feedback-policy entry points without a GPU: exported, declared, argument checks before any
device call, part of the evaluation kernel's translation unit with their source under the build
hash -- and the checker of tests/test_gpu_policy.py (tests/policy_ref.py) shown to pass its own
gates (a) and (c), with every mutant missing the gate named for it on every scenario, all on the
oracle alone.  The measured figures are printed wherever the suite runs."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import policy_ref as pf
from tests import solve_adjoint_ref as sr

NAMES = ("nmpc_solve_policy_batch", "nmpc_solve_policy_batch_dev")


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_solve_policy_batch(" in text and "int nmpc_solve_policy_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever
    else is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_policy.py::test_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    for B, nd, ins, outs in ((1, 1, [q, 0] * 10, (q,) * 5), (0, 1, [q, 0] * 10, (q,) * 5), (1, -1, [q, 0] * 10, (q,) * 5),
                             (1, 0, [q, 0] * 10, (q,) * 5), (1, 1, [q, -1] * 10, (q,) * 5),
                             (1, 1, [None, 0] * 10, (None,) * 5)):
        rc = L.nmpc_solve_policy_batch(None, B, nd, *ins, *outs, C.cast(buf, ip), q)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, nd)
    a = vp(C.addressof(buf))
    rc = L.nmpc_solve_policy_batch_dev(None, 1, 1, *([a, 0] * 10), *([a] * 7), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_policy_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_solve_tangent.hip (both on nmpc_point.hip's LDS carve-up and workspace slices), and the
    library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_solve_policy.hip"' in text
    assert text.index('#include "nmpc_solve_tangent.hip"') < text.index('#include "nmpc_solve_policy.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_solve_policy.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


LADDERS = {"1e-4": sr.LADDER, "1e-12": pf.LADDER_FINE}


def _cases():
    for name in pf.SOLVED:
        spec, prob, P, bounds, sols = sr.solved(name)
        assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
        yield name, spec, prob, pf.directions(spec, len(sols), 95), len(sols)


@pytest.mark.parametrize("rung", list(LADDERS))
def test_the_checker_passes_its_own_gates(rung):
    """Oracle solutions of the four solved cases (13 scenarios), dp = I and two N(0, 1) directions,
    the dense ladder started at 1e-4 and at 1e-12: gate (a) holds at either delta; from 1e-12 every
    scenario factorises at the first rung and gate (c) holds."""
    worst_a = worst_c = 0.0
    for name, spec, prob, dp, B in _cases():
        for b in range(B):
            ref = pf.policy_of(name, b, dp, ladder=LADDERS[rung])
            fa = pf.gate_a(ref, ref, dp[b])
            nx = prob.nx
            fc = pf.gate_c(ref["kff"], nx)
            print(f"{name} scenario {b}, ladder from {rung}: delta {ref['delta']:.3g}, gate (a) {fa:.2e} (bound "
                  f"{pf.TOL_A:.0e}), max|kff_0| {fc:.2e} ({fc / ref['delta']:.2f} delta)")
            assert fa <= pf.TOL_A, (name, b, fa)
            worst_a, worst_c = max(worst_a, fa), max(worst_c, fc / ref["delta"])
            if rung == "1e-12":
                assert ref["delta"] == 1e-12, (name, b, ref["delta"])
                assert fc <= pf.C_FACTOR * ref["delta"], (name, b, fc)
    print(f"ladder from {rung}: largest gate (a) {worst_a:.2e}, max|kff_0| / delta {worst_c:.2f}")


@pytest.mark.parametrize("which", pf.MUTANTS)
def test_every_mutant_misses_the_gate_named_for_it(which):
    """A checker with one part wrong (tests/policy_ref.py: MUTANTS) misses its gate on every one of
    the 13 scenarios: gate (a) at the default ladder's delta and at 1e-12 for noS, rawk, shift and
    transpose; gate (c) at 1e-12 for noS0, which gate (a) cannot see (dw^_0 = k_0 whatever K_0 is:
    its figure there is printed)."""
    gate = pf.GATE_OF[which]
    lo = np.inf
    for name, spec, prob, dp, B in _cases():
        for b in range(B):
            for rung in (("1e-12",) if gate == "c" else tuple(LADDERS)):
                ref = pf.policy_of(name, b, dp, ladder=LADDERS[rung])
                mut = pf.policy_of(name, b, dp, mutant=which, delta=ref["delta"])
                mut = dict(mut, A=ref["A"], B=ref["B"])
                fa = pf.gate_a(mut, ref, dp[b])
                fc = pf.gate_c(mut["kff"], prob.nx)
                print(f"{name} scenario {b}, mutant {which}, delta {ref['delta']:.3g}: gate (a) {fa:.2e} (bound "
                      f"{pf.TOL_A:.0e}), max|kff_0| {fc:.2e} (bound {pf.C_FACTOR * ref['delta']:.1e})")
                if gate == "a":
                    assert fa > pf.TOL_A, (which, name, b, rung, fa)
                    lo = min(lo, fa / pf.TOL_A)
                else:
                    assert ref["delta"] <= pf.C_DELTA
                    assert fc > pf.C_FACTOR * ref["delta"], (which, name, b, fc)
                    lo = min(lo, fc / (pf.C_FACTOR * ref["delta"]))
    print(f"mutant {which}: smallest figure / bound of gate ({gate}) {lo:.2e}")
