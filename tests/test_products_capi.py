"""The product entry points without a GPU: exported, argument checks before any device call,
part of the evaluation kernel's translation unit with their source under the build hash --
and the gate of tests/test_gpu_products.py shown to have teeth on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import products_ref as pr


def test_both_symbols_are_exported():
    L = _lib.lib()
    for name in ("nmpc_products_batch", "nmpc_products_batch_dev"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_products_batch(" in text and "int nmpc_products_batch_dev(" in text


def test_null_handle_is_invalid_for_both_entry_points():
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_products_batch(None, 1, 1, q, 0, q, 0, None, 0, 1.0, q, 0, q, q, q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_products_batch_dev(None, 1, 1, a, 0, a, 0, vp(0), 0, 1.0, a, 0, a, a, a, vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_products_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the products kernel's file is included by nmpc_eval.hip,
    and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        assert '#include "nmpc_products.hip"' in fh.read()
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_products.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    moved = ge.source_hash()
    assert moved != before
    # and the file the unit's kernels share
    with open(copy / "nmpc_eval_shared.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() not in (before, moved)


# the cases each mutant is shown on: ones where the mutated term exists (every case has
# dynamics, and every case but n1 a stage cost whose state depends on w; only cases with
# obstacles have row curvature)
@pytest.mark.parametrize("which,name", [("dyn_hess", "race_track_2"), ("dyn_hess", "uav5"), ("Hg", "n63_16obs"),
                                        ("Hg", "dynamic"), ("Hg", "n1"), ("Hxu", "nmpc_tt"), ("Hxu", "uav5")])
def test_the_gate_has_teeth_for_a_dropped_term(which, name):
    """A reference with one term of its Hessian dropped -- the dynamics' second derivatives,
    the obstacle curvature, or the state-control cross term -- fails the comparison of
    tests/products_ref.py against the unmutated reference, on every scenario of the case, on
    the parity test's own directions with (obj_factor, lam_g) = (1, random).  The unmutated
    reference passes against itself, and the Jacobian and tangent products (untouched by the
    mutations) still pass."""
    spec, d, ref = pr.reference(name)
    _, _, evs = pr.evals(name)
    combo = pr.COMBOS[0]
    for b, ev in enumerate(evs):
        good = ref[combo][b]
        assert max(pr.figures(good, good).values()) == 0.0
        mut = pr.mutant_products(ev, d["v"][b], combo[0], d["lam_g"][b], which)
        fig = pr.figures(mut, good)
        print(f"{name} scenario {b}, mutant {which}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert fig["hv"] > 1.0, (which, name, b, fig)
        assert fig["jv"] <= 1.0 and fig["dX"] <= 1.0
        with pytest.raises(AssertionError):
            pr.check_against(mut, good, f"{name} mutant {which}")
    # the mutation did not leak into the shared reference
    again = pr.cpu_products(evs[0], d["v"][0], combo[0], d["lam_g"][0])
    assert max(pr.figures(again, ref[combo][0]).values()) == 0.0


@pytest.mark.parametrize("name", ["race_track_2", "nmpc_tt", "n63_16obs", "dynamic", "weights_in_p", "uav5"])
def test_the_gate_has_teeth_for_one_entry_off_by_1e_7(name):
    """One stage-cost Hessian entry of one stage (the largest) off by 1e-7 relative.
      * The dense-extraction gate (identity directions, each column against its own largest
        entry) catches it on every scenario of every multi-stage case, by 58x to 1,000x
        (measured here; 1,000x = the entry alone sets its column's scale).
      * The parity test's random directions spread the bound over the whole of |W| |v|, so one
        entry of one stage is at the edge of that gate: 0.3x to 22x the bound over the
        scenarios (measured).  The case as a whole -- the test asserts every scenario -- still
        fails on each of the six cases, which is what is asserted here."""
    spec, d, ref = pr.reference(name)
    _, _, evs = pr.evals(name)
    combo = pr.COMBOS[0]
    eye = np.eye(spec.nw)
    rnd = []
    for b, ev in enumerate(evs):
        dense = pr.figures(pr.mutant_products(ev, eye, 1.0, d["lam_g"][b], "Hl"),
                           pr.cpu_products(ev, eye, 1.0, d["lam_g"][b]))
        fig = pr.figures(pr.mutant_products(ev, d["v"][b], combo[0], d["lam_g"][b], "Hl"), ref[combo][b])
        print(f"{name} scenario {b}, Hl entry x (1 + 1e-7): error / bound, dense {dense['hv']:.2e}, "
              f"random directions {fig['hv']:.2e}")
        assert dense["hv"] > 1.0 and dense["jv"] == 0.0 and dense["dX"] == 0.0, (name, b, dense)
        rnd.append(fig["hv"])
    assert max(rnd) > 1.0, (name, rnd)
