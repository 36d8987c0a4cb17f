"""The parameter-product entry points without a GPU: exported, argument checks before any
device call, part of the evaluation kernel's translation unit with their source under the build
hash -- and the checker of tests/test_gpu_param.py (tests/param_ref.py) shown to be right
against differences of the oracle, its gate shown to have teeth, and the basis of the tolerance
measured, all on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import eval_ref as er
from tests import param_ref as qr
from tests import products_ref as pr

NAMES = ("nmpc_param_products_batch", "nmpc_param_products_batch_dev")


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_param_products_batch(" in text and "int nmpc_param_products_batch_dev(" in text


def test_null_handle_is_invalid_for_both_entry_points():
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_param_products_batch(None, 1, 1, q, 0, q, 0, None, 0, 1.0, q, 0, q, q, q, q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_param_products_batch_dev(None, 1, 1, a, 0, a, 0, vp(0), 0, 1.0, a, 0, a, a, a, a, vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_param_products_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_kkt.hip, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_pproducts.hip"' in text
    assert text.index('#include "nmpc_kkt.hip"') < text.index('#include "nmpc_pproducts.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_pproducts.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


@pytest.mark.parametrize("name", list(er.CASES))
def test_the_checker_matches_differences_of_the_oracle(name):
    """tests/param_ref.py's dense dg/dp, d_p grad_w L, dX/dp and grad_p L against
    Richardson-extrapolated central differences of SSEval's g, sigma grad F + J' lam, X and L
    (relative steps 1e-4 and 2e-4 times max(1, |p_i|)), two scenarios per case, sigma 1 and
    0.37: within 1e-7 of each array's largest entry.  Measured: at most 1.7e-9 (Jp 9.2e-10,
    cross 2.7e-10, dX/dp 1.1e-10, grad_p L 1.7e-9), the differences' own rounding; a dropped term
    changes the cross derivative by 5e-4 to 1 of a column's largest entry (next test)."""
    spec, d, evs = pr.evals(name)
    prob = er.problem_of(spec)
    for b in range(2):
        for sig in (1.0, 0.37):
            dn = qr.dense(evs[b], sig, d["lam_g"][b])
            ri = qr.richardson(prob, d["w"][b], d["p"][b], sig, d["lam_g"][b])
            fig = {k: float(np.max(np.abs(dn[k] - ri[k])) / np.max(np.abs(dn[k]))) for k in ("Jp", "C", "Xp", "gp")}
            print(f"{name} scenario {b} sigma {sig}: checker vs Richardson, of the largest entry: "
                  + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
            assert all(v <= 1e-7 for v in fig.values()), (name, b, sig, fig)
    # entries of p that nothing reads: exactly zero columns / entries
    dn = qr.dense(evs[0], 1.0, d["lam_g"][0])
    for i, kind in enumerate(qr.entry_kinds(prob)):
        if kind is None:
            assert np.all(dn["Jp"][:, i] == 0) and np.all(dn["C"][:, i] == 0) and np.all(dn["Xp"][:, i] == 0)
            assert dn["gp"][i] == 0 and dn["gp_scale"][i] == 0


# the cases each dropped term is shown on, and the smallest / largest error over bound of
# d_p grad_w L measured over their scenarios (sigma = 1, lam_g random, the parity test's
# directions)
TEETH = [("cross0", "n1"),            # 5.7e9 .. 9.7e9
         ("cross0", "nmpc_tt"),       # 6.6e5 .. 6.0e7
         ("cross0", "race_track_2"),  # 2.0e8 .. 3.6e9
         ("cross0", "uav5"),          # 5.5e8 .. 1.3e9
         ("tshift", "race_track_2"),  # 4.4e8 .. 2.3e9
         ("tshift", "uav5"),          # 9.3e8 .. 3.7e9
         ("oshift", "dynamic"),       # 2.4e7 .. 3.2e8 (and dg/dp by 2.1e9)
         ("wgrad", "weights_in_p"),   # 6.1e8 .. 2.8e9
         ("dynxx", "race_track_2"),   # 6.5e8 .. 8.8e9
         ("dynxx", "dynamic")]        # 4.9e9 .. 7.0e9


@pytest.mark.parametrize("which,name", TEETH)
def test_the_gate_has_teeth_for_a_dropped_term(which, name):
    """A checker with one term dropped -- the stage-0 cross term Hxu_0' xi_0, the target's move,
    the obstacles' moves, the unit-weight gradient, or the dynamics' d2_xx on xi -- fails the
    comparison of tests/param_ref.py against the full one on every scenario of the case (the
    factors: TEETH above; no case had to be left out).  The full checker passes against itself,
    and the products the term is no part of still pass."""
    spec, d, ref = qr.reference(name)
    _, _, evs = pr.evals(name)
    combo = qr.COMBOS[0]
    for b, ev in enumerate(evs):
        good = ref[combo][b]
        assert max(qr.figures(good, good).values()) == 0.0
        mut = qr.cpu_products(ev, d["dp"][b], combo[0], d["lam_g"][b], which)
        fig = qr.figures(mut, good)
        print(f"{name} scenario {b}, dropped {which}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert fig["hp"] > 1.0, (which, name, b, fig)
        assert fig["dXp"] == 0.0 and fig["gp"] == 0.0
        assert (fig["jp"] > 1.0) if which == "oshift" else (fig["jp"] == 0.0)
        with pytest.raises(AssertionError):
            qr.check_against(mut, good, f"{name} dropped {which}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_one_ulp_basis_of_the_tolerance(name):
    """Every entry of w and p moved by one ulp (random sign), three draws per scenario, sigma 1
    and 0.37: how far the checker's four products move, relative to the gate's scales.  The
    figures are in tests/param_ref.py's docstring; the gate must keep 100x over them."""
    from oracle import nmpc_oracle as orc

    spec, d, ref = qr.reference(name)
    prob = er.problem_of(spec)
    rng = np.random.default_rng(5)
    worst = {}
    for b in range(er.CASES[name]):
        for combo in qr.COMBOS[:2]:
            for _ in range(3):
                w, p = d["w"][b], d["p"][b]
                w2 = np.where(rng.random(w.shape) < 0.5, np.nextafter(w, np.inf), np.nextafter(w, -np.inf))
                p2 = np.where(rng.random(p.shape) < 0.5, np.nextafter(p, np.inf), np.nextafter(p, -np.inf))
                moved = qr.cpu_products(orc.SSEval(prob, w2, p2), d["dp"][b], combo[0], d["lam_g"][b])
                for k, v in qr.figures(moved, ref[combo][b]).items():
                    worst[k] = max(worst.get(k, 0.0), v * qr.TOL)
    print(f"{name}: one ulp of w and p moves, of the scale: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v <= qr.TOL / 100 for v in worst.values()), (name, worst)
