"""The adjoint-product entry points without a GPU: exported, argument checks before any device
call, part of the evaluation kernel's translation unit with their source under the build hash --
and the checker of tests/test_gpu_adjoint.py (tests/adjoint_ref.py) shown to be the transpose of
the two forward checkers, its gate shown to have teeth, and the basis of the tolerance measured,
all on the oracle alone."""
import ctypes as C
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import adjoint_ref as ar
from tests import eval_ref as er
from tests import param_ref as qr
from tests import products_ref as pr

NAMES = ("nmpc_adjoint_products_batch", "nmpc_adjoint_products_batch_dev")


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_adjoint_products_batch(" in text and "int nmpc_adjoint_products_batch_dev(" in text


def test_null_handle_is_invalid_for_both_entry_points():
    """NMPC_E_INVALID before anything is read or written.  The other invalid-argument cases need
    a live handle, which needs a device: tests/test_gpu_adjoint.py::
    test_argument_validation_on_a_live_handle runs every one of them on both entry points."""
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_adjoint_products_batch(None, 1, 1, q, 0, q, 0, None, 0, 1.0, q, 0, q, 0, q, 0, q, q)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_adjoint_products_batch_dev(None, 1, 1, a, 0, a, 0, vp(0), 0, 1.0, a, 0, a, 0, a, 0, a, a, vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    # ... whatever else is wrong with the call
    rc = L.nmpc_adjoint_products_batch(None, 0, 0, None, 0, None, 0, None, 0, 1.0, None, 0, None, 0, None, 0, None, None)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_adjoint_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_pproducts.hip, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_adjoint.hip"' in text
    assert text.index('#include "nmpc_pproducts.hip"') < text.index('#include "nmpc_adjoint.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_adjoint.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


def _scn(d, b, keys=ar.SEEDS):
    return {k: (d[k][b] if k in keys else None) for k in ar.SEEDS}


@pytest.mark.parametrize("name", list(er.CASES))
def test_the_checker_is_the_transpose_of_the_forward_checkers(name):
    """<y, jv> + <z, hv> + <Xb, dX> = <wbar, v> against products_ref.cpu_products and
    <y, jp> + <z, hp> + <Xb, dXp> = <pbar, dp> against param_ref.cpu_products, on their own
    directions, every scenario and (obj_factor, lam_g) combination: within TOL of the sum of the
    absolute terms.  An entry of p that nothing reads has an exactly zero pbar and scale."""
    spec, d, dn = ar.reference(name)
    _, dv, rv = pr.reference(name)
    _, dq, rq = qr.reference(name)
    kinds = qr.entry_kinds(er.problem_of(spec))
    worst = 0.0
    for combo in ar.COMBOS:
        for b in range(er.CASES[name]):
            s = _scn(d, b)
            adj = ar.products_of(dn[combo][b], **s)
            for fwd, dirs, out, keys in ((rv[combo][b], dv["v"][b], "wbar", ("jv", "hv", "dX")),
                                         (rq[combo][b], dq["dp"][b], "pbar", ("jp", "hp", "dXp"))):
                for a in range(ar.NA):
                    for j in range(dirs.shape[0]):
                        terms = [s[sk][a] * fwd[fk][j] for sk, fk in zip(ar.SEEDS, keys)]
                        lhs = sum(float(np.sum(t)) for t in terms)
                        rt = adj[out][a] * dirs[j]
                        den = sum(float(np.sum(np.abs(t))) for t in terms) + float(np.sum(np.abs(rt)))
                        worst = max(worst, abs(lhs - float(np.sum(rt))) / (ar.TOL * den))
            for i, kind in enumerate(kinds):
                if kind is None:
                    assert np.all(adj["pbar"][:, i] == 0.0) and np.all(adj["scale"]["pbar"][:, i] == 0.0), i
    print(f"{name}: dot-product identities, largest defect / bound {worst:.2e}")
    assert worst <= 1.0, (name, worst)


# the cases each dropped term is shown on (tests/test_param_capi.py's, with n1 for the stage-0
# cross term), and the smallest / largest error over bound of pbar for the z seed alone measured
# over their scenarios (sigma = 1, lam_g random, the parity test's seeds)
TEETH = [("cross0", "n1"),            # 1.0e10 (N = 1: C' z is this term alone)
         ("cross0", "nmpc_tt"),       # 3.3e5 .. 3.2e7
         ("cross0", "race_track_2"),  # 1.4e8 .. 2.3e9
         ("cross0", "uav5"),          # 2.6e8 .. 2.8e9
         ("tshift", "race_track_2"),  # 3.0e9 .. 8.3e9
         ("tshift", "uav5"),          # 3.3e9 .. 8.8e9
         ("oshift", "dynamic"),       # 6.0e9 .. 8.3e9
         ("wgrad", "weights_in_p"),   # 5.5e9 .. 9.0e9
         ("dynxx", "race_track_2"),   # 3.5e9 .. 9.4e9
         ("dynxx", "dynamic")]        # 4.0e9 .. 7.9e9


@pytest.mark.parametrize("which,name", TEETH)
def test_the_gate_has_teeth_for_a_dropped_term(which, name):
    """A checker built from param_ref.dense with one term dropped -- the stage-0 cross term
    Hxu_0' xi_0, the target's move, the obstacles' moves, the unit-weight gradient, or the
    dynamics' d2_xx on xi -- misses the gate on pbar for the z seed alone on every scenario of the
    case (the factors: TEETH above; no case had to be left out).  The full checker passes against
    itself, and wbar, which holds no parameter derivative, is untouched."""
    spec, d, dn = ar.reference(name)
    _, _, evs = pr.evals(name)
    combo = ar.COMBOS[0]
    for b, ev in enumerate(evs):
        good = ar.products_of(dn[combo][b], z=d["z"][b])
        assert max(ar.figures(good, good).values()) == 0.0
        mut = ar.products_of(ar.dense(ev, combo[0], d["lam_g"][b], which), z=d["z"][b])
        fig = ar.figures(mut, good)
        print(f"{name} scenario {b}, dropped {which}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
        assert fig["pbar"] > 1.0, (which, name, b, fig)
        assert fig["wbar"] == 0.0
        with pytest.raises(AssertionError):
            ar.check_against(mut, good, f"{name} dropped {which}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_one_ulp_basis_of_the_tolerance(name):
    """Every entry of w and p moved by one ulp (random sign), three draws per scenario, sigma 1
    and 0.37, all three seeds together: how far the checker's wbar and pbar move, relative to
    the gate's scales.  The figures are in tests/adjoint_ref.py's docstring; the gate must keep
    100x over them."""
    from oracle import nmpc_oracle as orc

    spec, d, dn = ar.reference(name)
    prob = er.problem_of(spec)
    rng = np.random.default_rng(5)
    worst = {}
    for b in range(er.CASES[name]):
        for combo in ar.COMBOS[:2]:
            ref = ar.products_of(dn[combo][b], **_scn(d, b))
            for _ in range(3):
                w, p = d["w"][b], d["p"][b]
                w2 = np.where(rng.random(w.shape) < 0.5, np.nextafter(w, np.inf), np.nextafter(w, -np.inf))
                p2 = np.where(rng.random(p.shape) < 0.5, np.nextafter(p, np.inf), np.nextafter(p, -np.inf))
                moved = ar.products_of(ar.dense(orc.SSEval(prob, w2, p2), combo[0], d["lam_g"][b]), **_scn(d, b))
                for k, v in ar.figures(moved, ref).items():
                    worst[k] = max(worst.get(k, 0.0), v * ar.TOL)
    print(f"{name}: one ulp of w and p moves, of the scale: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    assert all(v <= ar.TOL / 100 for v in worst.values()), (name, worst)
