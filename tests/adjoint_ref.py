"""Checker side of the adjoint-product tests (tests/test_gpu_adjoint.py,
tests/test_adjoint_capi.py): the transposes of the oracle's dense J, W, Z (tests/products_ref.py:
SSEval.J, hessian, Z) and Jp = dg/dp, C = d_p grad_w L, Xp = dX/dp (tests/param_ref.py: dense)
applied to seeds, on the cases and points of tests/eval_ref.py; the scales of the tolerance and
the comparison.  The six matrices are pinned to Richardson-extrapolated differences of the
oracle's function layer by tests/test_products_capi.py and tests/test_param_capi.py.

  wbar = J' y + W' z + Z' Xb         pbar = Jp' y + C' z + Xp' Xb

Seeds: y (ng), z (nw), Xb (nX) ~ N(0, 1) per entry, NA = 3 per scenario.

Tolerance eval_ref.TOL = 1e-10: wbar per seed relative to max_i (|J|' |y| + |W|' |z| + |Z|' |Xb|)_i,
pbar per entry relative to the same sum of absolute terms (|Jp|' |y| + |C|' |z| + |Xp|' |Xb|)_i --
entries of p have different units, as for grad_p L.  Where a scale is exactly 0 the result must
be exactly 0.

Basis of the tolerance, measured on the CPU (tests/test_adjoint_capi.py::
test_one_ulp_basis_of_the_tolerance prints it): a one-ulp change of every entry of w and p,
three draws per scenario, sigma 1 and 0.37, lam_g random, all three seeds together, moves the
checker's products by at most
                   wbar     pbar     (of the scale)
  race_track_2   6.3e-16  2.4e-14
  nmpc_tt        3.7e-15  3.7e-15
  n63_16obs      7.5e-16  1.3e-15
  n1             2.8e-16  4.7e-16
  dynamic        6.2e-16  1.4e-14
  weights_in_p   6.6e-16  1.1e-14
  uav5           1.0e-15  2.2e-14
so 1e-10 leaves at least 4,000x on every case for a different operation order.  `n1`, whose
forward Hessian product cancels inside one entry (tests/products_ref.py: margin 140x), is not
special here: with N(0, 1) seeds on g and X the scale of wbar's single stage is dominated by
J' y and Z' Xb, which do not cancel."""
from __future__ import annotations

import functools

import numpy as np

from tests import eval_ref as er
from tests import param_ref as qr
from tests import products_ref as pr

TOL = er.TOL
NA = 3
COMBOS = pr.COMBOS
KEYS = ("wbar", "pbar")
SEEDS = ("y", "z", "Xb")


def draw_seeds(spec, B, na, seed):
    """y (B, na, ng), z (B, na, nw), Xb (B, na, nX): N(0, 1) per entry."""
    rng = np.random.default_rng(seed)
    return {"y": rng.standard_normal((B, na, spec.ng)), "z": rng.standard_normal((B, na, spec.nw)),
            "Xb": rng.standard_normal((B, na, spec.nX))}


def dense(ev, obj_factor, lam_g, drop=None):
    """One scenario on the oracle: the six matrices whose transposes are applied.  lam_g None =
    zeros; drop: one of param_ref.MUTANTS, that term of C (and, for the obstacles' moves, of Jp)
    left out."""
    lg = np.zeros(ev.prob.ng) if lam_g is None else lam_g
    dn = qr.dense(ev, obj_factor, lam_g, drop)
    return {"J": ev.J, "W": ev.hessian(obj_factor, lg), "Z": pr.stack_Z(ev), "Jp": dn["Jp"], "C": dn["C"],
            "Xp": dn["Xp"]}


def products_of(dn, y=None, z=None, Xb=None):
    """Seeds (na, n) or None -> wbar (na, nw), pbar (na, np) and the scales: (na,) for wbar, (na, np)
    for pbar."""
    terms = [(s, dn[a], dn[b]) for s, a, b in ((y, "J", "Jp"), (z, "W", "C"), (Xb, "Z", "Xp")) if s is not None]
    assert terms, "no seed"
    wbar = sum(s @ A for s, A, _ in terms)
    pbar = sum(s @ Ap for s, _, Ap in terms)
    ws = sum(np.abs(s) @ np.abs(A) for s, A, _ in terms)
    ps = sum(np.abs(s) @ np.abs(Ap) for s, _, Ap in terms)
    return {"wbar": wbar, "pbar": pbar, "scale": {"wbar": np.max(ws, axis=1), "pbar": ps}}


@functools.lru_cache(maxsize=None)
def reference(name, seed=2024):
    """(spec, inputs incl. seeds "y", "z", "Xb" (B, NA, n), {combo: [per-scenario dense matrices]})."""
    spec, d, evs = pr.evals(name, seed)
    d = dict(d, **draw_seeds(spec, er.CASES[name], NA, seed + 17))
    dn = {c: [dense(ev, c[0], d["lam_g"][b] if c[1] else None) for b, ev in enumerate(evs)] for c in COMBOS}
    return spec, d, dn


def figures(got, ref):
    """Largest error of each product over its bound TOL * scale (wbar per seed, pbar per entry);
    where the scale is exactly 0 (no term exists) the result must be exactly 0."""
    fig = {}
    for k in KEYS:
        if got.get(k) is None:
            continue
        a, r, s = np.asarray(got[k], float), ref[k], ref["scale"][k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err = np.abs(a - r) if k == "pbar" else np.max(np.abs(a - r), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(s > 0, err / (TOL * s), np.where(err == 0, 0.0, np.inf))
        fig[k] = float(np.max(np.where(np.isnan(err), np.inf, q)))
    return fig


def check_against(got, ref, what=""):
    """got: one scenario's wbar (na, nw) and / or pbar (na, np).  Prints every figure before asserting."""
    fig = figures(got, ref)
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return fig
