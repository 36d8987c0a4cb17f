"""Checker side of the Jacobian- / Hessian-vector product tests (tests/test_gpu_products.py,
tests/test_products_capi.py): the oracle's second-order layer (oracle.nmpc_oracle.SSEval: J,
hessian(obj_factor, lam_g), Z) applied to directions, on the cases and points of
tests/eval_ref.py, the scales of the tolerance, the comparison, and mutants of the reference.

Directions: v ~ N(0, 1) * max(1e-3, 0.1 (ubx - lbx)), one set per scenario.

Tolerance eval_ref.TOL = 1e-10, relative to the absolute-product scales of each direction,
max_i (|W| |v|)_i, max_i (|J| |v|)_i and max_i (|Z| |v|)_i -- not to |W v|, which can be far
smaller (max |W v| is 0.1 to 0.75 of the scale on these points, and cancels further in single
components).  Measured on the CPU on all seven cases with these scales (nv = 3, obj_factor 1
and 0.37, lam_g random, three draws per scenario): a one-ulp change of every entry of w and p
moves SSEval's W v by at most 3.3e-15 of the scale on six cases, J v by at most 1.8e-15 and
Z v by at most 5.4e-16, so 1e-10 leaves more than four orders of magnitude for a different
operation order.  On `n1` W v moves by up to 7.1e-13 of the scale: there W is the single entry
sum_o lam_o Hg_o of the last stage seen through B_0, the sum of ten curvature terms of random
sign, and the cancellation is inside that entry, so |W| |v| cannot see it; the margin is 140x
(the GPU measured 1.1e-13 there, at most 5e-16 elsewhere).  The bound is still 1,000x below a
1e-7 error: tests/test_products_capi.py shows on the oracle alone which wrong Hessians it
catches (a dropped term: by 1e7 to 1e10; one stage-cost Hessian entry off by 1e-7 relative: by
58x to 1,000x through the identity directions, 0.3x to 22x through three random ones)."""
from __future__ import annotations

import functools

import numpy as np

from tests import eval_ref as er

TOL = er.TOL
NV = 3
# (obj_factor, lam_g given) of the parity test
COMBOS = ((1.0, True), (0.37, True), (0.0, True), (1.0, False))


def draw_directions(spec, nv, B, seed):
    """(B, nv, nw): N(0, 1) scaled by the bound width of each decision variable."""
    rng = np.random.default_rng(seed)
    lbx, ubx = spec.bounds()[:2]
    width = np.where(np.isfinite(ubx - lbx), ubx - lbx, 10.0)
    return rng.standard_normal((B, nv, spec.nw)) * np.maximum(1e-3, 0.1 * width)


def stack_Z(ev):
    """SSEval.Z (N+1, nx, nw) as the (nX, nw) matrix dX/dw in X's stage-major layout."""
    return ev.Z.reshape(-1, ev.Z.shape[2])


def products_of(J, W, Z, V):
    """V (nv, nw) -> jv, hv, dX as (nv, n) and the per-direction scales (nv,) of each."""
    aV = np.abs(V)
    out = {"jv": V @ J.T, "hv": V @ W.T, "dX": V @ Z.T}
    out["scale"] = {"jv": np.max(aV @ np.abs(J).T, axis=1), "hv": np.max(aV @ np.abs(W).T, axis=1),
                    "dX": np.max(aV @ np.abs(Z).T, axis=1)}
    return out


def cpu_products(ev, V, obj_factor, lam_g):
    """One scenario on the oracle: SSEval `ev`, directions V (nv, nw); lam_g None = zeros."""
    lg = np.zeros(ev.prob.ng) if lam_g is None else lam_g
    return products_of(ev.J, ev.hessian(obj_factor, lg), stack_Z(ev), V)


@functools.lru_cache(maxsize=None)
def evals(name, seed=2024):
    """(spec, eval_ref's inputs, per-scenario SSEval) of a case, computed once and shared."""
    from oracle import nmpc_oracle as orc

    spec, d, _ = er.reference(name, seed)
    prob = er.problem_of(spec)
    return spec, d, [orc.SSEval(prob, d["w"][b], d["p"][b]) for b in range(er.CASES[name])]


@functools.lru_cache(maxsize=None)
def reference(name, seed=2024):
    """(spec, inputs incl. directions "v" (B, NV, nw), {combo: [per-scenario products]})."""
    spec, d, evs = evals(name, seed)
    d = dict(d, v=draw_directions(spec, NV, er.CASES[name], seed + 7))
    ref = {c: [cpu_products(ev, d["v"][b], c[0], d["lam_g"][b] if c[1] else None) for b, ev in enumerate(evs)]
           for c in COMBOS}
    return spec, d, ref


def figures(got, ref):
    """Largest error of each product over its bound TOL * scale (per direction); where the
    scale is exactly 0 (no term exists) the result must be exactly 0."""
    fig = {}
    for k in ("jv", "hv", "dX"):
        if got.get(k) is None:
            continue
        a, r, s = np.asarray(got[k], float), ref[k], ref["scale"][k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err = np.max(np.abs(a - r), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(s > 0, err / (TOL * s), np.where(err == 0, 0.0, np.inf))
        fig[k] = float(np.max(np.where(np.isnan(err), np.inf, q)))
    return fig


def check_against(got, ref, what=""):
    """got: one scenario's jv, hv, dX as (nv, n).  Prints every figure before asserting."""
    fig = figures(got, ref)
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return fig


# ---- mutants of the reference: what an error in one part of the kernel's Hessian looks like
MUTANTS = ("dyn_hess", "Hg", "Hxu", "Hl")


def mutant_products(ev, V, obj_factor, lam_g, which):
    """cpu_products with one part of the oracle's Hessian wrong:
      dyn_hess: the dynamics' second derivatives dropped (Hxx and Hxu parts);
      Hg:       the obstacle rows' curvature dropped;
      Hxu:      the dynamics' state-control cross term dropped;
      Hl:       the largest stage-cost Hessian entry of stages >= 1 off by 1e-7 relative."""
    import copy
    from oracle import nmpc_oracle as orc

    m = copy.copy(ev)
    real = orc.dyn_hess
    try:
        if which == "dyn_hess":
            orc.dyn_hess = lambda *a: tuple(np.zeros_like(t) for t in real(*a))
        elif which == "Hxu":
            orc.dyn_hess = lambda *a: (real(*a)[0], np.zeros_like(real(*a)[1]))
        elif which == "Hg":
            m.Hg = np.zeros_like(ev.Hg)
        elif which == "Hl":
            m.Hl = ev.Hl.copy()
            k, i, j = np.unravel_index(int(np.argmax(np.abs(m.Hl[1:]))), m.Hl[1:].shape)
            m.Hl[k + 1, i, j] *= 1.0 + 1e-7
            if i != j:
                m.Hl[k + 1, j, i] = m.Hl[k + 1, i, j]
        else:
            raise KeyError(which)
        return cpu_products(m, V, obj_factor, lam_g)
    finally:
        orc.dyn_hess = real
