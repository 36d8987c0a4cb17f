"""Checker side of the fused forward-mode sensitivity tests (tests/test_gpu_solve_tangent.py,
tests/test_solve_tangent_capi.py), on the oracle alone: the dense forward-mode sensitivity of a
solution,

    hp = C dp,   jp = Jp dp,   dXp = Xp dp
    M dx = -hp - J' Sigma_s jp                       (free variables; 0 on fixed ones)
    dlam_g = Sigma_s (J dx + jp),   dX = Z dx + dXp

with J, W, Z, Jp, C, Xp of tests/adjoint_ref.dense (tests/param_ref.dense's parameter matrices),
M of tests/kkt_ref.dense_M, the weights of tests/kkt_ref.barrier_weights and the delta of
tests/solve_adjoint_ref.ladder_delta -- the formula of Solver.sensitivity(tangent="exact") with
dense matrices and numpy.linalg.solve in place of every kernel, and the state trajectory's
tangent beside it.  dlam_g and dX come with the scales of gate (b): the per-entry sums of the
absolute terms, Sigma_s (|J| |dx| + |Jp| |dp|) and |Z| |dx| + |Xp| |dp|.

Solved cases: tests/solve_adjoint_ref.SOLVED.

Mutants, for the teeth of the gate: one term of the formula wrong,
  "norhsjp": rhs = -hp                      (J' Sigma_s jp dropped from the right-hand side)
  "nojp":    dlam_g = Sigma_s J dx          (jp dropped from the row step)
  "noXp":    dX = Z dx                      (the parameters' own state tangent dropped)
  "hpsign":  rhs = +hp - J' Sigma_s jp
  "nofloor": Sigma_s without the bound_relax_factor floor under an active row's slack
             (tests/solve_adjoint_ref.weights_nofloor): the formula itself wherever no active
             row's slack lies below the floor."""
from __future__ import annotations

import numpy as np

from tests import adjoint_ref as ar
from tests import kkt_ref as kr
from tests import solve_adjoint_ref as sr

TOL = ar.TOL
ND = 2
MUTANTS = ("norhsjp", "nojp", "noXp", "hpsign", "nofloor")
SOLVED = sr.SOLVED
KEYS = ("dlam_g", "dX")


def draw_directions(spec, B, nd, seed):
    """dp (B, nd, np): N(0, 1) per entry."""
    return np.random.default_rng(seed).standard_normal((B, nd, spec.np))


def products_on(ref, dx, dp, mutant=None):
    """dlam_g (nd, ng), dX (nd, nX) of the dense matrices on a given dx (nd, nw), with the
    per-entry sums of the absolute terms that scale gate (b)."""
    dn, ss = ref["dn"], ref["ss"]
    J, Z, Jp, Xp = dn["J"], dn["Z"], dn["Jp"], dn["Xp"]
    jp, dXp = dp @ Jp.T, dp @ Xp.T
    with np.errstate(invalid="ignore"):
        dlam = ss * (dx @ J.T) if mutant == "nojp" else ss * (dx @ J.T + jp)
        dX = dx @ Z.T if mutant == "noXp" else dx @ Z.T + dXp
        scale = {"dlam_g": ss * (np.abs(dx) @ np.abs(J).T + np.abs(dp) @ np.abs(Jp).T),
                 "dX": np.abs(dx) @ np.abs(Z).T + np.abs(dp) @ np.abs(Xp).T}
    return {"dlam_g": dlam, "dX": dX, "scale": scale}


def dense_tangent(prob, x, lam_g, lam_x, p, bounds, dp, delta=None, mutant=None, g=None, brf=1e-8):
    """One scenario; dp (nd, np); delta None = ladder_delta's.  Returns dx (nd, nw), dlam_g
    (nd, ng), dX (nd, nX), their scales, hp, jp, the reduced M, its right-hand sides and their
    scale, the free set, Sigma_s and the delta used."""
    from oracle import nmpc_oracle as orc

    lbx, ubx, lbg, ubg = bounds
    ev = orc.SSEval(prob, x, p)
    dn = ar.dense(ev, 1.0, lam_g)
    J = dn["J"]
    gv = ev.g if g is None else g
    sx = kr.barrier_weights(x, lam_x, lbx, ubx, brf)
    ss = sr.weights_nofloor(gv, lam_g, lbg, ubg) if mutant == "nofloor" else kr.barrier_weights(gv, lam_g, lbg, ubg, brf)
    assert not np.any(np.isinf(ss)), "equality rows are not supported"
    free = np.isfinite(sx)
    with np.errstate(invalid="ignore"):
        def M_of(dl):
            return kr.dense_M(ev, dn["W"], np.where(free, sx, 0.0), ss, dl)[np.ix_(free, free)]

        if delta is None:
            delta = sr.ladder_delta(M_of) if np.all(np.isfinite(ss)) else 0.0
            assert delta is not None, "no rung of the ladder factorises"
        Mf = M_of(delta)
        hp, jp = dp @ dn["C"].T, dp @ dn["Jp"].T
        r = (hp if mutant == "hpsign" else -hp)
        if mutant != "norhsjp":
            r = r - (ss * jp) @ J
        rs = np.abs(dp) @ np.abs(dn["C"]).T + (ss * (np.abs(dp) @ np.abs(dn["Jp"]).T)) @ np.abs(J)
        dx = np.zeros((dp.shape[0], prob.nw))
        dx[:, free] = np.linalg.solve(Mf, r[:, free].T).T if np.all(np.isfinite(Mf)) else np.nan
    ref = {"dx": dx, "hp": hp, "jp": jp, "M": Mf, "rhs": r[:, free], "rhs_scale": rs[:, free], "free": free, "ss": ss,
           "dn": dn, "ev": ev, "delta": delta}
    ref.update(products_on(ref, dx, dp, mutant))
    return ref


def tangent_of(name, b, dp, mutant=None, delta=None):
    """The checker at scenario b of a solved case (tests/solve_adjoint_ref.solved); dp (B, nd, np)."""
    spec, prob, P, bounds, sols = sr.solved(name)
    s = sols[b]
    return dense_tangent(prob, s["x"], s["lam_g"], s["lam_x"], P[b], bounds, dp[b], mutant=mutant, delta=delta)


def figures(got, ref):
    """Gate (b): the largest error of dlam_g and of dX over TOL x the sum of the absolute terms,
    per entry; where the sum is exactly 0 (no term exists) the result must be exactly 0."""
    fig = {}
    for k in KEYS:
        if got.get(k) is None:
            continue
        a, r, s = np.asarray(got[k], float), ref[k], ref["scale"][k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err = np.abs(a - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(s > 0, err / (TOL * s), np.where(err == 0, 0.0, np.inf))
        fig[k] = float(np.max(np.where(np.isnan(err), np.inf, q)))
    return fig


def check_against(got, ref, what="", factor=1.0):
    """got: one scenario's dlam_g (nd, ng) and / or dX (nd, nX).  Prints every figure before asserting."""
    fig = figures(got, ref)
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= factor}
    assert not bad, (what, bad)
    return fig
