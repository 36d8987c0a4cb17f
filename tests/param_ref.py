"""Checker side of the parameter-product tests (tests/test_gpu_param.py,
tests/test_param_capi.py): the dense dg/dp, d_p grad_w L, dX/dp and grad_p L of the oracle
(oracle.nmpc_oracle.SSEval: A, Z's recursion, Gk, Hg, gl, Hl, dyn_hess, and stage_cost_derivs on
unit-weight copies of the problem), on the cases and points of tests/eval_ref.py, applied to
directions; the scales of the tolerance, the comparison, and mutants of the reference.

With L = sigma F + lam' g, xi_0 = dp[0:nx], xi_{k+1} = A_k xi_k, and a move of the target /
of an obstacle centre acting like the opposite move of (x, y) seen by the stage cost / by that
obstacle's row alone (both read their point only through differences):
  (dg/dp dp)_(k,i)      = G_(k,i) (xi_k - move_i)                                  k = 0 .. N
  h_k                   = sigma Hl_k (xi_k - target move) + sum_o lam_(k,o) Hg_o (xi_k - move_o)
                          + d2_xx(adj_(k+1)' T f) xi_k + sigma (dw1 gl_k^(1,0) + dw2 gl_k^(0,1))
  mu_k                  = h_k + A_k' mu_(k+1)
  (d_p grad_w L dp)_u_k = B_k' mu_(k+1) + Hxu_k' xi_k                              k = 0 .. N - 1
  grad_p L              = adj_0 | -sigma sum_k gl_k[0:2] | -sum_k lam_(k,o) G_(k,o)[0:2]
                          | sigma sum_k l_k^(1,0), sigma sum_k l_k^(0,1)

Directions: dp ~ N(0, 1) per entry, times 1e-2 max(1, |p_i|) for the x0 entries, 1 for target
and obstacle (and unread) entries, 0.1 for weight entries; nd = 3 per scenario.

Tolerance eval_ref.TOL = 1e-10, relative per direction to the absolute-product scales
max_i (|dg/dp| |dp|)_i, max_i (|d_p grad_w L| |dp|)_i, max_i (|dX/dp| |dp|)_i, and for grad_p L
per entry to the same sum with every term's absolute value (|sigma| sum |cost terms| +
sum |lam| |G|, through |A| for the x0 block).  Where a scale is exactly 0 the result must be
exactly 0.

Basis of the tolerance, measured on the CPU (tests/test_param_capi.py::
test_one_ulp_basis_of_the_tolerance prints it): a one-ulp change of every entry of w and p,
three draws per scenario, sigma 1 and 0.37, lam_g random, moves the checker's products by at most
                   jp       hp       dXp      gp      (of the scale)
  race_track_2   2.5e-15  3.5e-14  2.4e-16  6.6e-14
  nmpc_tt        5.9e-16  7.5e-15  4.8e-16  8.5e-15
  n63_16obs      4.1e-15  2.7e-15  6.2e-16  1.2e-14
  n1             1.2e-15  1.5e-15  6.1e-17  1.9e-14
  dynamic        7.8e-16  6.1e-15  2.5e-16  3.9e-14
  weights_in_p   1.2e-15  1.2e-14  2.5e-16  5.9e-14
  uav5           4.4e-16  2.2e-14  1.5e-16  3.1e-14
so 1e-10 leaves at least 1,500x on every case for a different operation order.  `n1`, whose
w-side Hessian product cancels inside one entry (tests/products_ref.py: margin 140x), is not
special here: its result is dominated by the stage-0 cross term Hxu_0' xi_0, which does not
cancel.
The checker itself agrees with Richardson-extrapolated central differences of SSEval's g,
sigma grad F + J' lam, X and L to at most 1.7e-9 of each array's largest entry (the
differences' own rounding; test_the_checker_matches_differences_of_the_oracle, bound 1e-7)."""
from __future__ import annotations

import dataclasses
import functools

import numpy as np

from tests import eval_ref as er
from tests import products_ref as pr

TOL = er.TOL
ND = 3
COMBOS = pr.COMBOS
KEYS = ("jp", "hp", "dXp")
# a term of the reference that a mutant drops (tests/test_param_capi.py)
MUTANTS = ("cross0", "tshift", "oshift", "wgrad", "dynxx")


def entry_kinds(prob):
    """Per entry of p: 'x0', 'target', 'obstacle', 'weight' or None (nothing reads it)."""
    kinds = [None] * prob.np_
    for i in range(prob.nx):
        kinds[i] = "x0"
    kinds[prob.target_index] = kinds[prob.target_index + 1] = "target"
    for idx in list(prob.obs_x_pidx) + list(prob.obs_y_pidx):
        if idx >= 0:
            kinds[idx] = "obstacle"
    for idx in (prob.w1_pidx, prob.w2_pidx):
        if idx >= 0:
            kinds[idx] = "weight"
    return kinds


def draw_directions(prob, P, nd, seed):
    """(B, nd, np) for the points P (B, np)."""
    rng = np.random.default_rng(seed)
    kinds = entry_kinds(prob)
    B = P.shape[0]
    sc = np.ones((B, prob.np_))
    for i, kd in enumerate(kinds):
        if kd == "x0":
            sc[:, i] = 1e-2 * np.maximum(1.0, np.abs(P[:, i]))
        elif kd == "weight":
            sc[:, i] = 0.1
    return rng.standard_normal((B, nd, prob.np_)) * sc[:, None, :]


def dense(ev, obj_factor, lam_g, drop=None):
    """One scenario on the oracle: SSEval `ev`; lam_g None = zeros.  Returns Jp (ng, np),
    C = d_p grad_w L (nw, np), Xp (nX, np), gp (np,) and gp's absolute scale (np,).
    drop: one of MUTANTS, that term left out."""
    from oracle import nmpc_oracle as orc

    prob = ev.prob
    N, m, nx, nu, nb, nobs, npp = prob.N, prob.m, prob.nx, prob.nu, prob.nb, prob.n_obs, prob.np_
    sig = float(obj_factor)
    lam = (np.zeros(prob.ng) if lam_g is None else np.asarray(lam_g, float)).reshape(N + 1, m)
    ti = prob.target_index
    xt, yt = ev.p[ti], ev.p[ti + 1]
    # moves: (nx, np) selectors of the entries of p that move the target / obstacle o
    Tm = np.zeros((nx, npp))
    if drop != "tshift":
        Tm[0, ti] = Tm[1, ti + 1] = 1.0
    Om = np.zeros((nobs, nx, npp))
    for o in range(nobs):
        if drop == "oshift":
            break
        if prob.obs_x_pidx[o] >= 0:
            Om[o, 0, prob.obs_x_pidx[o]] = 1.0
        if prob.obs_y_pidx[o] >= 0:
            Om[o, 1, prob.obs_y_pidx[o]] = 1.0
    # state tangent
    Xi = np.zeros((N + 1, nx, npp))
    Xi[0][:, :nx] = np.eye(nx)
    for k in range(N):
        Xi[k + 1] = ev.A[k] @ Xi[k]
    # rows
    Jp = np.zeros((N + 1, m, npp))
    for k in range(N + 1):
        Jp[k, :nb] = ev.Gk[k, :nb] @ Xi[k]
        for o in range(nobs):
            Jp[k, nb + o] = ev.Gk[k, nb + o] @ (Xi[k] - Om[o])
    # Lagrangian adjoint, stage 0 included, and its absolute version
    adj, aadj = np.zeros((N + 2, nx)), np.zeros((N + 2, nx))
    for k in range(N, -1, -1):
        adj[k] = sig * ev.gl[k] + ev.Gk[k].T @ lam[k]
        aadj[k] = abs(sig) * np.abs(ev.gl[k]) + np.abs(ev.Gk[k]).T @ np.abs(lam[k])
        if k < N:
            adj[k] += ev.A[k].T @ adj[k + 1]
            aadj[k] += np.abs(ev.A[k]).T @ aadj[k + 1]
    # unit-weight stage costs and gradients
    unit = {}
    for key, idx, (u1, u2) in (("w1", prob.w1_pidx, (1.0, 0.0)), ("w2", prob.w2_pidx, (0.0, 1.0))):
        if idx < 0:
            continue
        pu = dataclasses.replace(prob, w1=u1, w2=u2)
        vals, grads = np.zeros(N), np.zeros((N, nx))
        for k in range(N):
            vals[k], grads[k], _ = orc.stage_cost_derivs(pu, ev.X[:, k], xt, yt)
        unit[idx] = (vals, grads)
    # adjoint source tangent, adjoint tangent, result
    H = np.zeros((N + 1, nx, npp))
    Hxu = np.zeros((N, nx, nu))
    for k in range(N + 1):
        if k < N:
            H[k] += sig * ev.Hl[k] @ (Xi[k] - Tm)
            dHxx, Hxu[k] = orc.dyn_hess(prob, ev.X[:, k], ev.U[:, k], adj[k + 1])
            if drop != "dynxx":
                H[k] += dHxx @ Xi[k]
            if drop != "wgrad":
                for idx, (_, grads) in unit.items():
                    H[k][:, idx] += sig * grads[k]
        for o in range(nobs):
            Hg8 = np.zeros((nx, nx))
            Hg8[0:2, 0:2] = ev.Hg[k, o]
            H[k] += lam[k, nb + o] * (Hg8 @ (Xi[k] - Om[o]))
    M = np.zeros((N + 2, nx, npp))
    for k in range(N, -1, -1):
        M[k] = H[k] + (ev.A[k].T @ M[k + 1] if k < N else 0.0)
    Cm = np.zeros((N, nu, npp))
    for k in range(N):
        Cm[k] = ev.B[k].T @ M[k + 1]
        if not (drop == "cross0" and k == 0):
            Cm[k] += Hxu[k].T @ Xi[k]
    # gradient
    gp, gs = np.zeros(npp), np.zeros(npp)
    gp[:nx], gs[:nx] = adj[0], aadj[0]
    if N > 0:
        gp[ti:ti + 2] = -sig * np.sum(ev.gl[:N, 0:2], axis=0)
        gs[ti:ti + 2] = abs(sig) * np.sum(np.abs(ev.gl[:N, 0:2]), axis=0)
    for o in range(nobs):
        for c, idx in ((0, prob.obs_x_pidx[o]), (1, prob.obs_y_pidx[o])):
            if idx >= 0:
                gp[idx] += -np.sum(lam[:, nb + o] * ev.Gk[:, nb + o, c])
                gs[idx] += np.sum(np.abs(lam[:, nb + o] * ev.Gk[:, nb + o, c]))
    for idx, (vals, _) in unit.items():
        gp[idx] += sig * np.sum(vals)
        gs[idx] += abs(sig) * np.sum(np.abs(vals))
    return {"Jp": Jp.reshape(-1, npp), "C": Cm.reshape(-1, npp), "Xp": Xi.reshape(-1, npp), "gp": gp,
            "gp_scale": gs}


def products_of(dn, D):
    """D (nd, np) -> jp, hp, dXp as (nd, n), gp, and the scales: (nd,) per product, (np,) for gp."""
    aD = np.abs(D)
    out = {"jp": D @ dn["Jp"].T, "hp": D @ dn["C"].T, "dXp": D @ dn["Xp"].T, "gp": dn["gp"]}
    out["scale"] = {"jp": np.max(aD @ np.abs(dn["Jp"]).T, axis=1), "hp": np.max(aD @ np.abs(dn["C"]).T, axis=1),
                    "dXp": np.max(aD @ np.abs(dn["Xp"]).T, axis=1), "gp": dn["gp_scale"]}
    return out


def cpu_products(ev, D, obj_factor, lam_g, drop=None):
    return products_of(dense(ev, obj_factor, lam_g, drop), D)


@functools.lru_cache(maxsize=None)
def reference(name, seed=2024):
    """(spec, inputs incl. directions "dp" (B, ND, np), {combo: [per-scenario products]})."""
    spec, d, evs = pr.evals(name, seed)
    prob = er.problem_of(spec)
    d = dict(d, dp=draw_directions(prob, d["p"], ND, seed + 11))
    ref = {c: [cpu_products(ev, d["dp"][b], c[0], d["lam_g"][b] if c[1] else None) for b, ev in enumerate(evs)]
           for c in COMBOS}
    return spec, d, ref


def figures(got, ref):
    """Largest error of each product over its bound TOL * scale (per direction; gp per entry);
    where the scale is exactly 0 (no term exists) the result must be exactly 0."""
    fig = {}
    for k in KEYS + ("gp",):
        if got.get(k) is None:
            continue
        a, r, s = np.asarray(got[k], float), ref[k], ref["scale"][k]
        assert a.shape == r.shape, (k, a.shape, r.shape)
        err = np.abs(a - r) if k == "gp" else np.max(np.abs(a - r), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(s > 0, err / (TOL * s), np.where(err == 0, 0.0, np.inf))
        fig[k] = float(np.max(np.where(np.isnan(err), np.inf, q)))
    return fig


def check_against(got, ref, what=""):
    """got: one scenario's jp, hp, dXp as (nd, n) and gp (np,).  Prints every figure before asserting."""
    fig = figures(got, ref)
    print(f"{what}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, (what, bad)
    return fig


# ---- Richardson-extrapolated central differences of the oracle's own function layer
def richardson(prob, w, p, obj_factor, lam_g, h=1e-4):
    """Jp, C, Xp, gp by differences of SSEval's g, sigma grad F + J' lam, X and L at the
    relative steps h and 2h: (4 D(h) - D(2h)) / 3."""
    from oracle import nmpc_oracle as orc

    def layer(pp):
        ev = orc.SSEval(prob, w, pp)
        return (ev.g, obj_factor * ev.gradF + ev.J.T @ lam_g, ev.X.T.reshape(-1),
                np.array([obj_factor * ev.F + lam_g @ ev.g]))

    cols = [[], [], [], []]
    for i in range(len(p)):
        step = h * max(1.0, abs(p[i]))
        D = []
        for s in (step, 2 * step):
            pp, pm = p.copy(), p.copy()
            pp[i] += s
            pm[i] -= s
            D.append([(a - c) / (2 * s) for a, c in zip(layer(pp), layer(pm))])
        for j in range(4):
            cols[j].append((4 * D[0][j] - D[1][j]) / 3)
    Jp, Cm, Xp, gp = (np.stack(c, axis=1) for c in cols)
    return {"Jp": Jp, "C": Cm, "Xp": Xp, "gp": gp[0]}
