"""Checker side of the policy-value tests (tests/test_gpu_value.py, tests/test_value_capi.py), on the
oracle alone: the cost-to-go expansion of the unclamped feedback policy along the plan, one scenario at
a time, with oracle.nmpc_oracle's stage_cost_derivs, dyn_jac and dyn_hess,

    lam_N = 0, P_N = 0
    k = N-1 ... 0:  g_k, H_k = stage_cost_derivs at Xbar_k
                    A_k, B_k = dyn_jac at (Xbar_k, ubar_k);  Acl_k = A_k + B_k K_k     (K None: A_k)
                    Fxx, Fxu = dyn_hess at (Xbar_k, ubar_k, lam_{k+1})
                    M_k   = H_k + Fxx + Fxu K_k + K_k' Fxu'
                    lam_k = g_k + Acl_k' lam_{k+1}
                    P_k   = M_k + Acl_k' P_{k+1} Acl_k
    J = sum_k l_k(Xbar_k)
    dJ   = 1/2 <P_0, S0> + 1/2 sum_{k>=1} <P_k, W>,   varJ = lam_0' S0 lam_0 + sum_{k>=1} lam_k' W lam_k

with S0 and W the mirrors of their lower triangles.  For the tolerances of the GPU test, one step's
magnitudes at the checker's own P_{k+1} and lam_{k+1}:
    aP[k] = max entry of |M_k| + |Acl_k|' |P_{k+1}| |Acl_k|   (|M_k| the sum of its terms' magnitudes)
    aL[k] = max entry of |g_k| + |Acl_k|' |lam_{k+1}|
    sl[k] = |l_k|
`order` picks the association of the triple product (0: Acl' (P Acl), 1: (Acl' P) Acl).

Mutants, for the teeth of the CPU gate (tests/test_value_capi.py):
  "nodyn":     Fxx and Fxu dropped (the cost's curvature alone)
  "nocross":   the Fxu K terms dropped
  "shift", "transpose": tests/rollout_ref._mutate_K"""
from __future__ import annotations

import numpy as np

from tests import rollout_ref as rr
from tests.covariance_ref import mirror

MUTANTS = ("nodyn", "nocross", "shift", "transpose")


def value_one(prob, p, ubar, Xbar, K, mutant=None, order=0):
    """One scenario.  ubar (N, nu), Xbar (N + 1, nx), K (N, nu, nx) or None.  Returns J, l (N,), lam
    (N + 1, nx), P (N + 1, nx, nx) and the scales aP (N,), aL (N,)."""
    from oracle import nmpc_oracle as orc

    N, nx, nu = prob.N, prob.nx, prob.nu
    p = np.asarray(p, float)
    pw = prob.weighted(p)
    ti = prob.target_index
    K = rr._mutate_K(K, mutant)
    lam, P = np.zeros((N + 1, nx)), np.zeros((N + 1, nx, nx))
    l, aP, aL = np.zeros(N), np.zeros(N), np.zeros(N)
    for k in range(N - 1, -1, -1):
        try:
            l[k], g, H = orc.stage_cost_derivs(pw, Xbar[k], p[ti], p[ti + 1])
            A, Bm = orc.dyn_jac(prob, Xbar[k], ubar[k])
            Fxx, Fxu = orc.dyn_hess(prob, Xbar[k], ubar[k], lam[k + 1])
        except (ValueError, OverflowError, ZeroDivisionError):  # math.* on inf / nan
            l[k], g, H = np.nan, np.full(nx, np.nan), np.full((nx, nx), np.nan)
            A, Bm = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan)
            Fxx, Fxu = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan)
        if mutant == "nodyn":
            Fxx, Fxu = np.zeros_like(Fxx), np.zeros_like(Fxu)
        with np.errstate(invalid="ignore", over="ignore"):
            Acl = A if K is None else A + Bm @ K[k]
            M, Ma = H + Fxx, np.abs(H) + np.abs(Fxx)
            if K is not None and mutant != "nocross":
                C = Fxu @ K[k]
                M = M + C + C.T
                Ca = np.abs(Fxu) @ np.abs(K[k])
                Ma = Ma + Ca + Ca.T
            lam[k] = g + Acl.T @ lam[k + 1]
            P[k] = M + (Acl.T @ (P[k + 1] @ Acl) if order == 0 else (Acl.T @ P[k + 1]) @ Acl)
            aL[k] = float(np.max(np.abs(g) + np.abs(Acl).T @ np.abs(lam[k + 1])))
            aP[k] = float(np.max(Ma + np.abs(Acl).T @ np.abs(P[k + 1]) @ np.abs(Acl)))
    return {"J": float(np.sum(l)), "l": l, "lam": lam, "P": P, "aP": aP, "aL": aL}


def inner(P, S):
    """<P, S> over the lower triangle of S: sum_i P_ii S_ii + 2 sum_{i>j} P_ij S_ij."""
    return float(np.sum(P * mirror(np.asarray(S, float))))


def moments(ref, S0, W=None):
    """dJ and varJ of one case from value_one's lam and P, and their scales
    A = 1/2 (<|P_0|, |S0|> + sum <|P_k|, |W|>) and V = |lam_0|' |S0| |lam_0| + sum |lam_k|' |W| |lam_k|."""
    lam, P = ref["lam"], ref["P"]
    S = mirror(np.asarray(S0, float))
    with np.errstate(invalid="ignore"):
        dJ, var = 0.5 * float(np.sum(P[0] * S)), float(lam[0] @ S @ lam[0])
        A, V = 0.5 * float(np.sum(np.abs(P[0]) * np.abs(S))), float(np.abs(lam[0]) @ np.abs(S) @ np.abs(lam[0]))
        if W is not None:
            Wm = mirror(np.asarray(W, float))
            for k in range(1, len(lam)):
                dJ += 0.5 * float(np.sum(P[k] * Wm))
                var += float(lam[k] @ Wm @ lam[k])
                A += 0.5 * float(np.sum(np.abs(P[k]) * np.abs(Wm)))
                V += float(np.abs(lam[k]) @ np.abs(Wm) @ np.abs(lam[k]))
    return {"dJ": dJ, "varJ": var, "A": A, "V": V}


def pair_scales(ref, S0, W, N):
    """The gates' scales over the sigma-point pairs (tests/covariance_ref.sigma_points): A = sum over
    the pairs of |1/2 d' P_j d| and V = sum of (lam_j . d)^2, with j the pair's stage of entry, and the
    number of pairs."""
    from tests.covariance_ref import sigma_points

    pts = sigma_points(mirror(np.asarray(S0, float)), None if W is None else mirror(np.asarray(W, float)), N)
    A = sum(abs(0.5 * float(d @ ref["P"][j] @ d)) for j, d in pts)
    V = sum(float(ref["lam"][j] @ d) ** 2 for j, d in pts)
    return A, V, len(pts)


def value_batch(prob, P, ubar, Xbar, K, S0=None, W=None, **kw):
    """Every scenario and case: P (B, np), ubar (B, nw), Xbar (B, N + 1, nx), K (B, N, nu, nx) or None,
    S0 and W (B, nc, nx, nx) or None.  Returns J (B,), l (B, N), lam, P, aP, aL and, with S0, dJ, varJ,
    A, V (B, nc)."""
    N, nu = prob.N, prob.nu
    B = len(Xbar)
    refs = [value_one(prob, P[b], np.asarray(ubar[b], float).reshape(N, nu), Xbar[b], None if K is None else K[b], **kw)
            for b in range(B)]
    out = {k: np.stack([np.asarray(r[k]) for r in refs]) for k in refs[0]}
    if S0 is not None:
        nc = S0.shape[1]
        for k in ("dJ", "varJ", "A", "V"):
            out[k] = np.zeros((B, nc))
        for b in range(B):
            for c in range(nc):
                m = moments(refs[b], S0[b, c], None if W is None else W[b, c])
                for k in m:
                    out[k][b, c] = m[k]
    return out
