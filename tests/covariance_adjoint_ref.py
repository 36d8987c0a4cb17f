"""Checker side of the policy-covariance adjoint tests (tests/test_gpu_policy_covariance_adjoint.py,
tests/test_covariance_adjoint_capi.py), on the oracle alone: the reverse sweep of
tests/covariance_ref.covariance_one, one (scenario, case) at a time, with oracle.nmpc_oracle's dyn_jac,
dyn_hess and obstacle_derivs.  For seeds Sb (N + 1, nx, nx) on Sigma, ub (N, nu) on var_u and gb
(N + 1, m) on var_g, the gradient of

    L = sum_k <Sb_k, Sigma_k> + <ub, var_u> + <gb, var_g>

at the forward's own Sigma_k (an input), with sym(S) = (S + S') / 2:

    R_k(Lam): Lam[bi, bi] += gb[k, i]                            box row i on state bi
              Lam[0:2, 0:2] += gb[k, o] g g'                     obstacle row o
              obs_var_bar[o] += gb[k, o]
              pos = H_o (2 gb[k, o] Sigma_k[0:2, 0:2] g)         H_o = obstacle_derivs()[1]
              Xbar_bar[k, 0:2] += pos;  p_bar[obs_x_pidx[o]] -= pos[0], p_bar[obs_y_pidx[o]] -= pos[1]
    Lam_N = sym(Sb_N) + R_N
    k = N-1 ... 0:  W_bar += Lam_{k+1}
                    M = Lam_{k+1} Acl_k,  G = 2 M Sigma_k
                    K_bar_k = B_k' G + 2 diag(ub_k) K_k Sigma_k
                    A_bar = G,  B_bar = G K_k'
                    for i = 0, 1, 2 and (Hxx, Hxu) = dyn_hess(prob, Xbar_k, ubar_k, e_i):
                        Xbar_bar_k += Hxx A_bar[i, :] + Hxu B_bar[i, :];  ubar_bar_k += Hxu' A_bar[i, :]
                    Lam_k = Acl_k' M + sym(Sb_k) + K_k' diag(ub_k) K_k + R_k
    S0_bar = Lam_0

`order` picks the association of the triple products (0: Acl' (Lam Acl) and 2 (Lam Acl) Sigma, 1:
(Acl' Lam) Acl and 2 Lam (Acl Sigma)) and `dtype` the arithmetic (np.float64 or np.longdouble), as
covariance_ref has them; Acl_k is formed in fp64 in both.  The result also holds, for the tolerances of the
GPU test, the absolute-value version of every formula at the checker's own Lam_{k+1}:
    aL[k]  = max entry of |Acl_k|' |Lam_{k+1}| |Acl_k| + |sym Sb_k| + |K_k|' |ub_k| |K_k| + |R_k|
    aK[k], aU[k], aX[k], aW, aO, aP: K_bar_k's, ubar_bar_k's, Xbar_bar_k's formula and the stage sums of
    W_bar, obs_var_bar and p_bar with every factor replaced by its absolute value.

Mutants, for the teeth of the CPU gate (tests/test_covariance_adjoint_capi.py):
  "transpose": G = 2 Sigma_k M
  "shift":     K_{k+1} in K_k's place
  "noW":       W_bar leaves out Lam_N
  "half":      the factor 2 of G dropped
  "rows":      the obstacle rows' curvature term H g_bar dropped"""
from __future__ import annotations

import numpy as np

from tests import covariance_ref as cr

MUTANTS = ("transpose", "shift", "noW", "half", "rows")


def sym(S):
    return 0.5 * (S + np.swapaxes(S, -1, -2))


def adjoint_one(prob, p, ubar, Xbar, K, Sigma, Sb=None, ub=None, gb=None, mutant=None, order=0, dtype=np.float64):
    """One (scenario, case).  ubar (N, nu), Xbar (N + 1, nx), K (N, nu, nx) or None, Sigma (N + 1, nx, nx)
    the forward's (its lower triangles are read), the seeds or None.  Returns S0_bar, W_bar (nx, nx),
    Lambda (N + 1, nx, nx), obs_var_bar (n_obs,), K_bar (N, nu, nx) (None without K), ubar_bar (N, nu),
    Xbar_bar (N + 1, nx), p_bar (np,) and the scales aL (N + 1,), aK, aU, aX, aW, aO, aP shaped like the
    outputs they belong to."""
    from oracle import nmpc_oracle as orc

    N, nx, nu, m, nb, nobs = prob.N, prob.nx, prob.nu, prob.m, prob.nb, prob.n_obs
    p = np.asarray(p, float)
    ox, oy = prob.obstacles(p)
    if mutant == "shift" and K is not None:
        K = np.concatenate([K[1:], K[-1:]], axis=0)
    Sig = np.stack([cr.mirror(np.asarray(S, float)) for S in Sigma]).astype(dtype)
    zero = lambda *s: np.zeros(s, dtype=dtype)  # noqa: E731
    Sb = zero(N + 1, nx, nx) if Sb is None else np.asarray(Sb, float).astype(dtype)
    ub = zero(N, nu) if (ub is None or K is None) else np.asarray(ub, float).astype(dtype)
    gb = zero(N + 1, m) if gb is None else np.asarray(gb, float).astype(dtype)
    Lam, aL = zero(N + 1, nx, nx), np.zeros(N + 1)
    W_bar, aW = zero(nx, nx), np.zeros((nx, nx))
    ov_bar, aO = zero(nobs), np.zeros(nobs)
    K_bar, aK = (None, None) if K is None else (zero(N, nu, nx), np.zeros((N, nu, nx)))
    u_bar, aU = zero(N, nu), np.zeros((N, nu))
    X_bar, aX = zero(N + 1, nx), np.zeros((N + 1, nx))
    p_bar, aP = zero(len(p)), np.zeros(len(p))

    def rows(k):
        """R_k and its absolute version; adds the rows' terms of stage k to the other outputs."""
        R, Ra = zero(nx, nx), np.zeros((nx, nx))
        for i, bi in enumerate(prob.box_states):
            R[bi, bi] += gb[k, i]
            Ra[bi, bi] += abs(gb[k, i])
        if nobs:
            with np.errstate(invalid="ignore", divide="ignore"):
                G, H = orc.obstacle_derivs(Xbar[k], ox, oy)
            G, H = G.astype(dtype), H.astype(dtype)
            S2 = Sig[k][:2, :2]
            for o in range(nobs):
                w = gb[k, nb + o]
                R[:2, :2] += w * np.outer(G[o], G[o])
                Ra[:2, :2] += abs(w) * np.outer(np.abs(G[o]), np.abs(G[o]))
                ov_bar[o] += w
                aO[o] += abs(w)
                if mutant == "rows":
                    continue
                pos = H[o] @ (2.0 * w * (S2 @ G[o]))
                pa = np.abs(H[o]) @ (2.0 * abs(w) * (np.abs(S2) @ np.abs(G[o])))
                X_bar[k, :2] += pos
                aX[k, :2] += np.asarray(pa, float)
                for c, idx in enumerate((prob.obs_x_pidx[o], prob.obs_y_pidx[o])):
                    if idx >= 0:
                        p_bar[idx] -= pos[c]
                        aP[idx] += float(pa[c])
        return R, Ra

    R, Ra = rows(N)
    Lam[N] = sym(Sb[N]) + R
    aL[N] = float(np.max(np.abs(sym(Sb[N])) + Ra))
    for k in range(N - 1, -1, -1):
        try:
            A, Bm = orc.dyn_jac(prob, Xbar[k], ubar[k])
        except (ValueError, OverflowError):  # math.* on inf / nan
            A, Bm = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan)
        Acl = A
        Kk = zero(nu, nx)
        if K is not None:
            Kk = K[k].astype(dtype)
            with np.errstate(invalid="ignore"):
                Acl = A + Bm @ K[k]  # fp64 whatever `dtype`, as covariance_ref forms it
        Acl, Bm = Acl.astype(dtype), Bm.astype(dtype)
        L1, S = Lam[k + 1], Sig[k]
        if not (mutant == "noW" and k == N - 1):
            W_bar = W_bar + L1
        aW += np.abs(np.asarray(L1, float))
        with np.errstate(invalid="ignore", over="ignore"):
            M = L1 @ Acl
            if mutant == "transpose":
                G = 2.0 * (S @ M)
            elif order == 0:
                G = 2.0 * (M @ S)
            else:
                G = 2.0 * (L1 @ (Acl @ S))
            if mutant == "half":
                G = 0.5 * G
            Ga = 2.0 * (np.abs(L1) @ np.abs(Acl) @ np.abs(S))
            if K is not None:
                K_bar[k] = Bm.T @ G + 2.0 * ub[k][:, None] * (Kk @ S)
                aK[k] = np.abs(Bm).T @ Ga + 2.0 * np.abs(ub[k])[:, None] * (np.abs(Kk) @ np.abs(S))
            A_bar, B_bar = G, G @ Kk.T
            Aa, Ba = Ga, Ga @ np.abs(Kk).T
            for i in range(3):
                e = np.zeros(nx)
                e[i] = 1.0
                try:
                    Hxx, Hxu = orc.dyn_hess(prob, Xbar[k], ubar[k], e)
                except (ValueError, OverflowError):
                    Hxx, Hxu = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan)
                Hxx, Hxu = Hxx.astype(dtype), Hxu.astype(dtype)
                X_bar[k] += Hxx @ A_bar[i] + Hxu @ B_bar[i]
                u_bar[k] += Hxu.T @ A_bar[i]
                aX[k] += np.asarray(np.abs(Hxx) @ Aa[i] + np.abs(Hxu) @ Ba[i], float)
                aU[k] += np.asarray(np.abs(Hxu).T @ Aa[i], float)
            R, Ra = rows(k)
            AtLA = Acl.T @ M if order == 0 else (Acl.T @ L1) @ Acl
            Lam[k] = AtLA + sym(Sb[k]) + Kk.T @ (ub[k][:, None] * Kk) + R
            aL[k] = float(np.max(np.abs(Acl).T @ np.abs(L1) @ np.abs(Acl) + np.abs(sym(Sb[k]))
                                 + np.abs(Kk).T @ (np.abs(ub[k])[:, None] * np.abs(Kk)) + Ra))
    return {"S0_bar": Lam[0].copy(), "W_bar": W_bar, "Lambda": Lam, "obs_var_bar": ov_bar, "K_bar": K_bar,
            "ubar_bar": u_bar, "Xbar_bar": X_bar, "p_bar": p_bar,
            "aL": aL, "aK": aK, "aU": aU, "aX": aX, "aW": aW, "aO": aO, "aP": aP}


OUT = ("S0_bar", "W_bar", "Lambda", "obs_var_bar", "K_bar", "ubar_bar", "Xbar_bar", "p_bar")


def adjoint_batch(prob, P, ubar, Xbar, K, Sigma, Sb=None, ub=None, gb=None, **kw):
    """Every case of every scenario: P (B, np), ubar (B, nw), Xbar (B, N + 1, nx), K (B, N, nu, nx) or None,
    Sigma and Sb (B, nc, N + 1, nx, nx), ub (B, nc, N, nu), gb (B, nc, N + 1, m).  Returns every entry of
    adjoint_one's result with (B, nc) in front."""
    N, nu = prob.N, prob.nu
    B, nc = Sigma.shape[:2]
    out = None
    for b in range(B):
        for c in range(nc):
            r = adjoint_one(prob, P[b], np.asarray(ubar[b], float).reshape(N, nu), Xbar[b], None if K is None else K[b],
                            Sigma[b, c], None if Sb is None else Sb[b, c], None if ub is None else ub[b, c],
                            None if gb is None else gb[b, c], **kw)
            r = {k: v for k, v in r.items() if v is not None}
            if out is None:
                out = {k: np.zeros((B, nc) + v.shape, dtype=v.dtype) for k, v in r.items()}
            for k, v in r.items():
                out[k][b, c] = v
    return out


def loss_one(prob, p, ubar, Xbar, K, S0, W, obs_var, Sb, ub, gb):
    """L of the module docstring through covariance_ref.covariance_one."""
    r = cr.covariance_one(prob, p, ubar, Xbar, K, S0, W, obs_var)
    return float(np.sum(Sb * r["Sigma"]) + np.sum(ub * r["var_u"]) + np.sum(gb * r["var_g"]))
