"""Checker side of the policy-covariance tests (tests/test_gpu_policy_covariance.py,
tests/test_covariance_capi.py), on the oracle alone: the first-order covariance of the state around
the plan under the feedback policy, one (scenario, case) at a time, with oracle.nmpc_oracle's dyn_jac
and obstacle_derivs and prob.box_states,

    Sigma_0 = S0                                             (lower triangle, mirrored)
    k = 0 ... N-1:  Acl_k      = A_k + B_k K_k                (K None: A_k)
                    var_u[k]   = diag(K_k Sigma_k K_k')       (K None: 0)
                    var_g[k,i] = Sigma_k[bi, bi]              box row i on state bi
                               = g' Sigma_k[0:2, 0:2] g + obs_var[o]     obstacle row o at Xbar_k
                    Sigma_{k+1} = Acl_k Sigma_k Acl_k' + W    (W None: 0)
    var_g[N] at Sigma_N, Xbar_N

and, for the tolerances of the GPU test, one step's magnitudes at the checker's own Sigma_k:
    a[k]    = max entry of |Acl_k| |Sigma_k| |Acl_k|' + |W|
    su[k]   = diag(|K_k| |Sigma_k| |K_k|'),   sg[k, i] = |g|' |Sigma_k| |g| + obs_var.
`order` picks the association of the triple product (0: (Acl Sigma) Acl', 1: Acl (Sigma Acl')) and
`dtype` the arithmetic (np.float64 or np.longdouble): two fp64 orders and fp64 against long double
show what rounding alone moves.  Acl_k itself is formed in fp64 in both: it is data of the recursion.
Where the policy is deadbeat in a state (1 + T K_k[r, c] ~ 1e-10 on the solved cases) that state's
variance is ~1e-21 beside 0.5 for the positions, and is set by the last bits of Acl_k, so a comparison
relative to the variance itself is only meaningful between evaluations that share Acl_k; B_k's
integrator rows hold T alone, so there Acl_k = fl(A_k + fl(T K_k)) entry by entry, which the kernel
reproduces bitwise (its products are rounded before their sums in forming Acl_k).

Mutants, for the teeth of the CPU gate (tests/test_covariance_capi.py):
  "transpose": Acl' Sigma Acl in place of Acl Sigma Acl'
  "shift":     K_{k+1} in K_k's place
  "noW":       the process noise dropped
  "openloop":  the gains dropped"""
from __future__ import annotations

import numpy as np

MUTANTS = ("transpose", "shift", "noW", "openloop")


def mirror(S):
    """The symmetric matrix whose lower triangle is S's."""
    L = np.tril(S)
    return L + np.tril(S, -1).T


def covariance_one(prob, p, ubar, Xbar, K, S0, W=None, obs_var=None, mutant=None, order=0, dtype=np.float64):
    """One (scenario, case).  ubar (N, nu), Xbar (N + 1, nx), K (N, nu, nx) or None, S0 and W (nx, nx)
    (W None: no noise), obs_var (n_obs,) or None.  Returns Sigma (N + 1, nx, nx), var_u (N, nu), var_g
    (N + 1, m) and the scales a (N,), su (N, nu), sg (N + 1, m)."""
    from oracle import nmpc_oracle as orc

    N, nx, nu, m, nb = prob.N, prob.nx, prob.nu, prob.m, prob.nb
    p = np.asarray(p, float)
    ox, oy = prob.obstacles(p)
    ov = np.zeros(prob.n_obs) if obs_var is None else np.asarray(obs_var, float)
    if mutant == "openloop":
        K = None
    if mutant == "shift" and K is not None:
        K = np.concatenate([K[1:], K[-1:]], axis=0)
    S = mirror(np.asarray(S0, float)).astype(dtype)
    Wm = None if (W is None or mutant == "noW") else mirror(np.asarray(W, float)).astype(dtype)
    Sigma = np.zeros((N + 1, nx, nx), dtype=dtype)
    var_u, var_g = np.zeros((N, nu), dtype=dtype), np.zeros((N + 1, m), dtype=dtype)
    a, su, sg = np.zeros(N), np.zeros((N, nu)), np.zeros((N + 1, m))

    def rows(k):
        for i, bi in enumerate(prob.box_states):
            var_g[k, i] = S[bi, bi]
            sg[k, i] = abs(S[bi, bi])
        if prob.n_obs:
            with np.errstate(invalid="ignore", divide="ignore"):
                G = orc.obstacle_derivs(Xbar[k], ox, oy)[0].astype(dtype)
            S2 = S[:2, :2]
            for o in range(prob.n_obs):
                var_g[k, nb + o] = G[o] @ S2 @ G[o] + ov[o]
                sg[k, nb + o] = np.abs(G[o]) @ np.abs(S2) @ np.abs(G[o]) + ov[o]

    for k in range(N):
        Sigma[k] = S
        rows(k)
        try:
            A, Bm = orc.dyn_jac(prob, Xbar[k], ubar[k])
        except (ValueError, OverflowError):  # math.* on inf / nan
            A, Bm = np.full((nx, nx), np.nan), np.full((nx, nu), np.nan)
        Acl = A
        if K is not None:
            Kk = K[k].astype(dtype)
            with np.errstate(invalid="ignore"):
                Acl = A + Bm @ K[k]  # fp64 whatever `dtype`: Acl is data of the recursion (module docstring)
        Acl = Acl.astype(dtype)
        if K is not None:
            with np.errstate(invalid="ignore"):
                var_u[k] = np.diag(Kk @ S @ Kk.T)
                su[k] = np.diag(np.abs(Kk) @ np.abs(S) @ np.abs(Kk).T)
        with np.errstate(invalid="ignore", over="ignore"):
            a[k] = float(np.max(np.abs(Acl) @ np.abs(S) @ np.abs(Acl).T + (0.0 if Wm is None else np.abs(Wm))))
            if mutant == "transpose":
                S = (Acl.T @ S) @ Acl
            elif order == 0:
                S = (Acl @ S) @ Acl.T
            else:
                S = Acl @ (S @ Acl.T)
            if Wm is not None:
                S = S + Wm
    Sigma[N] = S
    rows(N)
    return {"Sigma": Sigma, "var_u": var_u, "var_g": var_g, "a": a, "su": su, "sg": sg}


def sigma_of(var):
    """sqrt(max(var, 0)) that keeps a NaN."""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(var), np.nan, np.sqrt(np.maximum(var, 0.0)))


def covariance_batch(prob, P, ubar, Xbar, K, S0, W=None, obs_var=None, **kw):
    """Every case of every scenario: P (B, np), ubar (B, nw), Xbar (B, N + 1, nx), K (B, N, nu, nx) or
    None, S0 and W (B, nc, nx, nx), obs_var (B, n_obs) or None.  Returns Sigma (B, nc, N + 1, nx, nx),
    var_u (B, nc, N, nu), var_g (B, nc, N + 1, m) and the scales likewise."""
    N, nu = prob.N, prob.nu
    B, nc = S0.shape[:2]
    out = None
    for b in range(B):
        for c in range(nc):
            r = covariance_one(prob, P[b], np.asarray(ubar[b], float).reshape(N, nu), Xbar[b], None if K is None else K[b],
                               S0[b, c], None if W is None else W[b, c], None if obs_var is None else obs_var[b], **kw)
            if out is None:
                out = {k: np.zeros((B, nc) + v.shape, dtype=v.dtype) for k, v in r.items()}
            for k, v in r.items():
                out[k][b, c] = v
    return out


def draw_covariances(prob, B, sigma, seed=5):
    """S0 = 1/2 diag(sigma^2) + 1/2 Q Q' / nx with Q's rows N(0, 1) scaled by sigma, and W = 0.01 S0:
    (B, nx, nx) each."""
    nx = prob.nx
    sg = np.asarray(sigma, float)[:nx]
    rng = np.random.default_rng(seed)
    Q = rng.standard_normal((B, nx, nx)) * sg[:, None]
    S0 = 0.5 * np.diag(sg ** 2)[None] + 0.5 * Q @ np.swapaxes(Q, 1, 2) / nx
    S0 = 0.5 * (S0 + np.swapaxes(S0, 1, 2))
    return S0, 0.01 * S0


def sigma_points(S0, W, N):
    """The columns of the Cholesky factors of S0 (entering at stage 0) and of W (entering after each
    of the N stages): a list of (stage of entry, direction (nx,)), 0 = the initial state and j >= 1 =
    the process disturbance of stage j - 1."""
    pts = [(0, c) for c in np.linalg.cholesky(S0).T]
    if W is not None:
        L = np.linalg.cholesky(W)
        pts += [(j, c) for j in range(1, N + 1) for c in L.T]
    return pts
