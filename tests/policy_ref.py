"""Checker side of the feedback-policy tests (tests/test_gpu_policy.py, tests/test_policy_capi.py),
on the oracle alone: the neighbouring-extremal policy along a solution's plan,

    u_k(x, p') ~ u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d,      p' - p = sum_d c_d dp_d.

It is tests/kkt_ref.riccati_np's recursion returning (K, k), with one more term: stage 0's cross
term S_0 from oracle.nmpc_oracle.dyn_hess at stage 0 and the adjoint lam_1 (kkt_ref.stage_terms
loops from 1: with dX_0 = 0 a Newton step never reads it).  The right-hand side (r_k = hp,
q_k = G_k' (sigma_s jp)) and xi = (dX/dp) dp come from tests/solve_tangent_ref.dense_tangent
(`hp`, `jp`, dn["Xp"]), and kff = k - K xi.

Gate (a), the policy identity against the dense matrix: with dX^_0 = dp[x0],
    dw^_k = K_k dX^_k + kff_k,   dX^_{k+1} = A_k dX^_k + B_k dw^_k
must solve the dense system of the tangent checker,
    |M dw^ - rhs|_inf / (| |M| a |_inf + |rhs|_inf) <= kkt_ref.TOL,  a_k = |K_k| (|dX^_k| + |xi_k|) + |k_k|
on the free variables, the largest over the directions.  a replaces |dw^| of kkt_ref.rho: kff
cancels against K xi where dx is ~1e-9, so |dw^| does not measure the terms that were rounded.
Gate (c), K_0: for the unit directions of p's x0 block max |kff_0| <= 10 delta, asserted only at
delta <= 1e-10 (in exact arithmetic kff vanishes there at delta = 0; the slack block's delta
leaves delta G' jp, measured 0.26 delta).

Mutants, for the teeth of the gates:
  "noS":       every S_k dropped                 (gate (a))
  "noS0":      S_0 dropped: the K_0 that the solve kernels store    (gate (c))
  "rawk":      kff = k                           (gate (a))
  "shift":     K_{k+1} in K_k's place            (gate (a))
  "transpose": each block's layout transposed    (gate (a))"""
from __future__ import annotations

import numpy as np

from tests import adjoint_ref as ar
from tests import kkt_ref as kr
from tests import solve_adjoint_ref as sr
from tests import solve_tangent_ref as tr

TOL_A = kr.TOL
TOL_B = ar.TOL
C_FACTOR = 10.0      # gate (c): max |kff_0| <= C_FACTOR delta
C_DELTA = 1e-10      # ... where delta <= C_DELTA
MUTANTS = ("noS", "noS0", "rawk", "shift", "transpose")
GATE_OF = {"noS": "a", "noS0": "c", "rawk": "a", "shift": "a", "transpose": "a"}
SOLVED = sr.SOLVED
LADDER_FINE = (1e-12, 100.0, 8.0, 1e20)  # first_hessian_perturbation = 1e-12


def directions(spec, B, seed):
    """dp (B, np + 2, np): dp = I and two N(0, 1) directions."""
    return np.concatenate([np.repeat(np.eye(spec.np)[None], B, axis=0), tr.draw_directions(spec, B, 2, seed)], axis=1)


def dense_ladder_delta(prob, x, lam_g, lam_x, p, bounds, ladder, g=None, brf=1e-8):
    """The delta of the dense ladder (solve_adjoint_ref.ladder_delta) at a point."""
    from oracle import nmpc_oracle as orc

    lbx, ubx, lbg, ubg = bounds
    ev = orc.SSEval(prob, x, p)
    W = ev.hessian(1.0, lam_g)
    sx = kr.barrier_weights(x, lam_x, lbx, ubx, brf)
    ss = kr.barrier_weights(ev.g if g is None else g, lam_g, lbg, ubg, brf)
    free = np.isfinite(sx)
    return sr.ladder_delta(lambda dl: kr.dense_M(ev, W, np.where(free, sx, 0.0), ss, dl)[np.ix_(free, free)], ladder)


def recursion(ev, lam_g, sx, ss, delta, hp, jp, fixed, drop=None):
    """kkt_ref.riccati_np's backward sweep with S_0, every right-hand side at once: K (N, nu, nx),
    k (nd, N, nu).  drop: None, "all" (every S_k) or "S0"."""
    from oracle import nmpc_oracle as orc

    prob = ev.prob
    N, m, nx, nu = prob.N, prob.m, prob.nx, prob.nu
    Hxx, Hxu = kr.stage_terms(ev, 1.0, lam_g)
    lam = np.asarray(lam_g, float).reshape(N + 1, m)
    adj = np.zeros((N + 2, nx))
    for k in range(N, 0, -1):
        adj[k] = ev.gl[k] + ev.Gk[k].T @ lam[k]
        if k < N:
            adj[k] += ev.A[k].T @ adj[k + 1]
    Hxu = Hxu.copy()
    Hxu[0] = orc.dyn_hess(prob, ev.X[:, 0], ev.U[:, 0], adj[1])[1]
    if drop == "all":
        Hxu[:] = 0.0
    elif drop == "S0":
        Hxu[0] = 0.0
    nd = hp.shape[0]
    w = (ss + delta).reshape(N + 1, m)
    sj = (ss * jp).reshape(nd, N + 1, m)
    Q, q = np.zeros((N + 1, nx, nx)), np.zeros((N + 1, nx, nd))
    for k in range(1, N + 1):
        Q[k] = Hxx[k] + ev.Gk[k].T @ (w[k][:, None] * ev.Gk[k])
        q[k] = ev.Gk[k].T @ sj[:, k, :].T
    P, p = Q[N], q[N]
    K, kk = np.zeros((N, nu, nx)), np.zeros((N, nu, nd))
    for k in range(N - 1, -1, -1):
        A, B = ev.A[k], ev.B[k]
        f = fixed[nu * k:nu * k + nu]
        R = np.diag(np.where(f, 0.0, sx[nu * k:nu * k + nu]) + delta) + B.T @ P @ B
        S = Hxu[k].T + B.T @ P @ A
        r = hp[:, nu * k:nu * k + nu].T + B.T @ p
        R[f, :] = 0.0
        R[:, f] = 0.0
        R[f, f] = 1.0
        S[f, :] = 0.0
        r[f, :] = 0.0
        L = np.linalg.cholesky(R)
        K[k] = -np.linalg.solve(L.T, np.linalg.solve(L, S))
        kk[k] = -np.linalg.solve(L.T, np.linalg.solve(L, r))
        P, p = Q[k] + A.T @ P @ A + S.T @ K[k], q[k] + A.T @ p + K[k].T @ r
        P = 0.5 * (P + P.T)
    return K, np.ascontiguousarray(np.transpose(kk, (2, 0, 1)))


def dense_policy(prob, x, lam_g, lam_x, p, bounds, dp, delta=None, mutant=None, g=None, brf=1e-8, ladder=sr.LADDER):
    """One scenario; dp (nd, np); delta None = the dense ladder's.  Returns K (N, nu, nx), kff and
    k (nd, N, nu), xi (nd, N + 1, nx), A, B of the oracle, the delta used and `tan`, the dense
    tangent checker's result at that delta (M, rhs, free, dx, dX)."""
    lbx, ubx, lbg, ubg = bounds
    if delta is None:
        delta = dense_ladder_delta(prob, x, lam_g, lam_x, p, bounds, ladder, g=g, brf=brf)
        assert delta is not None, "no rung of the ladder factorises"
    tan = tr.dense_tangent(prob, x, lam_g, lam_x, p, bounds, dp, delta=delta, g=g, brf=brf)
    ev = tan["ev"]
    N, nx, nu = prob.N, prob.nx, prob.nu
    sx = kr.barrier_weights(x, lam_x, lbx, ubx, brf)
    fixed = ~tan["free"]
    drop = {"noS": "all", "noS0": "S0"}.get(mutant)
    K, k = recursion(ev, lam_g, np.where(fixed, 0.0, sx), tan["ss"], delta, tan["hp"], tan["jp"], fixed, drop)
    nd = dp.shape[0]
    xi = (dp @ tan["dn"]["Xp"].T).reshape(nd, N + 1, nx)
    kff = k.copy() if mutant == "rawk" else k - np.einsum("kij,dkj->dki", K, xi[:, :N])
    kff[:, fixed.reshape(N, nu)] = 0.0
    if mutant == "shift":
        K = np.concatenate([K[1:], K[-1:]], axis=0)
    elif mutant == "transpose":  # the column-major block read row by row
        K = np.stack([Kk.flatten(order="F").reshape(nu, nx) for Kk in K])
    return {"K": K, "kff": kff, "k": k, "xi": xi, "A": ev.A.copy(), "B": ev.B.copy(), "delta": delta, "tan": tan,
            "X": ev.X.T.copy()}


def policy_of(name, b, dp, mutant=None, delta=None, ladder=sr.LADDER):
    """The checker at scenario b of a solved case (tests/solve_adjoint_ref.solved); dp (B, nd, np)."""
    spec, prob, P, bounds, sols = sr.solved(name)
    s = sols[b]
    return dense_policy(prob, s["x"], s["lam_g"], s["lam_x"], P[b], bounds, dp[b], delta=delta, mutant=mutant,
                        ladder=ladder)


def propagate(K, kff, A, B, dX0):
    """dw^ (nd, N, nu), dX^ (nd, N + 1, nx) of the policy from dX^_0 (nd, nx)."""
    nd, N, nu = kff.shape
    nx = K.shape[2]
    dw, dX = np.zeros((nd, N, nu)), np.zeros((nd, N + 1, nx))
    dX[:, 0] = dX0
    for k in range(N):
        dw[:, k] = dX[:, k] @ K[k].T + kff[:, k]
        dX[:, k + 1] = dX[:, k] @ A[k].T + dw[:, k] @ B[k].T
    return dw, dX


def scale_a(K, k, xi, dX):
    """a_k = |K_k| (|dX^_k| + |xi_k|) + |k_k|, (nd, N, nu)."""
    N = K.shape[0]
    return np.einsum("kij,dkj->dki", np.abs(K), np.abs(dX[:, :N]) + np.abs(xi[:, :N])) + np.abs(k)


def gate_a(got, ref, dp):
    """The figure of gate (a) for one scenario: got holds K, kff, A, B (the policy under test);
    ref the checker's result at the same delta (its M, rhs, free set, xi and k for the scale)."""
    tan = ref["tan"]
    free = tan["free"]
    nx = got["K"].shape[2]
    with np.errstate(invalid="ignore", over="ignore"):
        dw, dX = propagate(got["K"], got["kff"], got["A"], got["B"], dp[:, :nx])
        a = scale_a(got["K"], ref["k"], ref["xi"], dX)
        worst = 0.0
        for d in range(dp.shape[0]):
            w, av, rhs = dw[d].reshape(-1)[free], a[d].reshape(-1)[free], tan["rhs"][d]
            r = float(np.max(np.abs(tan["M"] @ w - rhs), initial=0.0))
            den = float(np.max(np.abs(tan["M"]) @ av, initial=0.0)) + float(np.max(np.abs(rhs), initial=0.0))
            if not np.isfinite(r):
                return np.inf
            worst = max(worst, r / den if den > 0 else (0.0 if r == 0 else np.inf))
    return worst


def gate_c(kff, nx):
    """max |kff_0| over the unit directions of p's x0 block (the first nx directions of dp = I)."""
    return float(np.max(np.abs(kff[:nx, 0])))
