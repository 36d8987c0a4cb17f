"""Checker side of the policy-rollout adjoint tests (tests/test_gpu_policy_rollout_adjoint.py,
tests/test_rollout_adjoint_capi.py), on the oracle alone: the reverse sweep of tests/rollout_ref.py's
rollout_one at its trajectory X, one sample at a time, with oracle.nmpc_oracle's dyn_jac and
stage_cost_derivs.  For seeds Jb on J, Xb on X and Ub on the applied controls U,

    lam_N = Xb_N
    k = N-1 ... 0:  u_raw = ubar_k + K_k (x_k - Xbar_k),  u_k = clamp(u_raw)
                    mask_r = 1 where u_k[r] == u_raw[r], else 0
                    A_k, B_k = dyn_jac(x_k, u_k)
                    mu     = mask * (B_k^T lam_{k+1} + Ub_k)
                    wbar_k = lam_{k+1}
                    lam_k  = Jb grad l_k(x_k; p) + Xb_k + A_k^T lam_{k+1} + K_k^T mu
                    ubar_bar_k = mu,  K_bar_k = mu (x_k - Xbar_k)^T,  Xbar_bar_k = -K_k^T mu
                    p_bar[target x, y] -= Jb (grad l_k)[0, 1]
                    p_bar[w1_pidx] += Jb dd_k,  p_bar[w2_pidx] += Jb (Q_k - 1)   (uav5: no w2 term)
    e0_bar = lam_0,  p_bar[x0 block] += lam_0

is the gradient of Jb J + <Xb, X> + <Ub, U> with respect to (ubar, K, Xbar, p, e0, w).  Beside every
reduced output the checker returns S, the sum of the absolute values of the terms that make the entry
up (the scale a rounding error of the sum is measured against).  `adjoint_batch` adds the samples of a
scenario in sample order.

Mutants, for the teeth of the CPU gate (tests/test_rollout_adjoint_capi.py):
  "nomask":    the clamp's derivative taken as 1          (acts on samples with nsat > 0)
  "noKt":      the K_k^T mu term dropped from lam_k       (acts where K != 0)
  "shiftlam":  wbar_k = lam_k instead of lam_{k+1}        (acts everywhere)
  "transpose": each K_bar block written row-major into the column-major block (acts where K != 0)"""
from __future__ import annotations

import dataclasses

import numpy as np

MUTANTS = ("nomask", "noKt", "shiftlam", "transpose")
REDUCED = ("ubar_bar", "K_bar", "Xbar_bar", "p_bar")
PER_SAMPLE = ("e0_bar", "w_bar")


def read_entries(prob):
    """Indices of p that J, X and U read: the x0 block, the target's x and y, the weights' entries."""
    ti = prob.target_index
    idx = list(range(prob.nx)) + [ti, ti + 1]
    if prob.w1_pidx >= 0:
        idx.append(prob.w1_pidx)
    if prob.w2_pidx >= 0 and prob.model != "uav5":
        idx.append(prob.w2_pidx)
    return idx


def adjoint_one(prob, p, ubar, Xbar, K, X, Jb=0.0, Xb=None, Ub=None, lbx=None, ubx=None, mutant=None):
    """One sample.  Shapes as rollout_ref.rollout_one's; X (N + 1, nx) is its trajectory, Xb (N + 1, nx)
    and Ub (N, nu) or None.  Returns ubar_bar (N, nu), K_bar (N, nu, nx), Xbar_bar (N + 1, nx), p_bar
    (np,), e0_bar (nx,), w_bar (N, nx), nsat, and "S": the absolute-term sums of the four reduced ones."""
    from oracle import nmpc_oracle as orc

    N, nx, nu = prob.N, prob.nx, prob.nu
    p = np.asarray(p, float)
    pw = prob.weighted(p)
    pq = dataclasses.replace(pw, w1=0.0, w2=1.0)  # its stage cost is Q - 1
    ti = prob.target_index
    Xb = np.zeros((N + 1, nx)) if Xb is None else np.asarray(Xb, float)
    Ub = np.zeros((N, nu)) if Ub is None else np.asarray(Ub, float)
    out = {"ubar_bar": np.zeros((N, nu)), "K_bar": np.zeros((N, nu, nx)), "Xbar_bar": np.zeros((N + 1, nx)),
           "p_bar": np.zeros(len(p)), "w_bar": np.zeros((N, nx))}
    S = {k: np.zeros_like(out[k]) for k in REDUCED}
    nsat = 0
    lam = Xb[N].copy()
    for k in range(N - 1, -1, -1):
        x = X[k]
        dx = x - Xbar[k]
        ur = ubar[k] + (K[k] @ dx if K is not None else 0.0)
        u = ur.copy()
        if lbx is not None:
            u = np.where(u < lbx[k], lbx[k], u)
        if ubx is not None:
            u = np.where(u > ubx[k], ubx[k], u)
        mask = (u == ur).astype(float)
        nsat += int(np.sum((u != ur) & ~np.isnan(ur)))
        if mutant == "nomask":
            mask = np.ones(nu)
        A, Bm = orc.dyn_jac(prob, x, u)
        mu = mask * (Bm.T @ lam + Ub[k])
        amu = mask * (np.abs(Bm).T @ np.abs(lam) + np.abs(Ub[k]))
        out["w_bar"][k] = lam
        ktm = K[k].T @ mu if K is not None else np.zeros(nx)
        g = np.zeros(nx)
        if Jb != 0.0:
            _, g, _ = orc.stage_cost_derivs(pw, x, p[ti], p[ti + 1])
            g = Jb * g
            out["p_bar"][ti] -= g[0]
            out["p_bar"][ti + 1] -= g[1]
            S["p_bar"][ti] += abs(g[0])
            S["p_bar"][ti + 1] += abs(g[1])
            if prob.w1_pidx >= 0:
                t = Jb * float(np.hypot(x[0] - p[ti], x[1] - p[ti + 1]))
                out["p_bar"][prob.w1_pidx] += t
                S["p_bar"][prob.w1_pidx] += abs(t)
            if prob.w2_pidx >= 0 and prob.model != "uav5":
                t = Jb * orc.stage_cost(pq, x, p[ti], p[ti + 1])
                out["p_bar"][prob.w2_pidx] += t
                S["p_bar"][prob.w2_pidx] += abs(t)
        lam = g + Xb[k] + A.T @ lam + (0.0 if mutant == "noKt" else ktm)
        if mutant == "shiftlam":
            out["w_bar"][k] = lam
        out["ubar_bar"][k] = mu
        S["ubar_bar"][k] = amu
        if K is not None:
            blk = np.outer(mu, dx)
            out["K_bar"][k] = blk.flatten(order="C").reshape(nx, nu).T if mutant == "transpose" else blk
            S["K_bar"][k] = np.outer(amu, np.abs(dx))
            out["Xbar_bar"][k] = -ktm
            S["Xbar_bar"][k] = np.abs(K[k]).T @ amu
    out["e0_bar"] = lam
    out["p_bar"][:nx] += lam
    S["p_bar"][:nx] += np.abs(lam)
    out["nsat"] = nsat
    out["S"] = S
    return out


def adjoint_batch(prob, P, ubar, Xbar, K, X, Jb=None, Xb=None, Ub=None, lbx=None, ubx=None, mutant=None):
    """Every sample of every scenario, the reduced outputs added in sample order: P (B, np), ubar
    (B, nw), Xbar (B, N + 1, nx), K (B, N, nu, nx) or None, X (B, M, N + 1, nx), seeds Jb (B, M), Xb
    (B, M, N + 1, nx), Ub (B, M, N, nu) or None, bounds (nw,) shared or (B, nw).  Returns ubar_bar (B, nw),
    K_bar (B, N, nu, nx), Xbar_bar (B, N + 1, nx), p_bar (B, np), e0_bar (B, M, nx), w_bar (B, M, N, nx),
    nsat (B, M) and "S", the reduced outputs' absolute-term sums in the same shapes."""
    N, nx, nu = prob.N, prob.nx, prob.nu
    B, M = X.shape[:2]

    def bnd(v, b):
        if v is None:
            return None
        v = np.asarray(v, float)
        return (v if v.ndim == 1 else v[b]).reshape(N, nu)

    per = {"ubar_bar": np.zeros((B, M, N * nu)), "K_bar": np.zeros((B, M, N, nu, nx)),
           "Xbar_bar": np.zeros((B, M, N + 1, nx)), "p_bar": np.zeros((B, M, P.shape[1]))}
    out = {"e0_bar": np.zeros((B, M, nx)), "w_bar": np.zeros((B, M, N, nx)), "nsat": np.zeros((B, M), dtype=np.int32)}
    Sp = {k: np.zeros_like(per[k]) for k in REDUCED}
    for b in range(B):
        for s in range(M):
            r = adjoint_one(prob, P[b], np.asarray(ubar[b], float).reshape(N, nu), Xbar[b], None if K is None else K[b],
                            X[b, s], 0.0 if Jb is None else float(Jb[b, s]), None if Xb is None else Xb[b, s],
                            None if Ub is None else Ub[b, s], bnd(lbx, b), bnd(ubx, b), mutant=mutant)
            for k in REDUCED:
                per[k][b, s] = r[k].reshape(per[k].shape[2:])
                Sp[k][b, s] = r["S"][k].reshape(per[k].shape[2:])
            out["e0_bar"][b, s], out["w_bar"][b, s], out["nsat"][b, s] = r["e0_bar"], r["w_bar"], r["nsat"]
    out["per"], out["Sper"] = per, Sp
    return reduce_samples(out, M)


def reduce_samples(res, M):
    """adjoint_batch's result restricted to the first M samples: the reduced outputs and their S
    added in sample order over them, the per-sample outputs cut."""
    out = {k: res[k][:, :M] for k in PER_SAMPLE + ("nsat",)}
    out["per"], out["Sper"], out["S"] = res["per"], res["Sper"], {}
    for k in REDUCED:
        acc, accS = np.zeros_like(res["per"][k][:, 0]), np.zeros_like(res["per"][k][:, 0])
        for s in range(M):
            acc = acc + res["per"][k][:, s]
            accS = accS + res["Sper"][k][:, s]
        out[k], out["S"][k] = acc, accS
    return out


def clamp_set(U, lbx, ubx):
    """The entries of U on a face of the clamp box."""
    on = np.zeros(U.shape, dtype=bool)
    if lbx is not None:
        on |= U == lbx
    if ubx is not None:
        on |= U == ubx
    return on


def loss_one(r, Jb, Xb, Ub):
    """Jb J + <Xb, X> + <Ub, U> of one rollout_one result."""
    return Jb * r["J"] + float(np.sum(Xb * r["X"])) + float(np.sum(Ub * r["U"]))
