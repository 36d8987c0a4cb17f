"""Checker side of the policy-rollout tests (tests/test_gpu_policy_rollout.py,
tests/test_rollout_capi.py), on the oracle alone: the clamped feedback policy on the nonlinear plant,
one sample at a time, with oracle.nmpc_oracle's dynamics, stage_cost and stage_rows,

    x_0 = p[x0 block] + e0
    k = 0 ... N-1:  u_raw = ubar_k + K_k (x_k - Xbar_k)        (K None: open-loop replay)
                    u_k   = min(max(u_raw, lbx_k), ubx_k)      (a bound None: not applied)
                    J    += stage_cost(x_k; p)
                    x_{k+1} = x_k + T f(x_k, u_k) + w_k        (w None: no process disturbance)
    viol = max over the rows of stages 0 ... N of max(g - ubg, lbg - g, 0)   (+-1e19 rule)
    nsat = number of control entries with u_k != u_raw

and `margin`, the smallest |u_raw - bound| over the control entries not exactly on that bound: how far
the sample is from a clamp decision that rounding could flip.  A NaN among the states, the controls,
the row values or the bounds met makes J and viol NaN.

At an interior-point solution a control active at the plan sits on its bound or ~1e-6 inside it, and
the barrier weight makes its gain row 1e-9 to 1e-4: clamped at the solve's own bounds its u_raw stays
1e-16 to 1e-7 from the bound whatever the disturbance (measured on all four solved cases), so no
choice of disturbances gives such a rollout a margin above rounding.  `widen` therefore returns the
box the tests clamp at: the solve's bounds moved outwards by WIDEN of each control's range, an
actuator limit slightly beyond the planning limit.

Mutants, for the teeth of the CPU gates (tests/test_rollout_capi.py):
  "transpose": each K block's layout transposed      (linearisation)
  "shift":     K_{k+1} in K_k's place                (linearisation)
  "noclamp":   the clamp dropped                     (the clamp property)"""
from __future__ import annotations

import numpy as np

MUTANTS = ("transpose", "shift", "noclamp")
BIG = 1e19


def _mutate_K(K, mutant):
    if K is None or mutant not in ("transpose", "shift"):
        return K
    if mutant == "shift":
        return np.concatenate([K[1:], K[-1:]], axis=0)
    nu, nx = K.shape[1:]
    return np.stack([Kk.flatten(order="F").reshape(nu, nx) for Kk in K])  # the column-major block read row by row


def rollout_one(prob, p, ubar, Xbar, K, e0, w=None, lbx=None, ubx=None, lbg=None, ubg=None, mutant=None):
    """One sample.  ubar (N, nu), Xbar (N + 1, nx), K (N, nu, nx) or None, e0 (nx,), w (N, nx) or
    None, lbx / ubx (N, nu) or None, lbg / ubg (N + 1, m) or None.  Returns X (N + 1, nx), U (N, nu),
    J, viol, nsat and margin."""
    from oracle import nmpc_oracle as orc

    N, nx, nu, T = prob.N, prob.nx, prob.nu, prob.T
    p = np.asarray(p, float)
    pw = prob.weighted(p)
    ti = prob.target_index
    ox, oy = prob.obstacles(p)
    f = orc.dynamics5 if prob.model == "uav5" else orc.dynamics
    K = _mutate_K(K, mutant)
    X, U = np.zeros((N + 1, nx)), np.zeros((N, nu))
    x = p[:nx] + np.asarray(e0, float)
    J, viol, nsat, margin, bad = 0.0, 0.0, 0, np.inf, False

    def rows(k, x):
        nonlocal viol, bad
        with np.errstate(invalid="ignore"):
            g = orc.stage_rows(prob, x, ox, oy)
        bad |= bool(np.any(np.isnan(g)))
        if lbg is not None:
            lo, hi = lbg[k], ubg[k]
            bad |= bool(np.any(np.isnan(lo)) or np.any(np.isnan(hi)))
            with np.errstate(invalid="ignore"):
                v = np.concatenate([(g - hi)[hi < BIG], (lo - g)[lo > -BIG], [0.0]])
            viol = max(viol, float(np.nanmax(v)))

    for k in range(N):
        X[k] = x
        bad |= bool(np.any(np.isnan(x)))
        rows(k, x)
        with np.errstate(invalid="ignore", over="ignore"):
            ur = ubar[k] + (K[k] @ (x - Xbar[k]) if K is not None else 0.0)
        u = ur.copy()
        if mutant != "noclamp":
            for bnd, side in ((lbx, 0), (ubx, 1)):
                if bnd is None:
                    continue
                bk = bnd[k]
                bad |= bool(np.any(np.isnan(bk)))
                with np.errstate(invalid="ignore"):
                    off = np.abs(ur - bk)
                    on = (off > 0) & np.isfinite(off)
                    u = np.where(u < bk, bk, u) if side == 0 else np.where(u > bk, bk, u)
                margin = min(margin, float(np.min(off[on], initial=np.inf)))
        bad |= bool(np.any(np.isnan(ur)))
        nsat += int(np.sum((u != ur) & ~np.isnan(ur)))
        U[k] = u
        try:
            J += orc.stage_cost(pw, x, p[ti], p[ti + 1])
            with np.errstate(invalid="ignore", over="ignore"):
                x = x + T * f(x, u)
        except (ValueError, OverflowError, ZeroDivisionError):  # math.* on inf / nan / a zero footprint
            J, x = np.nan, np.full(nx, np.nan)
        if w is not None:
            x = x + w[k]
    X[N] = x
    bad |= bool(np.any(np.isnan(x)))
    rows(N, x)
    if bad:
        J = viol = np.nan
    return {"X": X, "U": U, "J": J, "viol": viol, "nsat": nsat, "margin": margin}


def rollout_batch(prob, P, ubar, Xbar, K, e0, w=None, lbx=None, ubx=None, lbg=None, ubg=None, mutant=None):
    """Every sample of every scenario: P (B, np), ubar (B, nw), Xbar (B, N + 1, nx), K (B, N, nu, nx)
    or None, e0 (B, M, nx), w (B, M, N, nx) or None; bounds (n,) shared or (B, n).  Returns X
    (B, M, N + 1, nx), U (B, M, N, nu), J, viol, nsat, margin (B, M)."""
    N, nx, nu, m = prob.N, prob.nx, prob.nu, prob.m
    B, M = e0.shape[:2]

    def bnd(v, b, shape):
        if v is None:
            return None
        v = np.asarray(v, float)
        return (v if v.ndim == 1 else v[b]).reshape(shape)

    out = {"X": np.zeros((B, M, N + 1, nx)), "U": np.zeros((B, M, N, nu)), "J": np.zeros((B, M)),
           "viol": np.zeros((B, M)), "nsat": np.zeros((B, M), dtype=np.int32), "margin": np.zeros((B, M))}
    for b in range(B):
        for s in range(M):
            r = rollout_one(prob, P[b], np.asarray(ubar[b], float).reshape(N, nu), Xbar[b], None if K is None else K[b],
                            e0[b, s], None if w is None else w[b, s], bnd(lbx, b, (N, nu)), bnd(ubx, b, (N, nu)),
                            bnd(lbg, b, (N + 1, m)), bnd(ubg, b, (N + 1, m)), mutant=mutant)
            for k in out:
                out[k][b, s] = r[k]
    return out


WIDEN = 1e-3


def widen(lbx, ubx):
    """The clamp box of the tests: (lbx, ubx) moved outwards by WIDEN (ubx - lbx)."""
    lbx, ubx = np.asarray(lbx, float), np.asarray(ubx, float)
    return lbx - WIDEN * (ubx - lbx), ubx + WIDEN * (ubx - lbx)


def draw_disturbances(prob, B, M, sigma, seed, big=(), scale=1.0):
    """e0 (B, M, nx) ~ N(0, diag sigma^2) and w (B, M, N, nx) a tenth of that size; sample 0 is
    undisturbed and the samples listed in `big` are multiplied by `scale`."""
    rng = np.random.default_rng(seed)
    sg = np.asarray(sigma, float)[:prob.nx]
    e0 = rng.standard_normal((B, M, prob.nx)) * sg
    w = 0.1 * rng.standard_normal((B, M, prob.N, prob.nx)) * sg
    for s in big:
        if s < M:
            e0[:, s] *= scale
            w[:, s] *= scale
    e0[:, 0] = 0.0
    w[:, 0] = 0.0
    return e0, w
