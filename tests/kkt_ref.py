"""Checker side of the KKT-solve tests (tests/test_gpu_kkt.py, tests/test_kkt_capi.py), on
oracle.nmpc_oracle.SSEval alone: the dense condensed KKT matrix

    M = W + diag(sigma_x) + delta I + J' diag(sigma_s + delta) J,   W = SSEval.hessian(obj_factor, lam_g)

at the cases and points of tests/eval_ref.py, its dense solve (numpy.linalg.solve) and inertia
(eigvalsh), the weights of the two regimes, the choice of delta, the gate quantity, and a numpy
fp64 restatement of the stage-wise (Riccati) recursion the kernel runs.

Gate: the normwise residual against the dense matrix,

    rho(dw) = |M dw - rhs|_inf / (| |M| |dw| |_inf + |rhs|_inf),

which depends neither on the conditioning of M nor on the operation order of the solve.
Bound: rho <= eval_ref.TOL = 1e-10.  Its basis is measured by tests/test_kkt_capi.py wherever
the suite runs: the numpy restatement below and numpy's dense solve both stay below nw * 2.2e-16
on every scenario of every case in both regimes (measured with these draws: 7.6e-16 and 5.6e-16,
with cond(M) up to 1.2e15), so 1e-10 leaves more than five orders of magnitude for a different
operation order and is still 1,000x below a 1e-7 error.

Forward error |dw - ref|_inf <= 1e-6 |ref|_inf against the dense solve is gated in the mild
regime only (the restatement measures 8.7e-9 there, at cond(M) up to 9e10); in the barrier
regime it reaches 8e-4 at cond(M) = 1.2e15, which is conditioning, not error, so it is printed
and not gated.

Regimes (per scenario, seeded):
  mild:    sigma_x = 10^U(-3,3), sigma_s = 10^U(-4,4);
  barrier: sigma_x = 10^U(-8,8); a fifth of the rows 10^U(4,10), the rest 10^U(-9,-3);
  teeth:   sigma_x = 10^U(-3,0), sigma_s = 10^U(-4,0) -- weights <= 1, for the mutants: a large
           barrier weight would hide a Hessian error behind Sigma.
delta = 0 where lambda_min(M0) > 1e-6 max|M0| (M0 = M at delta = 0), else 2 |lambda_min| + 1e-4.

Right-hand sides, NR = 3 per scenario: r_w alone, r_g alone, both; r_w ~ N(0,1) (1 + |grad f|_inf),
r_g ~ N(0,1)."""
from __future__ import annotations

import functools

import numpy as np

from tests import eval_ref as er
from tests import products_ref as pr

TOL = er.TOL
FWD_TOL = 1e-6
NR = 3
REGIMES = ("mild", "barrier")
COMBOS = ((1.0, 0), (0.37, 1))  # (obj_factor, draw of lam_g)
INDEF = 1e-3   # lambda_min(M) < -INDEF max|M|: judged indefinite
PD = 1e-6      # lambda_min(M0) > PD max|M0|: delta = 0


def draw_weights(spec, B, regime, seed):
    """sigma_x (B, nw), sigma_s (B, ng) of a regime."""
    rng = np.random.default_rng(seed)
    if regime == "mild":
        return 10.0 ** rng.uniform(-3, 3, (B, spec.nw)), 10.0 ** rng.uniform(-4, 4, (B, spec.ng))
    if regime == "barrier":
        act = rng.uniform(size=(B, spec.ng)) < 0.2
        ss = np.where(act, 10.0 ** rng.uniform(4, 10, (B, spec.ng)), 10.0 ** rng.uniform(-9, -3, (B, spec.ng)))
        return 10.0 ** rng.uniform(-8, 8, (B, spec.nw)), ss
    if regime == "teeth":
        return 10.0 ** rng.uniform(-3, 0, (B, spec.nw)), 10.0 ** rng.uniform(-4, 0, (B, spec.ng))
    raise KeyError(regime)


def draw_rhs(ev, seed):
    """r_w (NR, nw), r_g (NR, ng): r_w alone, r_g alone, both."""
    rng = np.random.default_rng(seed)
    nw, ng = ev.prob.nw, ev.prob.ng
    rw = rng.standard_normal((NR, nw)) * (1.0 + float(np.max(np.abs(ev.gradF))))
    rg = rng.standard_normal((NR, ng))
    rw[1] = 0.0
    rg[0] = 0.0
    return rw, rg


def dense_M(ev, W, sx, ss, delta):
    J = ev.J
    return W + np.diag(sx + delta) + J.T @ ((ss + delta)[:, None] * J)


def choose_delta(M0):
    lmin = float(np.linalg.eigvalsh(M0)[0])
    return 0.0 if lmin > PD * float(np.max(np.abs(M0))) else 2.0 * abs(lmin) + 1e-4


def rhs_of(ev, rw, rg):
    """(NR, nw): r_w + J' r_g."""
    return rw + rg @ ev.J


def rho(M, dw, rhs):
    """Normwise residual of one column."""
    den = float(np.max(np.abs(M) @ np.abs(dw))) + float(np.max(np.abs(rhs)))
    r = float(np.max(np.abs(M @ dw - rhs)))
    if not np.isfinite(r):
        return np.inf
    return r / den if den > 0 else (0.0 if r == 0 else np.inf)


def stage_terms(ev, obj_factor, lam_g):
    """Hxx_k (N+1, nx, nx), Hxu_k (N+1, nx, nu) of SSEval.hessian, stage by stage (k >= 1)."""
    from oracle import nmpc_oracle as orc

    prob = ev.prob
    N, m, nx, nu, nb = prob.N, prob.m, prob.nx, prob.nu, prob.nb
    lam = np.asarray(lam_g, float).reshape(N + 1, m)
    adj = np.zeros((N + 2, nx))
    for k in range(N, 0, -1):
        adj[k] = obj_factor * ev.gl[k] + ev.Gk[k].T @ lam[k]
        if k < N:
            adj[k] += ev.A[k].T @ adj[k + 1]
    Hxx, Hxu = np.zeros((N + 1, nx, nx)), np.zeros((N + 1, nx, nu))
    for k in range(1, N + 1):
        Hxx[k] = obj_factor * ev.Hl[k]
        if prob.n_obs:
            Hxx[k, 0:2, 0:2] += np.einsum("j,jab->ab", lam[k, nb:], ev.Hg[k])
        if k < N:
            d, Hxu[k] = orc.dyn_hess(prob, ev.X[:, k], ev.U[:, k], adj[k + 1])
            Hxx[k] += d
    return Hxx, Hxu


def riccati_np(ev, obj_factor, lam_g, sx, ss, delta, rw, rg, fixed=None):
    """The stage-wise recursion restated in numpy fp64, every right-hand side at once:
      Q_k = Hxx_k + G_k' (sigma_s + delta) G_k (k >= 1), S_k = Hxu_k' + B' P A,
      R~_k = diag(sigma_x + delta) + B' P B, P_k = Q_k + A' P A + S~' K, dX_0 = 0;
    a fixed variable has a unit pivot and a zero S~ row.  Returns (dw (NR, nw) or None, ok):
    ok = every R~_k positive definite (Cholesky)."""
    prob = ev.prob
    N, m, nx, nu = prob.N, prob.m, prob.nx, prob.nu
    Hxx, Hxu = stage_terms(ev, obj_factor, lam_g)
    nr = rw.shape[0]
    w = (ss + delta).reshape(N + 1, m)
    rgk = rg.reshape(nr, N + 1, m)
    fx = np.zeros(prob.nw, bool) if fixed is None else fixed
    Q, q = np.zeros((N + 1, nx, nx)), np.zeros((N + 1, nx, nr))
    for k in range(1, N + 1):
        Q[k] = Hxx[k] + ev.Gk[k].T @ (w[k][:, None] * ev.Gk[k])
        q[k] = -(ev.Gk[k].T @ rgk[:, k, :].T)
    P, p = Q[N], q[N]
    K, kk = np.zeros((N, nu, nx)), np.zeros((N, nu, nr))
    for k in range(N - 1, -1, -1):
        A, B = ev.A[k], ev.B[k]
        f = fx[nu * k:nu * k + nu]
        R = np.diag(np.where(f, 0.0, sx[nu * k:nu * k + nu]) + delta) + B.T @ P @ B
        S = Hxu[k].T + B.T @ P @ A
        r = -rw[:, nu * k:nu * k + nu].T + B.T @ p
        R[f, :] = 0.0
        R[:, f] = 0.0
        R[f, f] = 1.0
        S[f, :] = 0.0
        r[f, :] = 0.0
        try:
            L = np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            return None, False
        K[k] = -np.linalg.solve(L.T, np.linalg.solve(L, S))
        kk[k] = -np.linalg.solve(L.T, np.linalg.solve(L, r))
        P, p = Q[k] + A.T @ P @ A + S.T @ K[k], q[k] + A.T @ p + K[k].T @ r
        P = 0.5 * (P + P.T)
    dw = np.zeros((nr, prob.nw))
    dx = np.zeros((nx, nr))
    for k in range(N):
        du = K[k] @ dx + kk[k]
        dw[:, nu * k:nu * k + nu] = du.T
        dx = ev.A[k] @ dx + ev.B[k] @ du
    return dw, True


@functools.lru_cache(maxsize=None)
def reference(name, regime, combo, seed=2024):
    """One (case, regime, combo): spec, inputs (x, p, lam_g, sigma_x, sigma_s, delta, r_w
    (B, NR, nw), r_g (B, NR, ng), obj_factor) and per scenario the dense M, M0's lambda_min
    ratio, rhs (NR, nw), the dense solve ref (NR, nw) and cond(M)."""
    spec, d, evs = pr.evals(name, seed)
    B = er.CASES[name]
    ci = COMBOS.index(combo)
    obj = combo[0]
    lam = 10.0 * np.random.default_rng(seed + 31 + combo[1]).standard_normal((B, spec.ng))
    sx, ss = draw_weights(spec, B, regime, seed + 100 * {"mild": 1, "barrier": 2, "teeth": 7}[regime] + ci)
    delta = np.zeros(B)
    rw, rg = np.zeros((B, NR, spec.nw)), np.zeros((B, NR, spec.ng))
    per = []
    for b, ev in enumerate(evs):
        W = ev.hessian(obj, lam[b])
        M0 = dense_M(ev, W, sx[b], ss[b], 0.0)
        delta[b] = choose_delta(M0)
        M = dense_M(ev, W, sx[b], ss[b], delta[b])
        rw[b], rg[b] = draw_rhs(ev, seed + 1000 + b)
        rhs = rhs_of(ev, rw[b], rg[b])
        per.append({"M": M, "W": W, "rhs": rhs, "ref": np.linalg.solve(M, rhs.T).T, "cond": float(np.linalg.cond(M)),
                    "lmin0": float(np.linalg.eigvalsh(M0)[0]) / float(np.max(np.abs(M0)))})
    inp = {"x": d["w"], "p": d["p"], "lam_g": lam, "sigma_x": sx, "sigma_s": ss, "delta": delta, "r_w": rw, "r_g": rg,
           "obj_factor": obj}
    return spec, inp, per, evs


def figures(dw, one, regime):
    """Per column: rho against the dense matrix and the forward error against the dense solve
    relative to |ref|_inf."""
    rhos = [rho(one["M"], dw[c], one["rhs"][c]) for c in range(dw.shape[0])]
    with np.errstate(invalid="ignore", divide="ignore"):
        fwd = [float(np.max(np.abs(dw[c] - one["ref"][c])) / np.max(np.abs(one["ref"][c]))) for c in range(dw.shape[0])]
    return max(rhos), max(fwd)


def check_solution(dw, one, regime, what=""):
    """dw (NR, nw) of one scenario.  Prints the figures before asserting them."""
    r, f = figures(np.asarray(dw, float), one, regime)
    print(f"{what}: rho {r:.2e} (bound {TOL:.0e}), forward {f:.2e}"
          f" ({'bound %.0e' % FWD_TOL if regime == 'mild' else 'not gated'}), cond {one['cond']:.1e}")
    assert r <= TOL, (what, "rho", r)
    if regime == "mild":
        assert f <= FWD_TOL, (what, "forward", f)
    return r, f


def check_steps(ev, dw, dX, jdw, what=""):
    """dX_out and jdw_out (NR, n) against Z dw and J dw of the oracle applied to the same dw,
    within TOL of the absolute-product scales of tests/products_ref.py."""
    Z, J = pr.stack_Z(ev), ev.J
    out = {}
    for k, A, got in (("dX", Z, dX), ("jdw", J, jdw)):
        ref, scale = dw @ A.T, np.max(np.abs(dw) @ np.abs(A).T, axis=1)
        err = np.max(np.abs(np.asarray(got, float) - ref), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(scale > 0, err / (TOL * scale), np.where(err == 0, 0.0, np.inf))
        out[k] = float(np.max(np.where(np.isnan(err), np.inf, q)))
    print(f"{what}: error / bound dX {out['dX']:.2e}, jdw {out['jdw']:.2e}")
    assert out["dX"] <= 1.0 and out["jdw"] <= 1.0, (what, out)
    return out


def indefinite_cases(name, seed=2024):
    """sigma = 0, delta = 0, lam_g random: per scenario lambda_min(M) / max|M| of M = W (the
    inertia test's verdict: < -INDEF judged indefinite) and the inputs."""
    spec, d, evs = pr.evals(name, seed)
    B = er.CASES[name]
    lam = 10.0 * np.random.default_rng(seed + 57).standard_normal((B, spec.ng))
    ratio = np.zeros(B)
    for b, ev in enumerate(evs):
        W = ev.hessian(1.0, lam[b])
        ratio[b] = float(np.linalg.eigvalsh(W)[0]) / max(float(np.max(np.abs(W))), 1e-300)
    return spec, {"x": d["w"], "p": d["p"], "lam_g": lam}, ratio


def mutant_W(ev, obj_factor, lam_g, which):
    """The oracle's Hessian with one part wrong (tests/products_ref.py's mutants)."""
    return pr.mutant_products(ev, np.eye(ev.prob.nw), obj_factor, lam_g, which)["hv"].T


# ---- sensitivity: the formula of Solver.sensitivity evaluated densely on the oracle
def barrier_weights(v, lam, lo, hi, brf=1e-8):
    with np.errstate(invalid="ignore"):
        sl = np.maximum(v - lo, brf * np.maximum(1.0, np.abs(lo)))
        su = np.maximum(hi - v, brf * np.maximum(1.0, np.abs(hi)))
        s = np.maximum(-lam, 0.0) / sl + np.maximum(lam, 0.0) / su
    return np.where(lo == hi, np.inf, s)


def dense_sensitivity(prob, x, lam_g, lam_x, p, dp, lbx, ubx, lbg, ubg, step, delta=0.0):
    """One scenario: dx (nd, nw), dlam_g (nd, ng), the reduced M and rhs (nd, nfree), the free
    index set, with the central differences of SSEval's grad_l and g at p +- step dp, M at the
    given delta (Solver.sensitivity reports the one it used)."""
    from oracle import nmpc_oracle as orc

    ev = orc.SSEval(prob, x, p)
    sx = barrier_weights(x, lam_x, lbx, ubx)
    ss = barrier_weights(ev.g, lam_g, lbg, ubg)
    free = np.isfinite(sx)
    M = dense_M(ev, ev.hessian(1.0, lam_g), np.where(free, sx, 0.0), ss, delta)
    nd = dp.shape[0]
    rhs, dg = np.zeros((nd, prob.nw)), np.zeros((nd, prob.ng))
    for j in range(nd):
        ep, em = orc.SSEval(prob, x, p + step * dp[j]), orc.SSEval(prob, x, p - step * dp[j])
        dgl = ((ep.gradF + ep.J.T @ lam_g) - (em.gradF + em.J.T @ lam_g)) / (2 * step)
        dg[j] = (ep.g - em.g) / (2 * step)
        rhs[j] = -dgl - ev.J.T @ (ss * dg[j])
    Mf = M[np.ix_(free, free)]
    dx = np.zeros((nd, prob.nw))
    dx[:, free] = np.linalg.solve(Mf, rhs[:, free].T).T
    dlam = ss * (dx @ ev.J.T + dg)
    return {"dx": dx, "dlam_g": dlam, "M": Mf, "rhs": rhs[:, free], "free": free, "cond": float(np.linalg.cond(Mf))}
