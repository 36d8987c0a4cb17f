"""Checker side of the fp32-leg step tests (tests/test_gpu_fp32_step.py, tests/test_fp32_step.py):
the stage-wise recursion of tests/kkt_ref.py::riccati_np restated with a precision argument, and
iterative refinement around it, on the cases, weights, right-hand sides and dense matrices of
tests/kkt_ref.py.

What the fp32 kernel classes do (nlpsol option linear_solver_precision="single"): the
factorisation (P_k, S~_k, R~_k and its Cholesky factor), the gains K_k and the backward vector
recursion with its solves for k_k run in float32; the gains are stored as doubles, and the forward
sweep du_k = K_k dx_k + k_k, dx_{k+1} = A dx_k + B du_k runs in fp64.  Solver::refine then forms
the residual of the step in fp64, solves it with the same float32 factors and adds the
correction.  Here:

    Factor(ev, ..., dtype)     the recursion with every backward quantity in `dtype`;
    Factor.solve(rw, rg)       one solve M dw = r_w + J' r_g: backward in `dtype`, forward in fp64;
    refine(F, M, dw, rhs)      dw + F.solve(rhs - M dw), the residual with the DENSE matrix in fp64
                               (not the kernel's stage-wise suffix sums: an independent form);
    steps(...)                 dw0, dw1, dw2: no, one and two refinements.

With dtype = float64 Factor.solve is operation for operation kkt_ref.riccati_np (asserted bitwise
by tests/test_fp32_step.py), which itself is unchanged.

Bounds of the GPU test, per case (max over scenarios and right-hand sides of a (case, regime,
combo)), all from this restatement and never from the kernel:

    rho(dw0) <= FACTOR * rho0_ref
    rho(dw1) <= bound1 = max(FACTOR * rho1_ref, nw * 2.2e-16)
    rho(dw2) <= bound2 = max(FACTOR * rho2_ref, nw * 2.2e-16)

FACTOR = 30 is the margin tests/trace_cases.py grants a different operation order; nw * 2.2e-16 is
the fp64 floor tests/kkt_ref.py documents.  SEPARATION: the CPU test asserts rho0_ref >= 100 *
bound1 on every mild and teeth case, so a refinement that did nothing misses bound1 by at least
100 / 30."""
from __future__ import annotations

import functools

import numpy as np

from tests import eval_ref as er
from tests import kkt_ref as kr

FACTOR = 30.0      # tests/trace_cases.FACTOR
MARGIN = 10.0      # tests/trace_cases.MARGIN: by how much a mutant must miss
SEPARATION = 100.0
EPS = float(np.finfo(float).eps)
GATED = ("mild", "teeth")
MUTANTS = ("no_delta", "no_Hxu", "no_sigma_x", "float32_residual")


class Factor:
    """The backward sweep of kkt_ref.riccati_np in `dtype`; ok = every R~_k positive definite
    and finite.  A fixed variable has a unit pivot and a zero S~ row."""

    def __init__(self, ev, obj_factor, lam_g, sx, ss, delta, dtype=np.float64, fixed=None):
        prob = ev.prob
        N, m, nx, nu = prob.N, prob.m, prob.nx, prob.nu
        t = self.t = np.dtype(dtype).type
        self.ev, self.N, self.m, self.nx, self.nu = ev, N, m, nx, nu
        Hxx, Hxu = kr.stage_terms(ev, obj_factor, lam_g)
        w = (ss + delta).reshape(N + 1, m)
        self.fx = np.zeros(prob.nw, bool) if fixed is None else np.asarray(fixed, bool)
        Q = np.zeros((N + 1, nx, nx))
        for k in range(1, N + 1):
            Q[k] = Hxx[k] + ev.Gk[k].T @ (w[k][:, None] * ev.Gk[k])
        Q = Q.astype(t)
        self.A = [np.asarray(ev.A[k]).astype(t) for k in range(N)]
        self.B = [np.asarray(ev.B[k]).astype(t) for k in range(N)]
        self.L, self.K = [None] * N, np.zeros((N, nu, nx), t)
        self.ok = True
        P = Q[N]
        with np.errstate(all="ignore"):
            for k in range(N - 1, -1, -1):
                A, B = self.A[k], self.B[k]
                f = self.fx[nu * k:nu * k + nu]
                R = np.diag((np.where(f, 0.0, sx[nu * k:nu * k + nu]) + delta).astype(t)) + B.T @ P @ B
                S = Hxu[k].T.astype(t) + B.T @ P @ A
                R[f, :] = 0.0
                R[:, f] = 0.0
                R[f, f] = 1.0
                S[f, :] = 0.0
                try:
                    if not np.all(np.isfinite(R)):
                        raise np.linalg.LinAlgError
                    L = np.linalg.cholesky(R)
                except np.linalg.LinAlgError:
                    self.ok = False
                    return
                self.L[k] = L
                self.K[k] = -np.linalg.solve(L.T, np.linalg.solve(L, S))
                P = Q[k] + A.T @ P @ A + S.T @ self.K[k]
                P = t(0.5) * (P + P.T)
                assert P.dtype == t and L.dtype == t

    def solve(self, rw, rg):
        """dw (nr, nw) of M dw = r_w + J' r_g: the vector recursion and k_k in the factor's
        precision, the forward sweep in fp64 with the stored gains."""
        ev, N, m, nx, nu, t = self.ev, self.N, self.m, self.nx, self.nu, self.t
        nr = rw.shape[0]
        rgk = rg.reshape(nr, N + 1, m)
        q = np.zeros((N + 1, nx, nr), t)
        for k in range(1, N + 1):
            q[k] = (-(ev.Gk[k].T @ rgk[:, k, :].T)).astype(t)
        p = q[N]
        kk = np.zeros((N, nu, nr), t)
        for k in range(N - 1, -1, -1):
            A, B, L = self.A[k], self.B[k], self.L[k]
            f = self.fx[nu * k:nu * k + nu]
            r = (-rw[:, nu * k:nu * k + nu].T).astype(t) + B.T @ p
            r[f, :] = 0.0
            kk[k] = -np.linalg.solve(L.T, np.linalg.solve(L, r))
            p = q[k] + A.T @ p + self.K[k].T @ r
        dw = np.zeros((nr, nu * N))
        dx = np.zeros((nx, nr))
        for k in range(N):
            du = self.K[k].astype(float) @ dx + kk[k].astype(float)
            dw[:, nu * k:nu * k + nu] = du.T
            dx = ev.A[k] @ dx + ev.B[k] @ du
        return dw


def hxu_matrix(ev, obj_factor, lam_g):
    """The part of W that comes from the state-control cross terms S_k = Hxu_k' alone."""
    _, Hxu = kr.stage_terms(ev, obj_factor, lam_g)
    nu, N = ev.prob.nu, ev.prob.N
    W = np.zeros((ev.prob.nw, ev.prob.nw))
    for k in range(1, N):
        Cx = ev.Z[k].T @ Hxu[k]
        W[:, nu * k:nu * k + nu] += Cx
        W[nu * k:nu * k + nu, :] += Cx.T
    return W


def residual_matrix(M, ev, obj_factor, lam_g, sx, delta, mutant=None):
    """The matrix of the refinement's residual rhs - M dw: M, or a mutant of it."""
    if mutant is None or mutant == "float32_residual":
        return M
    if mutant == "no_delta":      # the control diagonal's delta (the rows' delta is part of Q_k)
        return M - delta * np.eye(M.shape[0])
    if mutant == "no_Hxu":
        return M - hxu_matrix(ev, obj_factor, lam_g)
    if mutant == "no_sigma_x":
        return M - np.diag(sx)
    raise KeyError(mutant)


def refine(F, Mres, dw, rhs, free=None, mutant=None):
    """One refinement step: dw + solve(rhs - Mres dw), the residual in fp64 (float32 for the
    'float32_residual' mutant) and zero on fixed variables."""
    if mutant == "float32_residual":
        res = (rhs.astype(np.float32) - dw.astype(np.float32) @ Mres.astype(np.float32).T).astype(float)
    else:
        res = rhs - dw @ Mres.T
    if free is not None:
        res = np.where(free, res, 0.0)
    return dw + F.solve(res, np.zeros((dw.shape[0], F.ev.prob.ng)))


def steps(ev, one, inp, b, dtype=np.float32, fixed=None, mutant=None, nref=2):
    """[dw0, dw1, ...] (nr, nw) of scenario b, or None where the factorisation fails."""
    sx = inp["sigma_x"][b] if fixed is None else np.where(fixed, 0.0, inp["sigma_x"][b])
    F = Factor(ev, inp["obj_factor"], inp["lam_g"][b], sx, inp["sigma_s"][b], inp["delta"][b], dtype, fixed)
    if not F.ok:
        return None
    free = None if fixed is None else ~np.asarray(fixed, bool)
    Mres = residual_matrix(one["M"], ev, inp["obj_factor"], inp["lam_g"][b], sx, inp["delta"][b], mutant)
    out = [F.solve(inp["r_w"][b], inp["r_g"][b])]
    for _ in range(nref):
        out.append(refine(F, Mres, out[-1], one["rhs"], free, mutant))
    return out


def rhos(dws, one, free=None):
    """Per step: rho (kkt_ref.rho) of every column, (len(dws), nr); on the reduced system where
    variables are fixed."""
    M, rhs = one["M"], one["rhs"]
    if free is not None:
        M, rhs = M[np.ix_(free, free)], rhs[:, free]
        dws = [d[:, free] for d in dws]
    return np.array([[kr.rho(M, d[c], rhs[c]) for c in range(rhs.shape[0])] for d in dws])


@functools.lru_cache(maxsize=None)
def case_figures(name, regime, combo):
    """The float32 restatement on one (case, regime, combo): per scenario the rho of dw0, dw1,
    dw2 (max over columns; nan where the float32 factorisation fails), and `ok` per scenario."""
    spec, inp, per, evs = kr.reference(name, regime, combo)
    B = er.CASES[name]
    r = np.full((B, 3), np.nan)
    ok = np.zeros(B, bool)
    for b, ev in enumerate(evs):
        dws = steps(ev, per[b], inp, b)
        if dws is None:
            continue
        ok[b] = True
        r[b] = np.max(rhos(dws, per[b]), axis=1)
    return r, ok


def bounds(name, regime, combo):
    """rho0_ref, rho1_ref, rho2_ref of the case (max over scenarios) and the three bounds."""
    r, ok = case_figures(name, regime, combo)
    assert np.all(ok), (name, regime, combo, ok)
    ref = np.max(r, axis=0)
    nw = kr.reference(name, regime, combo)[0].nw
    floor = nw * EPS
    return ref, np.array([FACTOR * ref[0], max(FACTOR * ref[1], floor), max(FACTOR * ref[2], floor)])


def draw_fixed(spec, B, seed=11):
    """sigma_x = +inf on a seeded third of the controls, all of one stage's among them."""
    rng = np.random.default_rng(seed)
    nu = spec.nw // spec.N
    fx = rng.uniform(size=(B, spec.nw)) < 1.0 / 3.0
    for b in range(B):
        k = (b + 1) % spec.N
        fx[b, nu * k:nu * k + nu] = True
    return fx
