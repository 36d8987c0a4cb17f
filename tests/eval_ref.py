"""Checker side of the evaluation / KKT-certificate tests (tests/test_gpu_eval.py): the
oracle's function layer (oracle.nmpc_oracle.SSEval) at a given point, the five certificate
numbers restated from tests/test_gpu_reference_runs.py::test_reference_run_kkt_certificate
(unnormalised), the cases, and the tolerances.

Tolerance 1e-10: a one-ulp change of w and p moves SSEval's F, g, X, grad F and
grad F + J' lam by at most 2e-13 relative to the scales below (measured on the CPU on five
shapes up to N = 63), so 1e-10 leaves 500x for a different operation order and is still
1,000x below the 1e-7 errors the trace tests are built to catch."""
from __future__ import annotations

import functools

import numpy as np

TOL = 1e-10
NOBOUND = 1e19  # |b| >= 1e19: no bound (include/nmpc_amd.h)


def problem_of(spec):
    """oracle Problem with exactly the spec's data (any obstacle table, weights in p, model)."""
    from oracle import nmpc_oracle as orc

    ob = spec.obstacles
    return orc.Problem(N=spec.N, T=spec.T, obs_x=[o.x for o in ob], obs_y=[o.y for o in ob],
                       obs_rsum=[o.r for o in ob], obs_x_pidx=[o.x_pidx for o in ob],
                       obs_y_pidx=[o.y_pidx for o in ob], w1=spec.w1, w2=spec.w2, vfov=spec.vfov, hfov=spec.hfov,
                       np_=spec.np, w1_pidx=spec.w1_pidx, w2_pidx=spec.w2_pidx, model=spec.model)


def case_spec(name):
    from nmpc_amd import make_spec
    from nmpc_amd.spec import Obstacle

    if name == "race_track_2":
        return make_spec("race_track_2", N=6, T=0.2)
    if name == "nmpc_tt":
        return make_spec("nmpc_tt", N=15, T=1.0)   # gradients ~1e3
    if name == "n63_16obs":  # every lane, every row slot
        obs = tuple(Obstacle(-300.0 + 700.0 * (j % 4), -200.0 + 450.0 * (j // 4), 35.0 + j) for j in range(16))
        return make_spec(None, N=63, T=0.2, obstacles=obs)
    if name == "n1":
        return make_spec("race_track_2", N=1, T=0.2)
    if name == "dynamic":
        return make_spec("dynamic", N=12, T=0.2, dynamic=True)
    if name == "weights_in_p":
        return make_spec("race_track_2", N=6, T=0.2, weights_in_p=True)
    if name == "uav5":
        return make_spec("nmpc_tt", N=5, T=0.2, model="uav5")
    raise KeyError(name)


CASES = {"race_track_2": 8, "nmpc_tt": 4, "n63_16obs": 3, "n1": 2, "dynamic": 3, "weights_in_p": 3, "uav5": 3}


def draw_point(spec, B, seed):
    """w ~ U(lbx, ubx), lam_g ~ 10 N(0,1), lam_x ~ N(0,1), p from draw_scenarios (cost weights
    taken from p: w1 ~ U(0.5, 2), w2 ~ U(1, 3))."""
    from nmpc_amd import draw_scenarios

    rng = np.random.default_rng(seed)
    lbx, ubx, lbg, ubg = spec.bounds()
    P = draw_scenarios(spec, B, seed=seed + 1)
    if spec.w1_pidx >= 0:
        P[:, spec.w1_pidx] = rng.uniform(0.5, 2.0, B)
        P[:, spec.w2_pidx] = rng.uniform(1.0, 3.0, B)
    w = rng.uniform(lbx, ubx, (B, spec.nw))
    lg = 10.0 * rng.standard_normal((B, spec.ng))
    lx = rng.standard_normal((B, spec.nw))
    return {"w": w, "p": P, "lam_g": lg, "lam_x": lx, "lbx": lbx, "ubx": ubx, "lbg": lbg, "ubg": ubg}


def cpu_kkt(gradF, JT_lg, g, x, lg, lx, lbx, ubx, lbg, ubg):
    """[stat, gmax, viol, compl, lmax] of tests/test_gpu_reference_runs.py:355-372, unnormalised,
    a bound being present where |b| < 1e19."""
    stat = float(np.max(np.abs(gradF + JT_lg + lx)))
    gmax = float(np.max(np.abs(gradF)))

    def over(v, lo, hi):
        up = np.where(np.abs(hi) < NOBOUND, v - hi, -np.inf)
        dn = np.where(np.abs(lo) < NOBOUND, lo - v, -np.inf)
        return max(float(np.max(up, initial=0.0)), float(np.max(dn, initial=0.0)))

    def cpl(lam, v, lo, hi):
        up = np.where(lam > 0, lam * np.where(np.abs(hi) < NOBOUND, hi - v, 0.0), 0.0)
        dn = np.where(lam < 0, -lam * np.where(np.abs(lo) < NOBOUND, v - lo, 0.0), 0.0)
        return float(max(np.max(np.abs(up), initial=0.0), np.max(np.abs(dn), initial=0.0)))

    with np.errstate(invalid="ignore"):
        viol = max(over(g, lbg, ubg), over(x, lbx, ubx), 0.0)
        compl = max(cpl(lg, g, lbg, ubg), cpl(lx, x, lbx, ubx))
    lmax = max(float(np.max(np.abs(lg), initial=0.0)), float(np.max(np.abs(lx), initial=0.0)))
    return np.array([stat, gmax, viol, compl, lmax])


def cpu_eval(prob, w, p, lg, lx, lbx, ubx, lbg, ubg):
    """One scenario on the oracle: f, g, X, grad_f, grad_l, kkt and the scales of the tolerances."""
    from oracle import nmpc_oracle as orc

    ev = orc.SSEval(prob, w, p)
    JT = ev.J.T @ lg
    finite = [np.abs(b)[np.abs(b) < NOBOUND] for b in (lbx, ubx, lbg, ubg)]
    S = max([float(np.max(np.abs(ev.g))), float(np.max(np.abs(w)))] + [float(np.max(b)) for b in finite if b.size])
    return {"f": ev.F, "g": ev.g, "X": ev.X.T.reshape(-1), "grad_f": ev.gradF, "grad_l": ev.gradF + JT + lx,
            "kkt": cpu_kkt(ev.gradF, JT, ev.g, w, lg, lx, lbx, ubx, lbg, ubg),
            "gscale": float(np.max(np.abs(ev.gradF))),
            "lscale": 1.0 + float(np.max(np.abs(ev.gradF))) + float(np.max(np.abs(JT))) + float(np.max(np.abs(lx))),
            "S": S}


@functools.lru_cache(maxsize=None)
def reference(name, seed=2024):
    """(spec, inputs, per-scenario oracle results) of a case, computed once and shared."""
    spec = case_spec(name)
    prob = problem_of(spec)
    d = draw_point(spec, CASES[name], seed)
    ref = [cpu_eval(prob, d["w"][b], d["p"][b], d["lam_g"][b], d["lam_x"][b], d["lbx"], d["ubx"], d["lbg"], d["ubg"])
           for b in range(CASES[name])]
    return spec, d, ref


def check_against(got, ref, b, what=""):
    """got: one scenario's f, g, X, grad_f, grad_l, kkt; ref: cpu_eval's dict.  Prints every
    figure relative to its bound before asserting, returns them."""
    fig = {}
    for k in ("f", "g", "X"):
        a, r = np.asarray(got[k], float).reshape(-1), np.asarray(ref[k], float).reshape(-1)
        fig[k] = float(np.max(np.abs(a - r) / (TOL * (1 + np.abs(r)))))
    fig["grad_f"] = (float(np.max(np.abs(got["grad_f"] - ref["grad_f"]))) / (TOL * ref["gscale"])
                     if ref["gscale"] > 0 else float(np.max(np.abs(got["grad_f"]))))
    fig["grad_l"] = float(np.max(np.abs(got["grad_l"] - ref["grad_l"]))) / (TOL * ref["lscale"])
    if got.get("kkt") is not None:
        kg, kr = np.asarray(got["kkt"], float), ref["kkt"]
        fig["stat"] = abs(kg[0] - kr[0]) / (TOL * ref["lscale"])
        fig["gmax"] = abs(kg[1] - kr[1]) / (TOL * kr[1]) if kr[1] > 0 else abs(kg[1])
        fig["viol"] = abs(kg[2] - kr[2]) / (TOL * (1 + ref["S"]))
        fig["compl"] = abs(kg[3] - kr[3]) / (TOL * (1 + kr[4]) * (1 + ref["S"]))
        fig["lmax"] = abs(kg[4] - kr[4]) / (TOL * kr[4]) if kr[4] > 0 else abs(kg[4])
    print(f"{what} scenario {b}: error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= 1.0}
    assert not bad, (what, b, bad)
    return fig
