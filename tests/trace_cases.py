"""Shared by tests/golden/gen_trace_spread.py, tests/test_oracle.py and tests/test_gpu_trace.py:
the cases of the first-iterations trace comparison, the comparator, and the deliberately wrong
oracles of the sensitivity test.  (Helper module, no tests.)

A case is a problem shape that runs one fp64 kernel class / model, with two scenarios, cold
start at zero.  The fixture (tests/golden/trace_spread.npz) holds, per case and scenario, the
plain oracle's trace of the first MAX_ITER iterations, the largest deviation of the oracle's
rounding variants (la_variant 1..3) from it per field, and the number of leading iterations
on which every variant takes the same line-search trial counts.  Nothing in it comes from the
kernel."""
import contextlib
import os

import numpy as np

from oracle import nmpc_oracle as orc

MAX_ITER = 8
# reference-side rounding variants, (la_variant, evaluation variant): the Newton step from a
# permuted Cholesky factorisation (oracle _Chol), and the objective from the literal form of
# the stage cost summed in reverse stage order (eval_variant below) instead of the derivative
# routine's algebraically equal form summed forward.  The kernel differs from the plain
# oracle in both ways (Riccati step; literal stage cost, butterfly sums).
VARIANTS = ((1, 0), (2, 0), (3, 0), (0, 1), (1, 1))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace_spread.npz")
# the fp32 leg (nlpsol option linear_solver_precision="single"; kernel classes A32, C32): the
# Newton step from a float32 Cholesky factor with one fp64 refinement step (oracle _Chol
# variants 4..7: identity and the three permutations), also crossed with evaluation variant 1.
# tests/golden/trace_spread_fp32.npz holds, per GATED case, their largest deviation from the
# plain fp64 oracle per field and, per scenario, the leading iterations on which all of them
# take the plain oracle's iteration and trial counts.  (la_variant 8, 0): the float32 factor
# with NO refinement, the deliberately wrong reference of the fp32 tests.
FP32_VARIANTS = ((4, 0), (5, 0), (6, 0), (7, 0), (4, 1))
FP32_UNREFINED = (8, 0)
FIXTURE_FP32 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trace_spread_fp32.npz")
FP32_MIN_LEAD = 4

# trace row fields (include/nmpc_amd.h: columns 1..6 of a trace row) and the convergence
# check's (columns 8..11 of the row of the same iteration count)
ROW_FIELDS = ("mu", "f", "theta", "delta", "alpha_p", "alpha_d")
CHK_FIELDS = ("err", "dinf", "cviol", "cmp")
FIELDS = ROW_FIELDS + CHK_FIELDS
# fixed relative figures: mu and delta_w 1e-12, f 1e-10 (tests/test_gpu.py's figures for its trace
# test).  f is not held to the variants' spread: they leave its evaluation untouched, so their
# f agrees to ~1e-16 and says nothing about another evaluation order.
FIXED_REL = {"mu": 1e-12, "delta": 1e-12, "f": 1e-10}
ABS_BELOW = ("theta",) + CHK_FIELDS  # fields compared absolutely where the value is below 1e-6
SMALL = 1e-6
FACTOR = 30.0                      # x the stored variant deviation
MUTATION = 1e-7

# name -> (layout, N, T, keyword arguments, what it is there for)
CASES = {
    "rt2_n8": ("race_track_2", 8, 0.2, {}, "class A"),
    "rt2_n20": ("race_track_2", 20, 0.2, {}, "class A, its capacity"),
    "tt_n15": ("nmpc_tt", 15, 1.0, {}, "class A, NLP scaling active"),
    "obs10_n15": ("10_obstacles", 15, 0.2, {}, "class A, far-away obstacle rows"),
    "rt2_n25": ("race_track_2", 25, 0.2, {}, "class B"),
    "obs11_n40": ("race_track_2", 40, 0.2, {"extra_obstacle": True}, "class C (16 rows per stage)"),
    "dyn_n50": ("dynamic", 50, 0.2, {"dynamic": True}, "class D, obstacle coordinates from p"),
    "uav5_n10": ("race_track_2", 10, 0.2, {"model": "uav5"}, "no-gimbal model"),
    "weights_n10": ("race_track_2", 10, 0.2, {"weights": True}, "cost weights from p"),
    "pinned_n8": ("race_track_2", 8, 0.2, {"pinned": True}, "class E (equality row)"),
}
EXTRA_OBSTACLE = (750.0, 500.0, 55.0)  # x, y, UAV_r + r: an 11th obstacle, so m = 16 > class D's 15
WEIGHTS = np.array([[0.5, 3.0], [2.0, 0.5]])
# The equality-row case is in the fixture but not in the GPU gate: the oracle's equality step
# does not go through _Chol, so la_variant 1..3 are bitwise the plain oracle there and every
# stored deviation but f's is exactly zero.
GATED = tuple(n for n in CASES if n != "pinned_n8")
# cases whose kernel class the tests tell apart through nmpc_kernel_info's LDS size
CLASS_OF = {"rt2_n8": "A", "rt2_n20": "A", "tt_n15": "A", "obs10_n15": "A", "uav5_n10": "A", "weights_n10": "A",
            "rt2_n25": "B", "obs11_n40": "C", "dyn_n50": "D"}


def build_case(name):
    """-> dict(prob, spec, P (2, np), bounds: one (lbx, ubx, lbg, ubg) per scenario)."""
    from nmpc_amd import make_spec, draw_scenarios
    from nmpc_amd.spec import LAYOUTS, UAV_R, Obstacle
    layout, N, T, kw, _ = CASES[name]
    model, dyn = kw.get("model", "uav8g"), kw.get("dynamic", False)
    if kw.get("pinned"):
        from tests.test_oracle import _pinned_z_problem
        prob = orc.make_problem(layout, N=N, T=T)
        cases = [_pinned_z_problem(b) for b in (0, 1)]
        return dict(prob=prob, spec=make_spec(layout, N=N, T=T), P=np.stack([c[1] for c in cases]),
                    bounds=[tuple(c[2:6]) for c in cases])
    prob = orc.make_problem(layout, N=N, T=T, dynamic=dyn, model=model)
    base = make_spec(layout, N=N, T=T, dynamic=dyn, model=model)
    spec = make_spec(layout, N=N, T=T, dynamic=dyn, model=model, weights_in_p=kw.get("weights", False))
    if kw.get("extra_obstacle"):
        xy, r = LAYOUTS[layout]
        ex, ey, er = EXTRA_OBSTACLE
        obs = tuple(Obstacle(float(x), float(y), UAV_R + r) for x, y in xy) + (Obstacle(ex, ey, er),)
        base = spec = make_spec(None, N=N, T=T, obstacles=obs)
        prob = orc.Problem(N=N, T=T, obs_x=[o.x for o in obs], obs_y=[o.y for o in obs],
                           obs_rsum=[o.r for o in obs])
    P = draw_scenarios(base, 2, seed=1003)
    if kw.get("weights"):
        P = np.hstack([P, WEIGHTS])
        prob.w1_pidx, prob.w2_pidx, prob.np_ = P.shape[1] - 2, P.shape[1] - 1, P.shape[1]
    return dict(prob=prob, spec=spec, P=P, bounds=[tuple(spec.bounds())] * 2)


@contextlib.contextmanager
def eval_variant(on=True):
    """The oracle with its function values evaluated another way (same functions, different
    rounding): the objective from orc.stage_cost's literal form per stage, the stages summed
    last to first, and the obstacle rows' distance by hypot."""
    if not on:
        yield
        return
    base = orc.SSEval

    class SSEvalLiteral(base):
        def __init__(self, prob, w, p):
            super().__init__(prob, w, p)
            q, ti = self.prob, self.prob.target_index
            self.F = sum(orc.stage_cost(q, self.X[:, k], self.p[ti], self.p[ti + 1]) for k in reversed(range(q.N)))

    rows0 = orc.stage_rows

    def stage_rows_hypot(prob, xk, ox, oy):  # the obstacle distance by hypot instead of sqrt(dx^2 + dy^2)
        return np.concatenate([xk[prob.box_states], -np.hypot(xk[0] - ox, xk[1] - oy) + prob.obs_rsum])

    orc.SSEval, orc.stage_rows = SSEvalLiteral, stage_rows_hypot
    try:
        yield
    finally:
        orc.SSEval, orc.stage_rows = base, rows0


def oracle_trace(case, b, variant=(0, 0)):
    """The oracle's first MAX_ITER iterations of scenario b: (rows (MAX_ITER, 8) in the kernel's
    column order, NaN past the end or from the first restoration iteration on; chk
    (MAX_ITER + 1, 4), NaN likewise; status; iterations)."""
    with eval_variant(bool(variant[1])):
        return _oracle_trace(case, b, variant[0])


def _oracle_trace(case, b, la_variant):
    ipo = orc.IpoptDense(case["prob"], dict(orc.REFERENCE_OPTS, max_iter=MAX_ITER), la_variant=la_variant)
    lbx, ubx, lbg, ubg = case["bounds"][b]
    r = ipo.solve(np.zeros(case["prob"].nw), lbx, ubx, lbg, ubg, case["P"][b], trace=True)
    rows = np.full((MAX_ITER, 8), np.nan)
    for k, t in enumerate(r["trace"][:MAX_ITER]):
        if t.get("resto") or t["iter"] != k + 1:
            break
        rows[k] = [t["iter"], t["mu"], t["f"], t["theta"], t["delta"], t["alpha_p"], t["alpha_d"], t["ls"]]
    n = int(np.sum(np.isfinite(rows[:, 0])))
    chk = np.full((MAX_ITER + 1, 4), np.nan)
    for c in ipo.chk:
        if c["it"] <= n and c["err"] >= 0 and np.isnan(chk[c["it"], 0]):
            chk[c["it"]] = [c[k] for k in CHK_FIELDS]
    return rows, chk, int(r["status"]), int(r["iter"])


def field_values(rows, chk, lead):
    """field -> the values compared on `lead` leading iterations: a row field on rows
    0..lead-1, a check field at the iteration counts 0..lead."""
    out = {f: rows[:lead, 1 + i] for i, f in enumerate(ROW_FIELDS)}
    out.update({f: chk[:lead + 1, i] for i, f in enumerate(CHK_FIELDS)})
    return out


def compare(fix, name, b, rows, chk, ref=None, fix32=None):
    """Compare a trace (rows, chk as oracle_trace returns them) with the fixture's plain
    oracle -- or with `ref` = (rows, chk) of another reference, e.g. a deliberately wrong
    oracle -- under the fixture's tolerances.  -> (lead, {field: worst deviation / tolerance});
    iter / ls mismatches are reported as field 'ls' with ratio inf.  mu, delta and f: the
    fixed figures of FIXED_REL.  Every other field: FACTOR x the variants' largest relative
    deviation on the case, or, for theta and the check fields where the reference value is
    below SMALL, FACTOR x their largest absolute deviation.
    fix32 (the fp32 fixture): the fp32 leg's comparison -- per field the larger of that
    tolerance and FACTOR x the refined float32 variants' deviation (f: the larger of its fixed
    figure and that; mu and delta keep their fixed 1e-12), on the leading iterations both
    fixtures vouch for."""
    key = f"{name}__{b}"
    lead = int(fix[key + "__lead"])
    if fix32 is not None:
        lead = min(lead, int(fix32[key + "__lead"]))
    prow, pchk = (fix[key + "__rows"], fix[key + "__chk"]) if ref is None else ref
    ratios = {}
    same = np.array_equal(rows[:lead, 0], prow[:lead, 0]) and np.array_equal(rows[:lead, 7], prow[:lead, 7])
    ratios["ls"] = 0.0 if same else np.inf
    want, got = field_values(prow, pchk, lead), field_values(rows, chk, lead)
    for i, f in enumerate(FIELDS):
        ref, g = want[f], got[f]
        if np.any(np.isnan(g) != np.isnan(ref)):
            ratios[f] = np.inf
            continue
        ok = ~np.isnan(ref)
        ref, g = ref[ok], g[ok]
        if f in FIXED_REL:
            tol = FIXED_REL[f] * np.abs(ref)
            if fix32 is not None and f == "f":  # the step's error reaches f: the larger of the two
                tol = max(FIXED_REL[f], FACTOR * fix32[name + "__dev_rel"][i]) * np.abs(ref)
        else:
            dev_rel, dev_abs = fix[name + "__dev_rel"][i], fix[name + "__dev_abs"][i]
            if fix32 is not None:
                dev_rel, dev_abs = max(dev_rel, fix32[name + "__dev_rel"][i]), max(dev_abs, fix32[name + "__dev_abs"][i])
            tol = FACTOR * dev_rel * np.abs(ref)
            if f in ABS_BELOW:
                tol = np.where(np.abs(ref) < SMALL, FACTOR * dev_abs, tol)
        d = np.abs(g - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d == 0, 0.0, d / tol)
        ratios[f] = float(np.max(r)) if r.size else 0.0
    return lead, ratios


def spread(plain, variants):
    """Per field: the variants' largest absolute deviation over the values below SMALL (theta
    and the check fields) and largest relative deviation over the others, on `lead` leading
    iterations (-> lead, dev_abs, dev_rel).  lead: the leading iterations every variant and
    the plain oracle ran in the main phase with equal iteration and trial counts."""
    prow, pchk = plain
    lead = 0
    for k in range(MAX_ITER):
        if np.isnan(prow[k, 0]) or any(np.isnan(v[0][k, 0]) or v[0][k, 0] != prow[k, 0] or v[0][k, 7] != prow[k, 7]
                                       for v in variants):
            break
        lead = k + 1
    dev_abs, dev_rel = np.zeros(len(FIELDS)), np.zeros(len(FIELDS))
    want = field_values(prow, pchk, lead)
    for vrow, vchk in variants:
        got = field_values(vrow, vchk, lead)
        for i, f in enumerate(FIELDS):
            ref, g = want[f], got[f]
            ok = ~np.isnan(ref)
            assert not np.any(np.isnan(g[ok])), (f, ref, g)
            ref, g = ref[ok], g[ok]
            small = (np.abs(ref) < SMALL) if f in ABS_BELOW else np.zeros(ref.shape, bool)
            d = np.abs(g - ref)
            if np.any(small):
                dev_abs[i] = max(dev_abs[i], float(np.max(d[small])))
            if np.any(~small):
                nz = ~small & (ref != 0)
                assert np.all(d[~small & (ref == 0)] == 0)
                if np.any(nz):
                    dev_rel[i] = max(dev_rel[i], float(np.max(d[nz] / np.abs(ref[nz]))))
    return lead, dev_abs, dev_rel


# ---------------------------------------------------------------- the wrong oracles
def _mut_cost_gradient(f):
    def g(prob, xk, xt, yt):
        v, gr, H = f(prob, xk, xt, yt)
        return v, gr * (1.0 + MUTATION), H
    return g


def _mut_cost_hessian(f):
    def g(prob, xk, xt, yt):
        v, gr, H = f(prob, xk, xt, yt)
        return v, gr, H * (1.0 + MUTATION)
    return g


def _mut_obstacle_row(f):
    def g(xk, ox, oy):
        G, H = f(xk, ox, oy)
        G = G.copy()
        G[0] *= 1.0 + MUTATION
        return G, H
    return g


def _mut_newton_step(f):
    def g(self, b):
        return f(self, b) * (1.0 + MUTATION)
    return g


# name -> (object, attribute, wrapper, needs obstacles)
MUTATIONS = {
    "cost_gradient": (orc, "_stage_cost_derivs8", _mut_cost_gradient, False),
    "obstacle_row": (orc, "obstacle_derivs", _mut_obstacle_row, True),
    "newton_step": (orc._Chol, "solve", _mut_newton_step, False),
    # the stage-cost Hessian separates from the variant spread by the same margin
    "cost_hessian": (orc, "_stage_cost_derivs8", _mut_cost_hessian, False),
}
EXTRA_MUTATIONS = {}
MARGIN = 10.0  # a mutation must miss the tolerance by this factor on some field of the case


@contextlib.contextmanager
def mutated(name):
    obj, attr, wrap, _ = {**MUTATIONS, **EXTRA_MUTATIONS}[name]
    orig = getattr(obj, attr)
    setattr(obj, attr, wrap(orig))
    try:
        yield
    finally:
        setattr(obj, attr, orig)


def applies(mutation, case):
    return not {**MUTATIONS, **EXTRA_MUTATIONS}[mutation][3] or case["prob"].n_obs > 0


_MUT_CACHE = {}


def unrefined_trace(name, case, b):
    """(rows, chk) of the oracle whose Newton step is the float32 factor's, unrefined."""
    k = (name, b, "unrefined32")
    if k not in _MUT_CACHE:
        _MUT_CACHE[k] = oracle_trace(case, b, FP32_UNREFINED)[:2]
    return _MUT_CACHE[k]


def mutated_trace(name, case, b, mutation):
    """(rows, chk) of the oracle with `mutation` applied (computed once per process)."""
    k = (name, b, mutation)
    if k not in _MUT_CACHE:
        with mutated(mutation):
            _MUT_CACHE[k] = oracle_trace(case, b)[:2]
    return _MUT_CACHE[k]
