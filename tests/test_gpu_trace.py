"""The kernel's iteration trace on the first iterations against the oracle's, on every fp64
class without equality rows (A, B, C, D; both models; weights from p), with a proof that the
comparison would notice a 1e-7 error in the gradient, a constraint row, the Newton step or
the Hessian.

Tolerances come from the oracle alone (tests/golden/trace_spread.npz, gen_trace_spread.py):
30 x the largest deviation of the oracle's rounding variants from the plain oracle per field
and case; mu, delta_w (1e-12) and f (1e-10) at fixed relative figures; iteration and
line-search trial counts equal.  tests/test_oracle.py runs the same comparator on the CPU.

The fp32 classes (nlpsol option linear_solver_precision="single": A32, C32) run the same cases
against the same plain fp64 oracle.  Their tolerance is per field the larger of the fp64 one and
30 x the deviation of the oracle's refined float32 variants (a float32 Cholesky factor with one
fp64 refinement step; tests/golden/trace_spread_fp32.npz), mu and delta_w still 1e-12, counts
equal; the oracle with an UNREFINED float32 step is the reference the kernel must miss."""
import numpy as np
import pytest

from tests import trace_cases as tc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fix():
    return np.load(tc.FIXTURE)


@pytest.fixture(scope="module")
def fix32():
    return np.load(tc.FIXTURE_FP32)


_GPU = {}


def _gpu_trace(name, single=False):
    """case, per scenario (rows, chk) in oracle_trace's form, the solver's kernel_info"""
    key = (name, "single") if single else name
    if key not in _GPU:
        from nmpc_amd import nlpsol, REFERENCE_OPTS
        case = tc.build_case(name)
        spec = case["spec"]
        lbx, ubx, lbg, ubg = case["bounds"][0]
        s = nlpsol("solver", "ipopt", spec, dict(REFERENCE_OPTS, linear_solver_precision="single") if single
                   else REFERENCE_OPTS)
        s.set_trace(True)
        s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=case["P"].T)
        tr = s.read_trace(2)
        its = s.stats()["iter_count"]
        out = []
        for b in range(2):
            rows = tr[b, :tc.MAX_ITER, :8].copy()
            chk = tr[b, :tc.MAX_ITER + 1, 8:12].copy()
            n = min(int(its[b]), tc.MAX_ITER)
            rows[n:] = np.nan
            chk[n + 1:] = np.nan
            out.append((rows, chk))
        _GPU[key] = (case, out, s.kernel_info())
    return _GPU[key]


@pytest.mark.parametrize("name", tc.GATED)
def test_first_iterations_match_the_oracle_within_its_rounding_spread(fix, name):
    _, traces, _ = _gpu_trace(name)
    bad = []
    for b, (rows, chk) in enumerate(traces):
        lead, ratios = tc.compare(fix, name, b, rows, chk)
        print(f"{name}/{b}: {lead} iterations; deviation / tolerance " +
              ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        bad += [(b, k, v) for k, v in ratios.items() if not v <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("name", tc.GATED)
def test_a_1e7_error_in_the_oracle_fails_the_comparison(fix, name):
    """The GPU trace against a deliberately wrong oracle (1e-7 relative in the stage-cost
    gradient, one obstacle row's gradient, the Newton step, the stage-cost Hessian): each must
    miss the tolerance on some field of the case by at least 10 x."""
    case, traces, _ = _gpu_trace(name)
    for mut in tc.MUTATIONS:
        if not tc.applies(mut, case):
            continue
        worst = {}
        for b, (rows, chk) in enumerate(traces):
            ratios = tc.compare(fix, name, b, rows, chk, ref=tc.mutated_trace(name, case, b, mut))[1]
            f = max(ratios, key=ratios.get)
            worst[b] = (f, ratios[f])
        print(f"{name} {mut}: {worst}")
        assert max(r for _, r in worst.values()) >= tc.MARGIN, (mut, worst)


@pytest.mark.parametrize("name", tc.GATED)
def test_fp32_first_iterations_match_the_oracle_within_the_refined_float32_spread(fix, fix32, name):
    """linear_solver_precision="single" at REFERENCE_OPTS: the kernel's trace against the plain
    fp64 oracle within the fp32 tolerance, iteration and trial counts equal on the leading
    iterations.  Measured on an MI355X: DESIGN.md 'fp32 leg: what is tested'."""
    _, traces, _ = _gpu_trace(name, single=True)
    bad = []
    for b, (rows, chk) in enumerate(traces):
        lead, ratios = tc.compare(fix, name, b, rows, chk, fix32=fix32)
        print(f"{name}/{b} fp32: {lead} iterations; deviation / tolerance " +
              ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
        assert lead >= tc.FP32_MIN_LEAD
        bad += [(b, k, v) for k, v in ratios.items() if not v <= 1.0]
    assert not bad, bad


@pytest.mark.parametrize("name", tc.GATED)
def test_fp32_trace_misses_the_unrefined_float32_oracle(fix, fix32, name):
    """The fp32 kernel's trace against the oracle whose Newton step is the float32 factor's with
    NO refinement: it must miss the fp32 tolerance on some field of the case by at least 10 x --
    the kernel refines, and the comparison can tell."""
    case, traces, _ = _gpu_trace(name, single=True)
    worst = {}
    for b, (rows, chk) in enumerate(traces):
        ratios = tc.compare(fix, name, b, rows, chk, ref=tc.unrefined_trace(name, case, b), fix32=fix32)[1]
        f = max(ratios, key=ratios.get)
        worst[b] = (f, ratios[f])
    print(f"{name} fp32 kernel against the unrefined float32 oracle: {worst}")
    assert max(r for _, r in worst.values()) >= tc.MARGIN, worst


def test_the_cases_run_the_intended_kernel_classes():
    """As far as the API tells: nmpc_kernel_info's LDS size is the class's layout size, so all
    class-A cases report one size and the A, B, C and D cases four different ones.  With
    linear_solver_precision="single" there are two sizes: A32 for the cases of class A (at most
    a quarter CU as well) and C32 for every other one, each different from its fp64 counterpart
    (the refinement classes keep a state step more in LDS, and A32 its trial rows in global
    memory)."""
    lds = {n: _gpu_trace(n)[2]["lds_bytes"] for n in tc.GATED}
    print(lds)
    by_class = {}
    for n, c in tc.CLASS_OF.items():
        by_class.setdefault(c, set()).add(lds[n])
    assert all(len(v) == 1 for v in by_class.values()), by_class
    assert len({next(iter(v)) for v in by_class.values()}) == 4, by_class
    a64 = by_class["A"].pop()
    assert a64 <= 40960  # the LDS-row class: a quarter CU
    lds32 = {n: _gpu_trace(n, single=True)[2]["lds_bytes"] for n in tc.GATED}
    print(lds32)
    by32 = {}
    for n, c in tc.CLASS_OF.items():
        by32.setdefault("A32" if c == "A" else "C32", set()).add(lds32[n])
    assert all(len(v) == 1 for v in by32.values()), by32
    a32, c32 = by32["A32"].pop(), by32["C32"].pop()
    assert a32 != c32 and a32 <= 40960
    assert a32 != a64 and c32 != by_class["C"].pop(), (a32, a64, c32)


def test_start_over_the_target_is_invalid_number_and_neighbours_are_unaffected():
    """A start exactly over the target (p[8:10] == p[0:2]): the distance term has no gradient
    (0 / 0) and the oracle stops with Invalid_Number_Detected (-13) at iteration 0.  The kernel
    must report the same status and iteration count, and the two ordinary scenarios batched
    around it must give what they give without it."""
    from nmpc_amd import nlpsol, make_spec, draw_scenarios, REFERENCE_OPTS
    from oracle import nmpc_oracle as orc

    spec = make_spec("race_track_2", N=8, T=0.2)
    P = draw_scenarios(spec, 3, seed=7)
    P[1, 8:10] = P[1, 0:2]
    lbx, ubx, lbg, ubg = spec.bounds()
    prob = orc.make_problem("race_track_2", N=8, T=0.2)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    sol = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    st, its = np.array(s.stats()["status_code"]), np.array(s.stats()["iter_count"])
    x_batch = sol["x"].copy()
    refs = []
    for b in range(3):
        with np.errstate(all="ignore"):  # the oracle's own 0 / 0 at scenario 1
            refs.append(orc.IpoptDense(prob, orc.REFERENCE_OPTS).solve(np.zeros(spec.nw), lbx, ubx, lbg, ubg, P[b]))
    print("GPU", list(st), list(its), "oracle", [(r["status"], r["iter"]) for r in refs])
    assert refs[1]["status"] == orc.INVALID_NUMBER_DETECTED and refs[1]["iter"] == 0
    assert int(st[1]) == orc.INVALID_NUMBER_DETECTED and int(its[1]) == 0
    for b in (0, 2):
        assert refs[b]["status"] == orc.SOLVE_SUCCEEDED and int(st[b]) == refs[b]["status"]
        err = np.max(np.abs(sol["x"][:, b] - refs[b]["x"]) / (1.0 + np.abs(refs[b]["x"])))
        assert err <= 1e-6, (b, err)
    sol2 = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P[[0, 2]].T)
    np.testing.assert_array_equal(sol2["x"], x_batch[:, [0, 2]])
