"""The solver's device primitives (nmpc_solve.hip: wsum / wmax / wmin, readlane_d, LogAcc,
rcp, rsq, qd), each against a plain host reference in higher precision.

The probe (tests/probe/nmpc_probe.hip) #includes the product's kernel source and is compiled
with the product's flags, so the functions under test are the solver's own text.  References:
exact rational arithmetic (fractions.Fraction) for sums, mpmath at 120 bits (the standard
library's decimal at 50 digits where mpmath is not installed) for reciprocals, logarithms
and square roots, and numpy's IEEE quotient for qd (correctly rounded and
independent of the device compiler).  Every bound comes from the operation's own rounding
analysis (stated at the test), none from what the kernel returns."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53

# high-precision scalars: _hp(float) converts exactly; +, -, /, abs and float() work on both kinds
try:
    import mpmath

    mpmath.mp.prec = 120
    _hp, _hp_log, _hp_sqrt = (lambda v: mpmath.mpf(float(v))), mpmath.log, mpmath.sqrt
except ImportError:  # the standard library's arbitrary-precision decimal, correctly rounded ln / sqrt
    import decimal

    _CTX = decimal.Context(prec=50)
    _hp = lambda v: _CTX.create_decimal(decimal.Decimal(float(v)))  # noqa: E731
    _hp_log, _hp_sqrt = (lambda d: _CTX.ln(d)), (lambda d: _CTX.sqrt(d))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


@pytest.fixture(scope="module")
def probe():
    from tests.probe import build
    return build.lib()


def _wreduce(probe, op, cases):
    cases = np.ascontiguousarray(cases, dtype=np.float64).reshape(-1, 64)
    out = np.full_like(cases, 12345.0)
    assert probe.nmpc_probe_wreduce(op, cases.shape[0], _dp(cases), _dp(out)) == 0
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _lanes_identical(out):
    b = _bits(out)
    return bool(np.all(b == b[:, :1]))


# ------------------------------------------------------------------ wsum
def test_wsum_accuracy_and_lane_agreement(probe):
    """|wsum - exact| <= 6 * 2^-53 * sum |v_i|: six butterfly levels, each adding one rounding
    of a partial sum bounded by sum |v_i| (first order).  All 64 lanes bitwise identical."""
    rng = np.random.default_rng(11)
    cases = [rng.standard_normal(64) for _ in range(8)]
    for _ in range(8):  # magnitudes over 1e+-30, with cancellation: pairs (v, -v (1 + eps))
        v = rng.standard_normal(32) * 10.0 ** rng.uniform(-30, 30, 32)
        w = -v * (1.0 + rng.uniform(-1e-9, 1e-9, 32))
        cases.append(rng.permutation(np.concatenate([v, w])))
    ints = [rng.integers(-1000, 1000, 64).astype(float) for _ in range(4)]
    out = _wreduce(probe, 0, cases + ints)
    assert _lanes_identical(out)
    worst = 0.0
    for c, o in zip(cases + ints, out):
        exact = sum(Fraction(float(x)) for x in c)
        bound = 6 * Fraction(U) * sum(abs(Fraction(float(x))) for x in c)
        err = abs(Fraction(float(o[0])) - exact)
        worst = max(worst, float(err / bound)) if bound else worst
        assert err <= bound, (float(err), float(bound))
    print(f"wsum: largest error / bound = {worst:.3f}")
    for c, o in zip(ints, out[len(cases):]):  # exact sums
        assert o[0] == float(np.sum(c.astype(np.int64)))


def test_wsum_single_nonzero_lane_is_returned_exactly(probe):
    # a wrong DPP control or a dropped row loses (or doubles) some lane's value
    rng = np.random.default_rng(12)
    vals = rng.standard_normal(64) * 10.0 ** rng.uniform(-200, 200, 64)
    out = _wreduce(probe, 0, np.diag(vals))
    assert _lanes_identical(out)
    np.testing.assert_array_equal(_bits(out[:, 0]), _bits(vals))


def test_wsum_propagates_nan_and_inf(probe):
    rng = np.random.default_rng(13)
    base = rng.standard_normal((64, 64))
    base[np.arange(64), np.arange(64)] = np.nan  # a NaN at each position
    out = _wreduce(probe, 0, base)
    assert np.all(np.isnan(out))
    c = rng.standard_normal((3, 64))
    c[0, 5], c[0, 40] = np.inf, -np.inf  # different halves
    c[1, 17], c[1, 18] = -np.inf, np.inf  # neighbours
    c[2, 63] = np.inf
    out = _wreduce(probe, 0, c)
    assert np.all(np.isnan(out[:2]))
    assert np.all(out[2] == np.inf)


# ------------------------------------------------------------------ wmax / wmin
@pytest.mark.parametrize("op,hostf,sign", [(1, np.fmax, 1.0), (2, np.fmin, -1.0)])
def test_wmax_wmin_equal_the_host_extremum(probe, op, hostf, sign):
    """Exact equality with the host's max / min; the extremum at each position; +-inf; a NaN
    lane is ignored (C fmax / fmin: the callers test non-finite values with a separate
    wany(bad)); all lanes identical."""
    rng = np.random.default_rng(20 + op)
    cases = []
    for pos in range(64):  # the extremum at each position
        c = rng.standard_normal(64)
        c[pos] = sign * 10.0
        cases.append(c)
    for pos in range(64):  # a NaN at each position, the extremum next to it
        c = rng.standard_normal(64) * 10.0 ** rng.uniform(-100, 100, 64)
        c[pos] = np.nan
        c[(pos + 1) % 64] = sign * 1e300
        cases.append(c)
    c = rng.standard_normal(64); c[9] = np.inf; cases.append(c)
    c = rng.standard_normal(64); c[50] = -np.inf; cases.append(c)
    c = rng.standard_normal(64); c[3] = np.inf; c[35] = -np.inf; c[20] = np.nan; cases.append(c)
    c = np.full(64, -np.inf); c[31] = -1e308; cases.append(c)
    c = np.full(64, np.inf); c[32] = 1e308; cases.append(c)
    cases.append(rng.standard_normal(64) * 5e-324 * 1000)  # denormals
    cases = np.array(cases)
    out = _wreduce(probe, op, cases)
    assert _lanes_identical(out)
    want = hostf.reduce(cases, axis=1)
    assert not np.any(np.isnan(want))
    np.testing.assert_array_equal(_bits(out[:, 0]), _bits(want))


# ------------------------------------------------------------------ readlane_d
def _bit_patterns64(rng, n):
    v = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    v[0::8] = (v[0::8] & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x7FF0000000000000)  # NaN payloads, quiet or not
    v[1::8] = (v[1::8] & np.uint64(0x800FFFFFFFFFFFFF))                                  # denormals, both signs
    v[2] = np.uint64(0x7FF0000000000001); v[3] = np.uint64(0xFFF8000000000000); v[4] = np.uint64(1)
    v[5] = np.uint64(0x8000000000000000)
    return v


def test_readlane_double_every_source_lane_bit_patterns(probe):
    rng = np.random.default_rng(30)
    inp = _bit_patterns64(rng, 64 * 64).reshape(64, 64)
    for r in range(64):
        inp[r] = np.roll(inp[r], r)  # every special pattern visits every lane
    src = np.arange(64, dtype=np.int32)
    out = np.zeros_like(inp)
    assert probe.nmpc_probe_readlane_f64(64, _dp(inp.view(np.float64)), _ip(src), _dp(out.view(np.float64))) == 0
    np.testing.assert_array_equal(out, np.repeat(inp[np.arange(64), src][:, None], 64, axis=1))


def test_readlane_float_every_source_lane_bit_patterns(probe):
    rng = np.random.default_rng(31)
    inp = rng.integers(0, 2 ** 32, 64 * 64, dtype=np.uint32)
    inp[0::8] = (inp[0::8] & np.uint32(0x007FFFFF)) | np.uint32(0x7F800000) | np.uint32(1)  # NaN payloads
    inp[1::8] = inp[1::8] & np.uint32(0x807FFFFF)                                            # denormals
    inp = inp.reshape(64, 64)
    for r in range(64):
        inp[r] = np.roll(inp[r], r)
    src = np.arange(64, dtype=np.int32)[::-1].copy()
    out = np.zeros_like(inp)
    assert probe.nmpc_probe_readlane_f32(64, _fp(inp.view(np.float32)), _ip(src), _fp(out.view(np.float32))) == 0
    np.testing.assert_array_equal(out, np.repeat(inp[np.arange(64), src][:, None], 64, axis=1))


# ------------------------------------------------------------------ LogAcc
NF = 24


def _logacc(probe, pairs, x, cnt):
    x = np.ascontiguousarray(x, dtype=np.float64)
    cnt = np.ascontiguousarray(cnt, dtype=np.int32)
    out = np.full(x.shape[0], 12345.0)
    assert probe.nmpc_probe_logacc(pairs, x.shape[0], x.shape[1], _dp(x), _ip(cnt), _dp(out)) == 0
    return out


def _logsum(row):
    return sum((_hp_log(_hp(v)) for v in row), _hp(0.0))


LOG_RANGES = {"solver": (math.log(1e-12), math.log(1e6)), "wide": (-40.0, 40.0),
              "extreme": (-499 * math.log(2), 499 * math.log(2))}


@pytest.mark.parametrize("pairs", [0, 1])
@pytest.mark.parametrize("rng_name", list(LOG_RANGES))
def test_logacc_matches_the_sum_of_logarithms(probe, pairs, rng_name):
    """1..24 positive factors per lane, log-uniform.  Bound 32 * 2^-53 + 4 * 2^-53 * |ref|: the
    product's <= 24 roundings plus one logarithm (a few ulp of a value below ln 2), and the
    roundings of e * ln 2 and of the final sum, relative to the result."""
    lo, hi = LOG_RANGES[rng_name]
    rng = np.random.default_rng(40 + pairs)
    reps = 8
    cnt = np.repeat(np.arange(1, NF + 1), reps)
    x = np.exp(rng.uniform(lo, hi, (cnt.size, NF)))
    out = _logacc(probe, pairs, x, cnt)
    worst = 0.0
    for i in range(cnt.size):
        ref = _logsum(x[i, :cnt[i]])
        bound = 32 * U + 4 * U * abs(float(ref))
        err = abs(float(_hp(out[i]) - ref))
        worst = max(worst, err / bound)
        assert err <= bound, (i, int(cnt[i]), float(out[i]), float(ref), err, bound)
    print(f"LogAcc {'mul2' if pairs else 'mul'} / {rng_name}: largest error / bound = {worst:.3f}")


@pytest.mark.parametrize("pairs", [0, 1])
def test_logacc_non_positive_and_tiny_factors(probe, pairs):
    """What the sum of the logarithms gives: a zero factor -inf, one negative factor NaN, a NaN
    factor NaN, and two tiny positive factors whose product underflows the finite sum of their
    logarithms."""
    x = np.ones((6, NF))
    cnt = np.full(6, 6, dtype=np.int32)
    x[0, :6] = [3.0, 0.5, 0.0, 7.0, 2.0, 1.5]            # a zero
    x[1, :6] = [3.0, 0.5, -2.0, 7.0, 2.0, 1.5]           # one negative
    x[2, :6] = [1e-160, 1e-170, 3.0, 4.0, 5.0, 6.0]      # the pair's product underflows to 0
    x[3, :6] = [2.0, 3.0, 1e-200, 1e-200, 5.0, 6.0]
    x[4, :6] = [2.0, 3.0, np.nan, 4.0, 5.0, 6.0]
    x[5, :6] = [2.0, 3.0, 4.0, 5.0, 6.0, -7.0]           # the negative one last
    out = _logacc(probe, pairs, x, cnt)
    print("LogAcc edges:", out)
    assert out[0] == -np.inf
    assert np.isnan(out[1]) and np.isnan(out[4]) and np.isnan(out[5])
    for i in (2, 3):
        ref = _logsum(x[i, :6])
        assert np.isfinite(out[i])
        assert abs(float(_hp(out[i]) - ref)) <= 32 * U + 4 * U * abs(float(ref)), (out[i], float(ref))


def test_logacc_sign_case_is_a_documented_precondition(probe):
    """Two negative factors in one lane: their signs cancel in the product, so the lane returns
    a finite value where the sum of the logarithms is NaN.  A per-lane sign flag that returns
    NaN was measured against the parent and cost more than the run-to-run spread (DESIGN.md
    11.2), so the case is a precondition of LogAcc, stated above the struct and met by its
    callers; this test holds the wording in place and shows the behaviour it warns of."""
    import os
    import __graft_entry__ as ge
    with open(os.path.join(ge.CSRC, "nmpc_solve.hip")) as fh:
        text = " ".join(fh.read().replace("//", " ").split())
    assert "PRECONDITION: at most one negative argument per lane." in text
    assert "the signs of two cancel in the product and the lane returns a finite value" in text
    x = np.ones((1, NF))
    x[0, :6] = [-1.0, -2.0, 3.0, 4.0, 5.0, 6.0]
    for pairs in (0, 1):
        out = _logacc(probe, pairs, x, np.array([6], dtype=np.int32))
        assert abs(out[0] - math.log(720.0)) <= 1e-14 * math.log(720.0), out


# ------------------------------------------------------------------ rcp / rsq
def _ulp_err(got, ref_mp):
    r = float(ref_mp)
    return abs(float((_hp(got) - ref_mp) / _hp(math.ulp(r))))


def _operands(rng, n):
    """The solver's range (slacks, distances, pivots: 1e-20 .. 1e20) and the full range in
    which the operand and the result are both normal numbers, plus its two ends."""
    a = 10.0 ** rng.uniform(-20, 20, n)
    b = np.ldexp(1.0 + rng.random(n), rng.integers(-1022, 1022, n))
    return np.concatenate([a, b, [2.0 ** -1022, 2.0 ** 1022, 1.0, 2.0, 3.0, 0.1]])


@pytest.mark.parametrize("op,name", [(0, "rcp"), (1, "rsq")])
def test_rcp_rsq_double_within_two_ulp(probe, op, name):
    """<= 2 ulp of the correctly rounded 1/x, 1/sqrt(x): the comment's "~1 ulp" of the Newton
    iterate plus the final rounding."""
    rng = np.random.default_rng(50 + op)
    x = _operands(rng, 6000)
    out = np.zeros_like(x)
    assert probe.nmpc_probe_unary(op, x.size, _dp(x), _dp(out)) == 0
    errs = np.array([_ulp_err(o, (_hp(1.0) / _hp(v)) if op == 0 else _hp(1.0) / _hp_sqrt(_hp(v)))
                     for v, o in zip(x, out)])
    k = int(np.argmax(errs))
    print(f"{name} (double): largest error {errs[k]:.3f} ulp at x = {x[k]!r}; "
          f"share above 0.5 ulp {np.mean(errs > 0.5):.4f}")
    assert errs[k] <= 2.0


def test_rsq_float_within_two_ulp(probe):
    # v_rsq_f32's documented 1 ulp, plus one
    rng = np.random.default_rng(52)
    x = np.concatenate([(10.0 ** rng.uniform(-20, 20, 20000)),
                        np.ldexp(1.0 + rng.random(20000), rng.integers(-126, 127, 20000))]).astype(np.float32)
    out = np.zeros_like(x)
    assert probe.nmpc_probe_rsqf(x.size, _fp(x), _fp(out)) == 0
    ref = 1.0 / np.sqrt(x.astype(np.float64))
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    errs = np.abs(out.astype(np.float64) - ref) / ulp
    k = int(np.argmax(errs))
    print(f"rsq (float): largest error {errs[k]:.3f} ulp at x = {x[k]!r}")
    assert errs[k] <= 2.0


# ------------------------------------------------------------------ qd
def _qd(probe, a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    q = np.full_like(a, 12345.0)
    assert probe.nmpc_probe_qd(a.size, _dp(a), _dp(b), _dp(q)) == 0
    return q


def _differ(q, a, b):
    with np.errstate(all="ignore"):
        want = a / b
    return np.flatnonzero(_bits(q) != _bits(want)), want


def _m(rng, n):
    return 1.0 + rng.random(n)


def _sgn(rng, n):
    return rng.choice([-1.0, 1.0], n)


def test_qd_is_bitwise_the_ieee_quotient_in_its_domain(probe):
    """2^20 random pairs of both signs, the exponents of a, b and a / b in [-500, 500] (there the
    Markstein correction's residual, ~2^-53 |a|, stays a normal number), plus the solver's
    shapes: 1 / b, mu / slack, tau * slack / step."""
    rng = np.random.default_rng(60)
    n = 1 << 20
    eb = rng.integers(-500, 501, n)
    ea = np.clip(eb + rng.integers(-499, 500, n), -500, 500)
    sets = {"random": (_sgn(rng, n) * np.ldexp(_m(rng, n), ea), _sgn(rng, n) * np.ldexp(_m(rng, n), eb))}
    k = 1 << 17
    sets["1/b"] = (np.ones(k), np.ldexp(_m(rng, k), rng.integers(-40, 40, k)))
    sets["mu/slack"] = (10.0 ** rng.integers(-11, 2, k).astype(float) * rng.choice([1.0, 0.2, 1.5], k),
                        10.0 ** rng.uniform(-12, 6, k))
    sets["tau*slack/step"] = (-0.99 * np.ldexp(_m(rng, k), rng.integers(-30, 10, k)),
                              -np.ldexp(_m(rng, k), rng.integers(-30, 10, k)))
    for name, (a, b) in sets.items():
        bad, want = _differ(_qd(probe, a, b), a, b)
        print(f"qd {name}: {bad.size} of {a.size} differ from a / b")
        assert bad.size == 0, (name, a[bad[:4]], b[bad[:4]], want[bad[:4]])


def test_qd_on_the_operands_of_the_sites_that_kept_plain_division(probe):
    """stage_cost's quotients -- c^2, s^2 and 1 over a^2 and over b^2, a = z (tan(x6 + hv) -
    tan(x6 - hv)) / 2 and b likewise from x5 and the horizontal field of view, over the model's
    heights and angles -- and the restoration gr term's -- mu / (s - lo), mu / (hi - s) with the
    row bounds of the model, mu / p, mu / n: the two sites kept the compiler's division because
    results moved in the last bit with qd.  If qd differed from a / b on such operands this
    would isolate the cause."""
    rng = np.random.default_rng(61)
    k = 1 << 17

    def half_axis(lim):  # z (tan(x + h) - tan(x - h)) / 2, squared, as stage_cost forms it
        z = rng.uniform(0.5, 200.0, k)
        ang, h = rng.uniform(-lim, lim, k), rng.choice([0.2, 0.35, 0.5], k)
        v = (z * np.tan(ang + h) - z * np.tan(ang - h)) / 2
        return v * v

    a2, b2 = half_axis(0.55), half_axis(0.55)  # |x6|, |x5| <= pi / 6 in the model, with margin
    assert np.all(np.isfinite(a2) & (a2 > 0) & np.isfinite(b2) & (b2 > 0))
    th = rng.uniform(-np.pi, np.pi, k)
    c2, s2, one = np.cos(th) ** 2, np.sin(th) ** 2, np.ones(k)
    mu = 10.0 ** rng.uniform(-11, 3, k)
    # slacks of the box rows: s within the row's bounds (z in [75, 150], angles in +-0.2618 .. +-pi/2),
    # from a relative distance of 1e-12 to the bound up to the whole range
    lo = rng.choice([75.0, -0.2618, -np.pi / 6, -np.pi / 2], k)
    hi = np.where(lo == 75.0, 150.0, -lo)
    frac = 10.0 ** rng.uniform(-12, 0, k)
    sv = np.where(rng.random(k) < 0.5, lo + frac * (hi - lo), hi - frac * (hi - lo))
    sl, su = sv - lo, hi - sv
    keep = (sl > 0) & (su > 0)
    obst = 10.0 ** rng.uniform(-9, 4, k)  # obstacle rows: hi - s, one-sided
    pn = 10.0 ** rng.uniform(-14, 5, k)
    sets = {"c^2/a^2": (c2, a2), "s^2/b^2": (s2, b2), "s^2/a^2": (s2, a2), "c^2/b^2": (c2, b2),
            "1/a^2": (one, a2), "1/b^2": (one, b2), "mu/(s-lo)": (mu[keep], sl[keep]),
            "mu/(hi-s)": (mu[keep], su[keep]), "mu/(hi-s) obstacle": (mu, obst), "mu/p, mu/n": (mu, pn)}
    total = 0
    for name, (a, b) in sets.items():
        bad, want = _differ(_qd(probe, a, b), a, b)
        total += bad.size
        print(f"qd {name}: {bad.size} of {a.size} differ from a / b", a[bad[:4]], b[bad[:4]])
    assert total == 0, "qd differs from a / b on a kept-division site's operands: the isolated cause"


def test_qd_edge_operands(probe):
    """What the sequence itself implies, with no range fix-up: a zero numerator gives a zero;
    a zero or infinite denominator gives NaN (rcp = inf or 0, then 0 * inf in the Newton
    step) where a / b gives +-inf or 0; a NaN operand gives NaN."""
    inf, nan = np.inf, np.nan
    a = np.array([0.0, -0.0, 0.0, 1.0, -3.0, 1.0, 5.0, nan, 2.0, nan, 0.0, 0.0])
    b = np.array([3.0, 7.0, -2.5, 0.0, 0.0, inf, -inf, 2.0, nan, nan, 0.0, inf])
    q = _qd(probe, a, b)
    print("qd edges:", q)
    assert np.all(q[:3] == 0.0)
    assert np.all(np.isnan(q[3:]))


def test_qd_domain_map(probe):
    """Where bitwise equality with a / b stops, over the exponents of a and b (printed for
    DESIGN.md; nothing asserted about the map itself beyond the launch succeeding)."""
    rng = np.random.default_rng(62)
    es = np.unique(np.r_[np.arange(-1022, 1024, 31), -1000, -980, -970, -969, -960, 1000, 1020, 1021, 1022, 1023])
    reps = 64
    EA, EB = np.meshgrid(es, es, indexing="ij")
    ea, eb = np.repeat(EA.ravel(), reps), np.repeat(EB.ravel(), reps)
    a, b = np.ldexp(_m(rng, ea.size), ea), np.ldexp(_m(rng, eb.size), eb)
    q = _qd(probe, a, b)
    with np.errstate(all="ignore"):
        want = a / b
    diff = (_bits(q) != _bits(want)).reshape(es.size, es.size, reps).any(axis=2)
    print(f"qd domain map: {int(diff.sum())} of {diff.size} exponent cells hold a difference")
    for name, cond in (("e_b", EB), ("e_a", EA), ("e_a - e_b", EA - EB)):
        good = cond[~diff]
        badv = cond[diff]
        print(f"  {name}: equal over [{good.min()}, {good.max()}]; differing cells span "
              f"[{badv.min() if badv.size else None}, {badv.max() if badv.size else None}]")
    # the largest box |e_a|, |e_b|, |e_a - e_b| <= E without any difference
    for E in (1000, 900, 800, 700, 600, 500, 400):
        box = (np.abs(EA) <= E) & (np.abs(EB) <= E) & (np.abs(EA - EB) <= E)
        if not diff[box].any():
            print(f"  no difference where |e_a|, |e_b|, |e_a - e_b| <= {E}")
            break
    print("  map (x: some pair of the cell differs), one row per exponent of a, columns = exponents of b:")
    print("  e_b = " + " ".join(str(int(e)) for e in es))
    for e, row in zip(es, diff):
        print(f"  e_a {int(e):5d} " + "".join("x" if d else "." for d in row))
