"""nmpc_policy_rollout_batch / nmpc_policy_rollout_batch_dev (Solver.policy_rollout,
policy_rollout_device, nmpc_amd.policy.rollout): M disturbance rollouts per scenario of the clamped
feedback policy on the nonlinear plant, one lane per sample, against the NumPy checker of
tests/rollout_ref.py (oracle dynamics, stage cost and rows, one sample at a time).

Cases: the four solved cases of tests/solve_adjoint_ref.py and the synthetic n1 and n63_16obs of the
policy tests; policies from policy_device on the same inputs; M = 3, 64 and 70 (a partial wave, a full
wave, a second block with a tail) are the first M of 70 samples drawn once.

Samples: sample 0 undisturbed; e0 ~ N(0, diag SIGMA^2), w a tenth of that per stage; samples 1 and 2
multiplied by SCALE so that clamps engage.  The clamp box is the solve's control bounds moved outwards
by 0.1 % of each range (tests/rollout_ref.widen says why: at the solve's own bounds the controls active
at the plan sit 1e-16 to 1e-7 from a clamp decision whatever the disturbance).  SIGMA, SCALE and the
seed are chosen on the checker alone (dense-oracle policies, no GPU), such that in every case some
sample has nsat > 0, some has nsat = 0 and the smallest clamp margin exceeds 1e-6; the test asserts the
three conditions from the checker's output at the policy it is given, trying the seeds of SEEDS in
order and keeping the first that meets them (a margin is a draw: 4e-6 was the smallest seen).

Tolerance of gate (b): max(1e-10 (1 + |value|), 100 s) per entry, s being the checker's own spread
when its e0 is perturbed relatively by 1e-15 (second seed).  Every figure is printed before it is
asserted."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import eval_ref as er
from tests import policy_ref as pf
from tests import rollout_ref as rr
from tests.test_gpu_solve_adjoint import _solved, _solver, _ulps  # the solved cases are shared
from tests.test_gpu_solve_tangent import _dirs, _prep

pytestmark = pytest.mark.gpu

SIGMA = (0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02)  # m, m, m, rad ...
SCALE = 20.0
BIG = (1, 2)
SEEDS = (12, 13, 14, 15)
MARGIN = 1e-6
M_ALL = 70
MS = (3, 64, 70)
OUT = ("J", "viol", "nsat", "X", "U")
CASES = tuple(pf.SOLVED) + ("n1", "n63_16obs")


def _f64(a):
    import torch

    return torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device="cuda")


def _with_spread(prob, P, ubar, Xbar, K, e0, w, bounds):
    """The checker's result and its spread s under a relative 1e-15 perturbation of e0."""
    ref = rr.rollout_batch(prob, P, ubar, Xbar, K, e0, w, *bounds)
    rng = np.random.default_rng(4242)
    per = rr.rollout_batch(prob, P, ubar, Xbar, K, e0 * (1.0 + 1e-15 * rng.standard_normal(e0.shape)), w, *bounds)
    with np.errstate(invalid="ignore"):
        spread = {k: np.abs(per[k] - ref[k]) for k in ("J", "viol", "X", "U")}
    return ref, spread


@functools.lru_cache(maxsize=None)
def _case(name):
    """Everything a case's tests share, computed once and left unchanged: the point, the policy of
    policy_device, 70 samples, the checker's result on them and its spread."""
    import torch

    if name in pf.SOLVED:
        spec, s, B, P, bounds, sol = _solved(name)
    else:
        spec = er.case_spec(name)
        s, B = _solver(spec), er.CASES[name]
        d = er.draw_point(spec, B, seed=31)
        bounds, P = (d["lbx"], d["ubx"], d["lbg"], d["ubg"]), d["p"]
        sol = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    prob = er.problem_of(spec)
    dsol, db, dP, _, _ = _prep(spec, sol, bounds, P, np.zeros((spec.np, 1)), B, 1, keys=(), g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, None)
    torch.cuda.synchronize()
    assert np.all(pol["info"].cpu().numpy() == 0), name
    K, Xbar = pol["K"].cpu().numpy(), pol["X"].cpu().numpy()
    ubar = np.ascontiguousarray(sol["x"].T)
    lo, hi = rr.widen(bounds[0], bounds[1])
    cb = (lo, hi, bounds[2], bounds[3])
    for seed in SEEDS:
        e0, w = rr.draw_disturbances(prob, B, M_ALL, SIGMA, seed, big=BIG, scale=SCALE)
        ref, spread = _with_spread(prob, P, ubar, Xbar, K, e0, w, cb)
        ok = (np.any(ref["nsat"][:, :3] > 0), np.any(ref["nsat"][:, :3] == 0), float(np.min(ref["margin"])) > MARGIN)
        print(f"{name}: seed {seed}: nsat 0 to {ref['nsat'].max()}, smallest clamp margin {np.min(ref['margin']):.2e}, "
              f"conditions {ok}")
        if all(ok):
            break
    assert all(ok), (name, ok)
    assert np.all(ref["nsat"][:, 0] == 0)
    dev = {"p": dP, "ubar": dsol["x"], "e0": _f64(e0), "w": _f64(w), "lbx": _f64(lo), "ubx": _f64(hi),
           "lbg": _f64(bounds[2]), "ubg": _f64(bounds[3])}
    return {"name": name, "spec": spec, "s": s, "prob": prob, "B": B, "P": P, "bounds": bounds, "cb": cb, "sol": sol,
            "pol": pol, "K": K, "Xbar": Xbar, "ubar": ubar, "e0": e0, "w": w, "ref": ref, "spread": spread, "dev": dev}


def _run(c, sl=slice(0, M_ALL), feedback=True, clamp=True, rows=True, dist=True, want=OUT, **over):
    """policy_rollout_device on the samples `sl` of a case; NumPy results."""
    import torch

    d = dict(c["dev"], **over)
    res = c["s"].policy_rollout_device(
        d["p"], d["ubar"], c["pol"]["raw"]["X"], d.get("K", c["pol"]["raw"]["K"]) if feedback else None,
        d["e0"][:, sl].contiguous(), w=d["w"][:, sl].contiguous() if dist else None, lbx=d["lbx"] if clamp else None,
        ubx=d["ubx"] if clamp else None, lbg=d["lbg"] if rows else None, ubg=d["ubg"] if rows else None, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(a, b, what, keys=OUT):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _against(name, got, ref, spread, sl, what):
    """Gate (b): X, U, J, viol within max(1e-10 (1 + |value|), 100 s), NaN where the checker has NaN,
    nsat equal.  Returns the largest error / tolerance per output."""
    figs = {}
    for k in ("X", "U", "J", "viol"):
        r, sp, g = ref[k][:, sl], spread[k][:, sl], got[k]
        bad = ~np.isfinite(r)
        np.testing.assert_array_equal(np.isnan(g), np.isnan(r), err_msg=f"{name} {what}: NaN pattern of {k}")
        np.testing.assert_array_equal(g[bad], r[bad], err_msg=f"{name} {what}: non-finite {k}")
        tol = np.maximum(1e-10 * (1.0 + np.abs(r[~bad])), 100.0 * np.where(np.isfinite(sp[~bad]), sp[~bad], 0.0))
        figs[k] = float(np.max(np.abs(g[~bad] - r[~bad]) / tol, initial=0.0))
    print(f"{name} {what}: error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + f"; nsat 0 to {ref['nsat'][:, sl].max()}")
    np.testing.assert_array_equal(got["nsat"], ref["nsat"][:, sl], err_msg=f"{name} {what}: nsat")
    for k, v in figs.items():
        assert v <= 1.0, (name, what, k, v)
    return figs


@pytest.mark.parametrize("name", CASES)
def test_gate_a_the_undisturbed_sample_is_the_plan(name):
    """Sample 0 (e0 = 0, no w), no clamp: X_out is Solver.evaluate's X bitwise -- the kernel's plant
    is the rollout's sequential recursion -- U_out is ubar bitwise, nsat 0, viol the checker's."""
    c = _case(name)
    spec, B, N = c["spec"], c["B"], c["spec"].N
    got = _run(c, slice(0, 1), clamp=False, dist=False)
    X = c["s"].evaluate(c["sol"]["x"], c["P"].T)["X"].T.reshape(B, N + 1, -1)
    print(f"{name}: X against evaluate's, largest difference {_ulps(got['X'][:, 0], X):.1f} ulps; "
          f"U against ubar {_ulps(got['U'][:, 0].reshape(B, -1), c['ubar']):.1f} ulps")
    np.testing.assert_array_equal(got["X"][:, 0], X)
    np.testing.assert_array_equal(got["U"][:, 0].reshape(B, -1), c["ubar"])
    assert np.all(got["nsat"] == 0)
    r = c["ref"]["viol"][:, :1]
    err = np.abs(got["viol"] - r)
    print(f"{name}: viol {got['viol'].ravel()}, against the checker's {np.max(err):.2e}")
    assert np.all(err <= 1e-10 * (1.0 + np.abs(r)))


@pytest.mark.parametrize("name", CASES)
def test_gate_b_every_sample_against_the_checker(name):
    """M = 3, 64, 70: X, U, J and viol within tolerance of the checker's, nsat equal."""
    c = _case(name)
    for M in MS:
        _against(name, _run(c, slice(0, M)), c["ref"], c["spread"], slice(0, M), f"M = {M}")


@pytest.mark.parametrize("name", CASES)
def test_gate_c_open_loop_replay(name):
    """feedback=False is bitwise a call with K of all zeros; J under feedback is finite wherever the
    checker's is."""
    import torch

    c = _case(name)
    ol = _run(c, feedback=False)
    zero = _run(c, K=torch.zeros_like(c["pol"]["raw"]["K"]))
    _same(ol, zero, f"{name}: K = None against K = 0")
    fb = _run(c)
    fin = np.isfinite(c["ref"]["J"])
    assert np.all(np.isfinite(fb["J"][fin])), name
    print(f"{name}: mean J open loop {np.nanmean(ol['J']):.4g}, under feedback {np.nanmean(fb['J']):.4g}; worst viol "
          f"{np.nanmax(ol['viol']):.3g} / {np.nanmax(fb['viol']):.3g}")


def test_gate_d_splits_sharing_and_the_host_entry_point():
    """All bitwise: M = 70 equals M = 64 and M = 6 on the split samples; ld = 0 sharing equals
    replicated inputs; the host entry point equals the device one for every subset of the outputs."""
    import torch

    c = _case("race_track_2")
    B, s = c["B"], c["s"]
    full = _run(c)
    a, b = _run(c, slice(0, 64)), _run(c, slice(64, 70))
    for k in OUT:
        np.testing.assert_array_equal(np.concatenate([a[k], b[k]], axis=1), full[k], err_msg=f"split: {k}")
    # ld = 0: scenario 0's p, plan, policy and samples shared by B scenarios, against replicated ones
    d, raw = c["dev"], c["pol"]["raw"]
    one = {k: d[k][0].contiguous() for k in ("p", "ubar", "e0", "w")}
    rep = {k: v.unsqueeze(0).expand(B, *v.shape).contiguous() for k, v in one.items()}
    K1, X1 = raw["K"][0].contiguous(), raw["X"][0].contiguous()
    kw = dict(lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], want=OUT)
    shared = s.policy_rollout_device(rep["p"], one["ubar"], X1, K1, one["e0"], w=one["w"], **kw)
    repl = s.policy_rollout_device(rep["p"], rep["ubar"], X1.unsqueeze(0).expand(B, *X1.shape).contiguous(),
                                   K1.unsqueeze(0).expand(B, *K1.shape).contiguous(), rep["e0"], w=rep["w"],
                                   lbx=d["lbx"].unsqueeze(0).expand(B, -1).contiguous(),
                                   ubx=d["ubx"].unsqueeze(0).expand(B, -1).contiguous(),
                                   lbg=d["lbg"].unsqueeze(0).expand(B, -1).contiguous(),
                                   ubg=d["ubg"].unsqueeze(0).expand(B, -1).contiguous(), want=OUT)
    torch.cuda.synchronize()
    for k in OUT:
        sh, rp = shared[k].cpu().numpy(), repl[k].cpu().numpy()
        np.testing.assert_array_equal(sh, rp, err_msg=f"ld = 0: {k}")
        np.testing.assert_array_equal(sh[0], full[k][0], err_msg=f"ld = 0 against the batch's scenario 0: {k}")
        for j in range(1, B):
            np.testing.assert_array_equal(sh[j], sh[0], err_msg=k)
    # every subset of the outputs, host against device entry point
    for n in range(1, len(OUT) + 1):
        for keys in itertools.combinations(OUT, n):
            if keys == ("nsat",):
                continue
            host = s.policy_rollout(c["P"], c["ubar"], c["Xbar"], c["K"], c["e0"], c["w"], *c["cb"], want=keys)
            dev = _run(c, want=keys)
            assert set(host) == set(dev) == set(keys), keys
            for k in keys:
                np.testing.assert_array_equal(host[k], full[k], err_msg=f"host, outputs {keys}: {k}")
                np.testing.assert_array_equal(dev[k], full[k], err_msg=f"device, outputs {keys}: {k}")


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_d_no_write_outside_the_outputs(name):
    """Output buffers carved out of one tensor of sentinels: every entry of them is written, nothing
    outside them is (uav5: blocks of 5 states and 3 controls)."""
    import torch

    c = _case(name)
    B, s, spec = c["B"], c["s"], c["spec"]
    N, nu, nx = spec.N, spec.nw // spec.N, spec.nX // (spec.N + 1)
    if name == "uav5":
        assert (nu, nx) == (3, 5)
    M, pad = 70, 64
    shapes = s._rollout_shapes(B, M)
    assert shapes["X"] == (B, M, N + 1, nx) and shapes["U"] == (B, M, N, nu)
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    ibig = torch.full((B * M + 2 * pad,), 77, dtype=torch.int32, device="cuda")
    out, o, spans = {"nsat": ibig[pad:pad + B * M].view(B, M)}, pad, []
    for k, shp in shapes.items():
        if k == "nsat":
            continue
        n = int(np.prod(shp))
        out[k] = big[o:o + n].view(shp)
        spans.append((o, o + n))
        o += n + pad
    d = c["dev"]
    res = s.policy_rollout_device(d["p"], d["ubar"], c["pol"]["raw"]["X"], c["pol"]["raw"]["K"], d["e0"], w=d["w"],
                                  lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], out=out)
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in OUT)
    h, hi = big.cpu().numpy(), ibig.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for a, b in spans:
        keep[a:b] = False
        assert not np.any(h[a:b] == 7.0)
    assert np.all(h[keep] == 7.0)
    assert np.all(hi[:pad] == 77) and np.all(hi[pad + B * M:] == 77) and not np.any(hi[pad:pad + B * M] == 77)
    _same({k: v.cpu().numpy() for k, v in res.items()}, _run(c), f"{name}: carved buffers against own ones")


def test_gate_e_nan_handling():
    """A NaN in one sample's e0 gives NaN in that sample's J and viol only; a scenario whose policy is
    NaN (info != 0: lbx > ubx through policy_device) gives NaN samples beside bitwise-untouched
    neighbours."""
    import torch

    c = _case("race_track_2")
    spec, s, B, P, bounds, sol = c["spec"], c["s"], c["B"], c["P"], c["bounds"], c["sol"]
    full = _run(c)
    e0 = c["dev"]["e0"].clone()
    e0[1, 5, 3] = float("nan")
    got = _run(c, e0=e0)
    assert np.isnan(got["J"][1, 5]) and np.isnan(got["viol"][1, 5])
    mask = np.ones((B, M_ALL), bool)
    mask[1, 5] = False
    for k in OUT:
        np.testing.assert_array_equal(got[k][mask], full[k][mask], err_msg=k)
    assert np.all(np.isfinite(full["J"])) and np.all(np.isfinite(full["viol"]))
    # a NaN in w reaches J and viol too, whichever state it enters
    w = c["dev"]["w"].clone()
    w[2, 7, spec.N - 1, 4] = float("nan")
    got = _run(c, w=w)
    assert np.isnan(got["J"][2, 7]) and np.isnan(got["viol"][2, 7])
    mask = np.ones((B, M_ALL), bool)
    mask[2, 7] = False
    np.testing.assert_array_equal(got["J"][mask], full["J"][mask])
    # an invalid scenario's policy
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in bounds[:2])
    lb3[5, 1] = ub3[5, 1] + 1.0
    dsol, db, dP, _, _ = _prep(spec, sol, (lb3, ub3, bounds[2], bounds[3]), P, np.zeros((spec.np, 1)), B, 1, keys=(),
                               g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, None)
    d = c["dev"]
    res = s.policy_rollout_device(d["p"], d["ubar"], pol["raw"]["X"], pol["raw"]["K"], d["e0"], w=d["w"], lbx=d["lbx"],
                                  ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], want=OUT)
    torch.cuda.synchronize()
    assert pol["info"].cpu().numpy().tolist() == [0, -11] + [0] * (B - 2)
    got = {k: v.cpu().numpy() for k, v in res.items()}
    assert np.all(np.isnan(got["J"][1])) and np.all(np.isnan(got["viol"][1]))
    for k in OUT:
        np.testing.assert_array_equal(np.delete(got[k], 1, axis=0), np.delete(full[k], 1, axis=0), err_msg=k)


def test_gate_f_nothing_read_back_nothing_allocated_and_the_feedforward(monkeypatch):
    """With torch.Tensor.cpu made to raise policy_rollout_device still completes, into preallocated
    buffers, and the handle's memory_info is unchanged; nmpc_amd.policy.rollout with coefficients c
    equals the checker fed ubar = u* + sum_d kff^(d) c_d formed in NumPy, at the moved parameters."""
    import torch
    from nmpc_amd import policy

    c = _case("race_track_2")
    spec, s, B, P, bounds, sol = c["spec"], c["s"], c["B"], c["P"], c["bounds"], c["sol"]
    d, raw = c["dev"], c["pol"]["raw"]
    full = _run(c)
    mem = s.memory_info()
    first = s.policy_rollout_device(d["p"], d["ubar"], raw["X"], raw["K"], d["e0"], w=d["w"], lbx=d["lbx"], ubx=d["ubx"],
                                    lbg=d["lbg"], ubg=d["ubg"], want=OUT)
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a host round trip in policy_rollout_device")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        again = s.policy_rollout_device(d["p"], d["ubar"], raw["X"], raw["K"], d["e0"], w=d["w"], lbx=d["lbx"],
                                        ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], out=first)
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    assert all(again[k] is first[k] for k in OUT)
    _same({k: v.cpu().numpy() for k, v in again.items()}, full, "into its own buffers")
    # the feedforward: a parameter move along two directions
    nd, M = 2, 3
    dp = _dirs(spec, B, nd, 97)
    dsol, db, dP, dd, _ = _prep(spec, sol, bounds, P, dp, B, nd, keys=(), g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, dd)
    coef = 0.05 * np.random.default_rng(99).standard_normal((B, nd))
    Pm = P + np.einsum("bd,pdb->bp", coef, dp)
    got = policy.rollout(s, pol, dsol, _f64(Pm), d["e0"][:, :M].contiguous(), w=d["w"][:, :M].contiguous(), c=_f64(coef),
                         lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], want=OUT)
    torch.cuda.synchronize()
    kff = pol["kff"].cpu().numpy()
    ubar = c["ubar"] + np.einsum("bdn,bd->bn", kff.reshape(B, nd, -1), coef)
    ref, spread = _with_spread(c["prob"], Pm, ubar, pol["X"].cpu().numpy(), pol["K"].cpu().numpy(), c["e0"][:, :M],
                               c["w"][:, :M], c["cb"])
    print(f"feedforward: smallest clamp margin {np.min(ref['margin']):.2e}")
    assert np.min(ref["margin"]) > MARGIN
    _against("race_track_2", {k: v.cpu().numpy() for k, v in got.items()}, ref, spread, slice(0, M), "policy.rollout with c")
    ol = policy.rollout(s, pol, dsol, _f64(Pm), d["e0"][:, :M].contiguous(), c=_f64(coef), feedback=False, want=("J", "U"))
    torch.cuda.synchronize()
    np.testing.assert_allclose(ol["U"].cpu().numpy()[:, 0].reshape(B, -1), ubar, rtol=1e-14, atol=1e-14)


def test_argument_validation_on_a_live_handle():
    """B <= 0, M <= 0, a NULL p, ubar, Xbar or e0, every main output NULL, lbg without ubg and the
    reverse, and a leading dimension that is neither 0 nor >= the vector length return NMPC_E_INVALID
    from both entry points before any device call: nothing is written, and the handle still works."""
    from nmpc_amd import _lib

    c = _case("race_track_2")
    spec, s, B = c["spec"], c["s"], c["B"]
    N, nu, nx = spec.N, spec.nw // spec.N, spec.nX // (spec.N + 1)
    L = _lib.lib()
    M = 5
    arr = {"p": c["P"], "ubar": c["ubar"], "Xbar": c["Xbar"], "K": np.swapaxes(c["K"], 2, 3),
           "lbx": np.repeat(c["cb"][0][None], B, 0), "ubx": np.repeat(c["cb"][1][None], B, 0),
           "lbg": np.repeat(c["cb"][2][None], B, 0), "ubg": np.repeat(c["cb"][3][None], B, 0),
           "e0": c["e0"][:, :M], "w": c["w"][:, :M]}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    names = tuple(arr)
    lens = dict(zip(names, (spec.np, spec.nw, spec.nX, nu * nx * N, spec.nw, spec.nw, spec.ng, spec.ng, nx * M, nx * N * M)))
    arr.update(J=np.full((B, M), 7.0), viol=np.full((B, M), 7.0), X=np.full((B, M, N + 1, nx), 7.0),
               U=np.full((B, M, N, nu), 7.0))
    nsat = np.full((B, M), 99, dtype=np.int32)
    dpt, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)

    def call(B_=B, M_=M, null=(), ld=None, dev=False):
        ld = dict(lens, **(ld or {}))
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k not in null else vp(0)  # noqa: E731
            gi = vp(nsat.ctypes.data)
        else:
            g = lambda k: arr[k].ctypes.data_as(dpt) if k not in null else None  # noqa: E731
            gi = nsat.ctypes.data_as(ip)
        args = [s._h, B_, M_]
        for k in names:
            args += [g(k), ld[k]]
        args += [g("J"), g("viol"), gi, g("X"), g("U")]
        return L.nmpc_policy_rollout_batch_dev(*args, vp(0)) if dev else L.nmpc_policy_rollout_batch(*args)

    main = ("J", "viol", "X", "U")
    # each with the full message of its rule; the last five break two rules at once: the earlier
    # one in the order of the checks answers
    req, ldm = "required pointer is null (p, ubar, Xbar, e0)", "leading dimension smaller than the vector length"
    outs, pair = "J_out, viol_out, X_out and U_out are all null", "lbg and ubg must be given together"
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("M = 0", dict(M_=0), "M <= 0"),
                 ("M < 0", dict(M_=-1), "M <= 0"), ("M too large", dict(M_=64 * 65535 + 1), "M > 64 x 65535"),
                 ("J, viol, X, U NULL", dict(null=main), outs), ("lbg without ubg", dict(null=("ubg",)), pair),
                 ("ubg without lbg", dict(null=("lbg",)), pair), ("ld_p negative", dict(ld={"p": -spec.np}), ldm),
                 ("ld_e0 one sample", dict(ld={"e0": nx}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in ("p", "ubar", "Xbar", "e0")]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and M = 0", dict(B_=0, M_=0), "B <= 0"), ("M = 0 and p NULL", dict(M_=0, null=("p",)), "M <= 0"),
                  ("e0 NULL and no output", dict(null=("e0",) + main), req),
                  ("no output and lbg without ubg", dict(null=main + ("ubg",)), outs),
                  ("lbg without ubg and ld_w short", dict(null=("ubg",), ld={"w": lens["w"] - 1}), pair)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error(), what
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    call(null=main)
    assert "J_out" in L.nmpc_last_error().decode()
    assert all(np.all(arr[k] == 7.0) for k in main) and np.all(nsat == 99)  # nothing ran
    # and the handle still works: J alone without K, bounds or w; then everything
    assert call(null=("K", "lbx", "ubx", "lbg", "ubg", "w", "viol", "X", "U")) == 0
    assert np.all(np.isfinite(arr["J"])) and np.all(nsat == 0) and all(np.all(arr[k] == 7.0) for k in ("viol", "X", "U"))
    assert call() == 0
    full = _run(c, slice(0, M))
    for k in main:
        np.testing.assert_array_equal(arr[k], full[k], err_msg=k)
    np.testing.assert_array_equal(nsat, full["nsat"])
