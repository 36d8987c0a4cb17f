"""nmpc_policy_value_batch / nmpc_policy_value_batch_dev (Solver.policy_value, policy_value_device,
nmpc_amd.policy.expected_cost): the cost-to-go expansion of the unclamped feedback policy along the plan
-- lam_k, P_k, J and per covariance case dJ (E[J] = J + dJ to second order) and varJ -- one wavefront per
scenario, against the NumPy checker of tests/value_ref.py (oracle stage_cost_derivs, dyn_jac and
dyn_hess, one scenario at a time) and against the rollout kernels themselves.

Cases, policies (policy_device) and helpers are tests/test_gpu_policy_rollout.py's, the covariances
tests/test_gpu_policy_covariance.py's: the four solved cases and the synthetic n1 and n63_16obs, so
N = 1, 5, 6, 12, 63, B = 2 ... 4, uav5's 5 x 5 / 3 x 5 blocks, `dynamic`, and nc = 2 (case 1 has W = 0).

Gate (a): P_k per entry within max(1e-10 a_k, 100 s), a_k the largest entry of
|M_k| + |Acl_k|' |P_{k+1}| |Acl_k| at the checker's own P_{k+1} (one step's magnitude) and s the
checker's spread under a relative 1e-15 perturbation of K, Xbar and ubar; lam_k likewise with
|g_k| + |Acl_k|' |lam_{k+1}|; dJ and varJ likewise against A = sum over the sigma-point pairs of
|1/2 d' P_j d| and V = sum of (lam_j . d)^2; J within N 2^-52 sum_k |l_k|.  Where a case leaves less
than a factor of 3, the distance of a second association of the checker's triple product is printed
beside it.  Gate (b1): lam against policy_rollout_adjoint_device at one undisturbed sample with Jb = 1
and no bounds (lam_0 = e0_bar, lam_{k+1} = w_bar[k]) within 1e-9 of the scenario's largest |lam| entry.
Gate (b2): dJ and varJ of case 0 against the +-eps sigma-point pairs through policy_rollout_device, all
pairs of both step sizes and the undisturbed sample in one call, at tests/test_value_capi.py's two
gates.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import covariance_ref as cr
from tests import value_ref as vr
from tests.test_gpu_policy_covariance import NC, _draw
from tests.test_gpu_policy_rollout import CASES, _case, _f64  # the cases and policies are shared
from tests.test_gpu_solve_tangent import _prep
from tests.test_value_capi import EPS_DJ, EPS_VAR, GATE_VAR, dj_gate

pytestmark = pytest.mark.gpu

OUT = ("J", "lam", "P", "dJ", "varJ")
WS_BYTES = 68 * 64 * 8  # the header's workspace statement: one products-kernel slice per scenario


def _scales(prob, ref, S0, W):
    """A and V (B, nc) over the sigma-point pairs, from `ref`'s lam and P (a W of zeros: no pairs)."""
    B, nc = S0.shape[:2]
    A, V = np.zeros((B, nc)), np.zeros((B, nc))
    for b in range(B):
        for c in range(nc):
            A[b, c], V[b, c], _ = vr.pair_scales({"lam": ref["lam"][b], "P": ref["P"][b]}, S0[b, c],
                                                 W[b, c] if np.any(W[b, c]) else None, prob.N)
    return A, V


@functools.lru_cache(maxsize=None)
def _val(name):
    """A case of the rollout tests with its covariances, the checker's result and its spread."""
    c = _case(name)
    prob, B = c["prob"], c["B"]
    S0, W = _draw(prob, B)
    args = (prob, c["P"])
    ref = vr.value_batch(*args, c["ubar"], c["Xbar"], c["K"], S0, W)
    rng = np.random.default_rng(4244)
    pert = [v * (1.0 + 1e-15 * rng.standard_normal(v.shape)) for v in (c["ubar"], c["Xbar"], c["K"])]
    per = vr.value_batch(*args, *pert, S0, W)
    spread = {k: np.abs(per[k] - ref[k]) for k in ("lam", "P", "dJ", "varJ")}
    A, V = _scales(prob, ref, S0, W)
    return dict(c, S0=S0, W=W, vref=ref, vspread=spread, vA=A, vV=V, dS0=_f64(S0), dW=_f64(W))


def _run(cv, want=OUT, feedback=True, noise=True, cases=True, **over):
    """policy_value_device on a case; NumPy results."""
    import torch

    d = dict(cv["dev"], S0=cv["dS0"], W=cv["dW"])
    d.update(over)
    res = cv["s"].policy_value_device(d["p"], d["ubar"], d.get("Xbar", cv["pol"]["raw"]["X"]),
                                      d.get("K", cv["pol"]["raw"]["K"]) if feedback else None,
                                      S0=d["S0"] if cases else None, W=d["W"] if noise and cases else None, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(a, b, what, keys=OUT):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _ratio(err, tol):
    return float(np.max(np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, 1.0) + np.where(tol > 0.0, 0.0, np.inf)),
                        initial=0.0))


def _ratios(got, ref, spread, A, V):
    """Largest error / tolerance of P_k, lam_k (k < N), dJ and varJ under gate (a)'s rule."""
    figs = {"P": _ratio(np.abs(got["P"][:, :-1] - ref["P"][:, :-1]),
                        np.maximum(1e-10 * ref["aP"][..., None, None], 100.0 * spread["P"][:, :-1])),
            "lam": _ratio(np.abs(got["lam"][:, :-1] - ref["lam"][:, :-1]),
                          np.maximum(1e-10 * ref["aL"][..., None], 100.0 * spread["lam"][:, :-1])),
            "dJ": _ratio(np.abs(got["dJ"] - ref["dJ"]), np.maximum(1e-10 * A, 100.0 * spread["dJ"])),
            "varJ": _ratio(np.abs(got["varJ"] - ref["varJ"]), np.maximum(1e-10 * V, 100.0 * spread["varJ"]))}
    return figs


@pytest.mark.parametrize("name", CASES)
def test_gate_a_against_the_checker(name):
    """P_k, lam_k, dJ and varJ of both cases within max(1e-10 x one step's magnitude, 100 s) of the
    checker's."""
    cv = _val(name)
    prob, ref, spread = cv["prob"], cv["vref"], cv["vspread"]
    got = _run(cv)
    assert all(np.all(np.isfinite(got[k])) for k in OUT), name
    figs = _ratios(got, ref, spread, cv["vA"], cv["vV"])
    print(f"{name}: kernel against the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + f"; largest |P| {np.abs(got['P']).max():.3g}, |lam| {np.abs(got['lam']).max():.3g}")
    if max(figs.values()) > 1.0 / 3.0:
        alt = vr.value_batch(prob, cv["P"], cv["ubar"], cv["Xbar"], cv["K"], cv["S0"], cv["W"], order=1)
        af = _ratios(alt, ref, spread, cv["vA"], cv["vV"])
        print(f"{name}: second association of the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in af.items()))
    for k, v in figs.items():
        assert v <= 1.0, (name, k, v)


@pytest.mark.parametrize("name", CASES)
def test_gate_a_plan_cost(name):
    """J within N 2^-52 sum_k |l_k| of the checker's."""
    cv = _val(name)
    ref = cv["vref"]
    got = _run(cv, want=("J",))
    tol = cv["prob"].N * 2.0 ** -52 * np.sum(np.abs(ref["l"]), axis=1)
    fig = _ratio(np.abs(got["J"] - ref["J"]), tol)
    print(f"{name}: J {got['J']}, |J - checker| / (N 2^-52 sum |l_k|) = {fig:.2e}")
    assert fig <= 1.0, (name, fig)


@pytest.mark.parametrize("name", CASES)
def test_gate_b1_lam_against_the_rollout_adjoint(name):
    """lam_0 = e0_bar and lam_{k+1} = w_bar[k] of the rollouts' reverse sweep at the undisturbed sample
    with Jb = 1, no bounds."""
    import torch

    cv = _val(name)
    prob, B, s, d, raw = cv["prob"], cv["B"], cv["s"], cv["dev"], cv["pol"]["raw"]
    N, nx = prob.N, prob.nx
    e0 = torch.zeros((B, 1, nx), dtype=torch.float64, device="cuda")
    X = s.policy_rollout_device(d["p"], d["ubar"], raw["X"], raw["K"], e0, want=("X",))["X"]
    adj = s.policy_rollout_adjoint_device(d["p"], d["ubar"], raw["X"], raw["K"], X,
                                          Jb=torch.ones((B, 1), dtype=torch.float64, device="cuda"), want=("e0_bar", "w_bar"))
    torch.cuda.synchronize()
    other = np.concatenate([adj["e0_bar"].cpu().numpy()[:, 0, None], adj["w_bar"].cpu().numpy()[:, 0]], axis=1)
    lam = _run(cv, want=("lam",))["lam"]
    assert other.shape == lam.shape == (B, N + 1, nx)
    top = np.max(np.abs(lam), axis=(1, 2))
    fig = float(np.max(np.max(np.abs(lam - other), axis=(1, 2)) / top))
    print(f"{name}: |lam - rollout adjoint| / max |lam| = {fig:.2e} (gate 1e-9)")
    assert fig <= 1e-9, (name, fig)


@pytest.mark.parametrize("name", CASES)
def test_gate_b2_moments_against_the_rollouts(name):
    """dJ and varJ of case 0 against the second and first differences of J over the sigma-point pairs of
    S0 and W through policy_rollout_device, unclamped, in one call."""
    import torch

    cv = _val(name)
    prob, B, s, d, raw = cv["prob"], cv["B"], cv["s"], cv["dev"], cv["pol"]["raw"]
    N, nx = prob.N, prob.nx
    n = nx * (N + 1)
    M = 4 * n + 1
    e0, w = np.zeros((B, M, nx)), np.zeros((B, M, N, nx))
    for b in range(B):
        pts = cr.sigma_points(cv["S0"][b, 0], cv["W"][b, 0], N)
        assert len(pts) == n
        for e, eps in enumerate((EPS_DJ, EPS_VAR)):
            for i, (j, dd) in enumerate(pts):
                for h, sgn in enumerate((1.0, -1.0)):
                    q = 1 + 2 * n * e + 2 * i + h
                    if j == 0:
                        e0[b, q] = sgn * eps * dd
                    else:
                        w[b, q, j - 1] = sgn * eps * dd
    J = s.policy_rollout_device(d["p"], d["ubar"], raw["X"], raw["K"], _f64(e0), w=_f64(w), want=("J",))["J"]
    torch.cuda.synchronize()
    J = J.cpu().numpy()
    J0 = J[:, 0]
    Ja, Jb = J[:, 1:1 + 2 * n], J[:, 1 + 2 * n:]
    d2 = np.sum((Ja[:, 0::2] + Ja[:, 1::2] - 2.0 * J0[:, None]) / (2.0 * EPS_DJ ** 2), axis=1)
    d1 = np.sum(((Jb[:, 0::2] - Jb[:, 1::2]) / (2.0 * EPS_VAR)) ** 2, axis=1)
    got = _run(cv)
    A, _ = _scales(prob, got, cv["S0"][:, :1], cv["W"][:, :1])
    gate = np.array([dj_gate(A[b, 0], n, J0[b]) for b in range(B)])
    fD = float(np.max(np.abs(d2 - got["dJ"][:, 0]) / gate))
    fV = float(np.max(np.abs(d1 - got["varJ"][:, 0]) / np.abs(got["varJ"][:, 0])))
    print(f"{name}: M = {M} rollouts per scenario; |sampled - dJ| / gate = {fD:.3f}, varJ relative error {fV:.2e} "
          f"(gate {GATE_VAR:.0e}); the undisturbed sample's J against J_out: {np.max(np.abs(J0 - got['J'])):.2e}")
    assert M > 64
    assert fD <= 1.0 and fV <= GATE_VAR, (name, fD, fV)


def test_gate_c_bitwise_properties():
    """Symmetry, the exact zeros of block N, repeatability, case splits, ld = 0 sharing, host against
    device for every subset of the outputs, K NULL against K = 0, the unread triangles, S0 = 0 and nc = 0."""
    import torch

    for name in ("race_track_2", "uav5"):
        cv = _val(name)
        B, s = cv["B"], cv["s"]
        full = _run(cv)
        np.testing.assert_array_equal(full["P"], np.swapaxes(full["P"], -1, -2), err_msg="P_k is symmetric")
        assert np.all(full["P"][:, -1] == 0.0) and np.all(full["lam"][:, -1] == 0.0)
        _same(_run(cv), full, f"{name}: two calls")
        for c in range(NC):
            one = _run(cv, S0=cv["dS0"][:, c:c + 1].contiguous(), W=cv["dW"][:, c:c + 1].contiguous())
            _same(one, full, f"{name}: nc = 1, case {c}", ("J", "lam", "P"))
            for k in ("dJ", "varJ"):
                np.testing.assert_array_equal(one[k][:, 0], full[k][:, c], err_msg=f"{name}: nc = 1, case {c}: {k}")
        _same(_run(cv, feedback=False), _run(cv, K=torch.zeros_like(cv["pol"]["raw"]["K"])), f"{name}: K NULL against K = 0")
        # the blocks are column-major: entry (i, j) with i < j sits at [..., j, i], below the tensor's diagonal
        nx = cv["prob"].nx
        low = torch.tril(torch.ones((nx, nx), dtype=torch.bool, device="cuda"), -1)
        S0n, Wn = cv["dS0"].clone(), cv["dW"].clone()
        S0n[..., low] = float("nan")
        Wn[..., low] = float("nan")
        _same(_run(cv, S0=S0n, W=Wn), full, f"{name}: NaN in the unread triangles")
        zero = _run(cv, S0=torch.zeros_like(cv["dS0"]), noise=False)
        assert np.all(zero["dJ"] == 0.0) and np.all(zero["varJ"] == 0.0)
        _same(zero, full, f"{name}: S0 = 0, W NULL", ("J", "lam", "P"))
        none = _run(cv, cases=False)
        assert set(none) == {"J", "lam", "P"}
        _same(none, full, f"{name}: nc = 0", ("J", "lam", "P"))
        # ld = 0: scenario 0's inputs shared by B scenarios, against replicated ones
        d, raw = cv["dev"], cv["pol"]["raw"]
        one = {"p": d["p"][0], "ubar": d["ubar"][0], "Xbar": raw["X"][0], "K": raw["K"][0], "S0": cv["dS0"][0], "W": cv["dW"][0]}
        one = {k: v.contiguous() for k, v in one.items()}
        rep = {k: v.unsqueeze(0).expand(B, *v.shape).contiguous() for k, v in one.items()}
        sh = s.policy_value_device(rep["p"], one["ubar"], one["Xbar"], one["K"], S0=one["S0"], W=one["W"], want=OUT)
        rp = s.policy_value_device(rep["p"], rep["ubar"], rep["Xbar"], rep["K"], S0=rep["S0"], W=rep["W"], want=OUT)
        torch.cuda.synchronize()
        for k in OUT:
            a, r = sh[k].cpu().numpy(), rp[k].cpu().numpy()
            np.testing.assert_array_equal(a, r, err_msg=f"{name}: ld = 0: {k}")
            np.testing.assert_array_equal(a[0], full[k][0], err_msg=f"{name}: ld = 0 against the batch's scenario 0: {k}")
        # every subset of the outputs, host against device entry point
        for n in range(1, len(OUT) + 1):
            for keys in itertools.combinations(OUT, n):
                host = s.policy_value(cv["P"], cv["ubar"], cv["Xbar"], cv["K"], cv["S0"], cv["W"], want=keys)
                dev = _run(cv, want=keys)
                assert set(host) == set(dev) == set(keys), keys
                for k in keys:
                    np.testing.assert_array_equal(host[k], full[k], err_msg=f"{name}: host, outputs {keys}: {k}")
                    np.testing.assert_array_equal(dev[k], full[k], err_msg=f"{name}: device, outputs {keys}: {k}")
        print(f"{name}: symmetry, block N, repeatability, case split, K NULL = K 0, unread triangles, zeros, nc = 0, ld = 0 "
              "and host = device: bitwise")


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_c_no_write_outside_the_outputs(name):
    """Output buffers carved out of one tensor of sentinels: every entry of them is written, nothing
    outside them is (uav5: blocks of 5 x 5 and rows of 5)."""
    import torch

    cv = _val(name)
    B, s = cv["B"], cv["s"]
    pad = 64
    shapes = s._value_shapes(B, NC)
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    out, o, spans = {}, pad, []
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = big[o:o + n].view(shp)
        spans.append((o, o + n))
        o += n + pad
    d = cv["dev"]
    res = s.policy_value_device(d["p"], d["ubar"], cv["pol"]["raw"]["X"], cv["pol"]["raw"]["K"], S0=cv["dS0"], W=cv["dW"],
                                out=out, want=())
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in OUT)
    h = big.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for a, b in spans:
        keep[a:b] = False
        assert not np.any(h[a:b] == 7.0)
    assert np.all(h[keep] == 7.0)
    _same({k: v.cpu().numpy() for k, v in res.items()}, _run(cv), f"{name}: carved buffers against own ones")


def test_gate_d_one_stage():
    """N = 1: lam_1 = P_1 = 0, so P_0 is the stage cost's Hessian, to gate (a)'s rule, and lam_0 its
    gradient; neither depends on K, bitwise."""
    import torch

    cv = _val("n1")
    assert cv["prob"].N == 1
    ref, full = cv["vref"], _run(cv)
    fig = _ratio(np.abs(full["P"][:, 0] - ref["P"][:, 0]), np.maximum(1e-10 * ref["aP"][:, 0, None, None], 100.0 * cv["vspread"]["P"][:, 0]))
    print(f"n1: |P_0 - checker's Hessian of l_0| / tolerance = {fig:.2e}")
    assert fig <= 1.0
    K = cv["pol"]["raw"]["K"]
    assert bool(torch.any(K != 0.0))
    _same(_run(cv, feedback=False), full, "n1: open loop")
    _same(_run(cv, K=(3.0 * K + 1.0).contiguous()), full, "n1: other gains")


def test_gate_e_nan_handling():
    """A NaN in one case's S0 stays in that case's dJ and varJ; a scenario whose policy is NaN (info != 0:
    lbx > ubx through policy_device) gives NaN J, lam_0, P_0, dJ and varJ beside bitwise-untouched
    neighbours."""
    import torch

    cv = _val("race_track_2")
    spec, s, B, P, bounds, sol = cv["spec"], cv["s"], cv["B"], cv["P"], cv["bounds"], cv["sol"]
    full = _run(cv)
    S0 = cv["dS0"].clone()
    S0[1, 0, 0, 2] = float("nan")  # entry (2, 0): read
    got = _run(cv, S0=S0)
    assert np.isnan(got["dJ"][1, 0]) and np.isnan(got["varJ"][1, 0])
    for k in ("dJ", "varJ"):
        a, f = got[k].copy(), full[k].copy()
        a[1, 0], f[1, 0] = 0.0, 0.0
        np.testing.assert_array_equal(a, f, err_msg=f"NaN in S0 of (1, 0): {k}")
    _same(got, full, "NaN in S0 of (1, 0)", ("J", "lam", "P"))
    # an invalid scenario's policy
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in bounds[:2])
    lb3[5, 1] = ub3[5, 1] + 1.0
    dsol, db, dP, _, _ = _prep(spec, sol, (lb3, ub3, bounds[2], bounds[3]), P, np.zeros((spec.np, 1)), B, 1, keys=(),
                               g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, None)
    torch.cuda.synchronize()
    assert pol["info"].cpu().numpy().tolist() == [0, -11] + [0] * (B - 2)
    for over in (dict(K=pol["raw"]["K"], Xbar=pol["raw"]["X"]), dict(K=pol["raw"]["K"])):  # (a NaN K alone too)
        got = _run(cv, **over)
        assert np.isnan(got["J"][1]) and np.all(np.isnan(got["lam"][1, 0])) and np.all(np.isnan(got["P"][1, 0]))
        assert np.all(np.isnan(got["dJ"][1])) and np.all(np.isnan(got["varJ"][1]))
        for k in OUT:
            np.testing.assert_array_equal(np.delete(got[k], 1, axis=0), np.delete(full[k], 1, axis=0), err_msg=k)


def test_gate_f_argument_validation_on_a_live_handle():
    """Every rule of the header from both entry points, with its full message, before any device call:
    nothing is written, and the handle still works.  Calls that break two rules get the earlier one's."""
    from nmpc_amd import _lib

    cv = _val("race_track_2")
    spec, s, B = cv["spec"], cv["s"], cv["B"]
    N, nu, nx = spec.N, spec.nw // spec.N, spec.nX // (spec.N + 1)
    L = _lib.lib()
    arr = {"p": cv["P"], "ubar": cv["ubar"], "Xbar": cv["Xbar"], "K": np.swapaxes(cv["K"], 2, 3), "S0": cv["S0"], "W": cv["W"]}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    names = tuple(arr)
    lens = dict(zip(names, (spec.np, spec.nw, spec.nX, nu * nx * N, nx * nx * NC, nx * nx * NC)))
    shapes = s._value_shapes(B, NC)
    arr.update({k: np.full(shapes[k], 7.0) for k in OUT})
    dpt, vp = C.POINTER(C.c_double), C.c_void_p

    def call(h=None, B_=B, nc_=NC, null=(), ld=None, dev=False):
        ld = dict(lens, **(ld or {}))
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k not in null else vp(0)  # noqa: E731
        else:
            g = lambda k: arr[k].ctypes.data_as(dpt) if k not in null else None  # noqa: E731
        args = [h or s._h, B_, nc_]
        for k in names:
            args += [g(k), ld[k]]
        args += [g(k) for k in OUT]
        return L.nmpc_policy_value_batch_dev(*args, vp(0)) if dev else L.nmpc_policy_value_batch(*args)

    req, ldm = "required pointer is null (p, ubar, Xbar)", "leading dimension smaller than the vector length"
    s0m = "required pointer is null (S0 with nc > 0)"
    nc0 = "nc = 0 takes J_out, lam_out and P_out alone (S0, W, dJ_out and varJ_out must be null)"
    outs = "J_out, lam_out, P_out, dJ_out and varJ_out are all null"
    cs = ("S0", "W", "dJ", "varJ")
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("nc < 0", dict(nc_=-1), "nc < 0"),
                 ("S0 NULL", dict(null=("S0",)), s0m), ("every output NULL", dict(null=OUT), outs),
                 ("ld_p negative", dict(ld={"p": -spec.np}), ldm), ("ld_S0 one case", dict(ld={"S0": nx * nx}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in ("p", "ubar", "Xbar")]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [(f"nc = 0 with {k}", dict(nc_=0, null=tuple(q for q in cs if q != k)), nc0) for k in cs]
        cases += [("nc = 0 with no output but dJ", dict(nc_=0, null=("S0", "W", "J", "lam", "P", "varJ")), nc0),
                  ("nc = 0 and no output", dict(nc_=0, null=cs + ("J", "lam", "P")), outs),
                  ("B = 0 and nc < 0", dict(B_=0, nc_=-1), "B <= 0"), ("nc < 0 and p NULL", dict(nc_=-1, null=("p",)), "nc < 0"),
                  ("Xbar NULL and S0 NULL", dict(null=("Xbar", "S0")), req),
                  ("S0 NULL and no output", dict(null=("S0",) + OUT), s0m),
                  ("no output and ld_W short", dict(null=OUT, ld={"W": lens["W"] - 1}), outs)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error().decode() == msg, (what, dev, L.nmpc_last_error())
    assert all(np.all(arr[k] == 7.0) for k in OUT)  # nothing ran
    # and the handle still works: nc = 0 and P alone without K; then everything
    assert call(nc_=0, null=cs + ("K", "J", "lam")) == 0
    assert np.all(np.isfinite(arr["P"])) and all(np.all(arr[k] == 7.0) for k in ("J", "lam", "dJ", "varJ"))
    assert call() == 0
    full = _run(cv)
    for k in OUT:
        np.testing.assert_array_equal(arr[k], full[k], err_msg=k)


def test_gate_g_python_layer(monkeypatch):
    """policy.expected_cost completes with Tensor.cpu made to raise and adds EJ = J + dJ; a handle whose
    workspace a policy launch has sized keeps its memory_info, a fresh one grows to the header's
    statement (one products-kernel slice per scenario, or the class's own where that is larger) and
    no further; feedback=False agrees with K NULL."""
    import torch
    from nmpc_amd import policy
    from tests.test_gpu_solve_adjoint import _solver

    cv = _val("race_track_2")
    spec, s, B = cv["spec"], cv["s"], cv["B"]
    d, raw = cv["dev"], cv["pol"]["raw"]
    full = _run(cv)
    fresh = _solver(spec)  # a handle that has run nothing else
    mem = fresh.memory_info()
    first = fresh.policy_value_device(d["p"], d["ubar"], raw["X"], raw["K"], S0=cv["dS0"], W=cv["dW"], want=OUT)
    torch.cuda.synchronize()
    after = fresh.memory_info()
    print(f"memory_info of a fresh handle before and after: {mem} / {after}")
    assert mem["ws_bytes"] == 0 and after["ws_bytes"] == B * max(after["ws_per_scenario"], WS_BYTES)
    assert {k: v for k, v in after.items() if k != "ws_bytes"} == {k: v for k, v in mem.items() if k != "ws_bytes"}
    _same({k: v.cpu().numpy() for k, v in first.items()}, full, "a fresh handle")
    fresh.policy_value_device(d["p"], d["ubar"], raw["X"], raw["K"], S0=cv["dS0"], W=cv["dW"], out=first, want=())
    torch.cuda.synchronize()
    assert fresh.memory_info() == after
    mem = s.memory_info()
    assert mem["ws_bytes"] >= B * WS_BYTES

    def boom(*a, **k):
        raise AssertionError("a host round trip in policy.expected_cost")

    dsol = {"x": d["ubar"]}
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        again = policy.expected_cost(s, cv["pol"], dsol, d["p"], cv["dS0"], W=cv["dW"], out=first, want=OUT)
        ol = policy.expected_cost(s, cv["pol"], dsol, d["p"], cv["dS0"], W=cv["dW"], feedback=False, want=OUT)
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    assert all(again[k] is first[k] for k in OUT)
    _same({k: v.cpu().numpy() for k, v in again.items() if k != "EJ"}, full, "policy.expected_cost into its own buffers")
    np.testing.assert_array_equal(again["EJ"].cpu().numpy(), full["J"][:, None] + full["dJ"])
    _same({k: v.cpu().numpy() for k, v in ol.items() if k != "EJ"}, _run(cv, feedback=False), "feedback=False against K NULL")
    default = policy.expected_cost(s, cv["pol"], dsol, d["p"], cv["dS0"], W=cv["dW"])
    torch.cuda.synchronize()
    assert set(default) == {"J", "dJ", "varJ", "EJ"}
