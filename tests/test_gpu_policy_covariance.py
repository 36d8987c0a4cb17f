"""nmpc_policy_covariance_batch / nmpc_policy_covariance_batch_dev (Solver.policy_covariance,
policy_covariance_device, nmpc_amd.policy.covariance): the first-order covariance of the state around
the plan under the feedback policy and the standard deviations of its rows and controls, one wavefront
per (scenario, case), against the NumPy checker of tests/covariance_ref.py (oracle dyn_jac and
obstacle_derivs, one case at a time) and against the rollout kernel itself.

Cases, policies (policy_device) and helpers are tests/test_gpu_policy_rollout.py's: the four solved
cases and the synthetic n1 and n63_16obs, so N = 1, 5, 6, 12, 63, B = 2 ... 4, and uav5's 5 x 5 / 3 x 5
blocks.  nc = 2: case 0 has S0 = 1/2 diag(SIGMA^2) + 1/2 Q Q' / nx and W = 0.01 S0
(covariance_ref.draw_covariances, seed 5), case 1 has S0 = diag(SIGMA^2) and W = 0.

Tolerance of gate (a): Sigma_{k+1} per entry within max(1e-10 a_k, 100 s), a_k = the largest entry
of |Acl_k| |Sigma_k| |Acl_k|' + |W| at the checker's own Sigma_k -- one step's magnitude; the absolute
recursion accumulated over the stages is useless as a scale, the closed loop contracts what the
absolute values do not -- and s the checker's spread under a relative 1e-15 perturbation of S0 and W.
sigma_u^2 and sigma_g^2 likewise against |K_k| |Sigma_k| |K_k|' and |g|' |Sigma_k| |g| + obs_var.  That
the rule is passable is shown on the CPU in the same test: a second fp64 association of the triple
product, and the recursion in long double, are held to PASSABLE of it.  A correct kernel lies no further
from the checker than its own rounding error plus the checker's, each of the size of the long-double
figure, so the rule is passable where that figure stays below PASSABLE = 0.5; the figures are printed.
(Measured: the second order <= 6e-6 everywhere; long double <= 1.4e-5 on Sigma, up to 5.4e-5 on the
variances of the solved cases, and 1e-2 / 0.12 on sigma_u^2 / sigma_g^2 of n63_16obs with W = 0, where
the closed loop has contracted a variance to 1e-21 beside entries of 1e-13 and its own size is the
scale.)  Gate (b) is the CPU test's sigma-point
gate with the rollout kernel as the plant.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import covariance_ref as cr
from tests import policy_ref as pf
from tests.test_gpu_policy_rollout import CASES, SIGMA, _case, _f64  # the cases and policies are shared
from tests.test_gpu_solve_tangent import _dirs, _prep

pytestmark = pytest.mark.gpu

OUT = ("Sigma", "sigma_u", "sigma_g")
NC = 2
EPS = 1e-3       # gate (b): the sigma-point pairs' size
GATE_B = 1e-6    # ... and its bound, relative to max |Sigma_k| per stage
PASSABLE = 0.5


def _draw(prob, B):
    """S0, W (B, NC, nx, nx) of the two cases."""
    nx = prob.nx
    S0a, Wa = cr.draw_covariances(prob, B, SIGMA, seed=5)
    S0b = np.repeat(np.diag(np.asarray(SIGMA[:nx]) ** 2)[None], B, axis=0)
    return np.stack([S0a, S0b], axis=1), np.stack([Wa, np.zeros_like(Wa)], axis=1)


@functools.lru_cache(maxsize=None)
def _cov(name):
    """A case of the rollout tests with its covariances, the checker's result and its spread."""
    c = _case(name)
    prob, B = c["prob"], c["B"]
    S0, W = _draw(prob, B)
    ref = cr.covariance_batch(prob, c["P"], c["ubar"], c["Xbar"], c["K"], S0, W)
    rng = np.random.default_rng(4243)
    per = cr.covariance_batch(prob, c["P"], c["ubar"], c["Xbar"], c["K"], S0 * (1.0 + 1e-15 * rng.standard_normal(S0.shape)),
                              W * (1.0 + 1e-15 * rng.standard_normal(W.shape)))
    spread = {k: np.abs(per[k] - ref[k]) for k in ("Sigma", "var_u", "var_g")}
    return dict(c, S0=S0, W=W, cref=ref, cspread=spread, dS0=_f64(S0), dW=_f64(W))


def _run(cv, want=OUT, feedback=True, noise=True, **over):
    """policy_covariance_device on a case; NumPy results."""
    import torch

    d = dict(cv["dev"], S0=cv["dS0"], W=cv["dW"])
    d.update(over)
    res = cv["s"].policy_covariance_device(d["p"], d["ubar"], d.get("Xbar", cv["pol"]["raw"]["X"]),
                                           d.get("K", cv["pol"]["raw"]["K"]) if feedback else None, d["S0"],
                                           W=d["W"] if noise else None, obs_var=d.get("obs_var"), want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(a, b, what, keys=OUT):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _ratios(got, ref, spread):
    """Largest error / tolerance of Sigma_{k+1}, sigma_u^2 and sigma_g^2 under gate (a)'s rule; `got`
    holds Sigma, var_u, var_g."""
    a = ref["a"][..., None, None]
    figs = {"Sigma": np.abs(got["Sigma"][:, :, 1:] - ref["Sigma"][:, :, 1:]) / np.maximum(1e-10 * a, 100.0 * spread["Sigma"][:, :, 1:])}
    for k, sc in (("var_u", "su"), ("var_g", "sg")):
        tol = np.maximum(1e-10 * ref[sc], 100.0 * spread[k])
        err = np.abs(got[k] - ref[k])
        figs[k] = np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, 1.0) + np.where(tol > 0.0, 0.0, np.inf))
    return {k: float(np.max(v, initial=0.0)) for k, v in figs.items()}


@pytest.mark.parametrize("name", CASES)
def test_gate_a_against_the_checker(name):
    """Sigma, sigma_u^2 and sigma_g^2 of both cases within max(1e-10 x one step's magnitude, 100 s) of
    the checker's; Sigma_0 is S0 bitwise; the rule itself is passable (module docstring)."""
    cv = _cov(name)
    prob, ref, spread = cv["prob"], cv["cref"], cv["cspread"]
    args = (prob, cv["P"], cv["ubar"], cv["Xbar"], cv["K"], cv["S0"], cv["W"])
    for what, alt in (("second fp64 order", cr.covariance_batch(*args, order=1)),
                      ("long double", cr.covariance_batch(*args, dtype=np.longdouble))):
        figs = _ratios({k: np.asarray(alt[k], dtype=np.float64) for k in ("Sigma", "var_u", "var_g")}, ref, spread)
        print(f"{name}: {what} against the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
        assert all(v <= PASSABLE for v in figs.values()), (name, what, figs)
    got = _run(cv)
    assert all(np.all(np.isfinite(got[k])) for k in OUT), name
    np.testing.assert_array_equal(got["Sigma"][:, :, 0], ref["Sigma"][:, :, 0], err_msg="Sigma_0 is S0")
    figs = _ratios({"Sigma": got["Sigma"], "var_u": got["sigma_u"] ** 2, "var_g": got["sigma_g"] ** 2}, ref, spread)
    print(f"{name}: kernel against the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + f"; largest sigma_g {got['sigma_g'].max():.3g}, sigma_u {got['sigma_u'].max():.3g}")
    for k, v in figs.items():
        assert v <= 1.0, (name, k, v)
    # stage 0's box rows: the square root of a copied entry
    nb = prob.nb
    s0 = np.sqrt(np.stack([cv["S0"][:, :, bi, bi] for bi in prob.box_states], axis=-1))
    np.testing.assert_array_equal(got["sigma_g"][:, :, 0, :nb], s0, err_msg="stage 0's box rows")


@pytest.mark.parametrize("name", pf.SOLVED)
def test_gate_b_kernel_against_kernel(name):
    """The sigma-point pairs of S0 and W (case 0) through policy_rollout_device, unclamped: the sums of
    the X and U differences against Sigma_out and sigma_u_out^2 at the CPU test's gate."""
    import torch

    cv = _cov(name)
    prob, B, s = cv["prob"], cv["B"], cv["s"]
    N, nx, nu = prob.N, prob.nx, prob.nu
    M = 2 * nx * (N + 1)
    e0, w = np.zeros((B, M, nx)), np.zeros((B, M, N, nx))
    for b in range(B):
        pts = cr.sigma_points(cv["S0"][b, 0], cv["W"][b, 0], N)
        assert 2 * len(pts) == M
        for i, (j, d) in enumerate(pts):
            for h, sgn in enumerate((1.0, -1.0)):
                if j == 0:
                    e0[b, 2 * i + h] = sgn * EPS * d
                else:
                    w[b, 2 * i + h, j - 1] = sgn * EPS * d
    d = cv["dev"]
    res = s.policy_rollout_device(d["p"], d["ubar"], cv["pol"]["raw"]["X"], cv["pol"]["raw"]["K"], _f64(e0), w=_f64(w),
                                  want=("X", "U"))
    torch.cuda.synchronize()
    X, U = res["X"].cpu().numpy(), res["U"].cpu().numpy()
    dX, dU = (X[:, 0::2] - X[:, 1::2]) / (2.0 * EPS), (U[:, 0::2] - U[:, 1::2]) / (2.0 * EPS)
    Sig, vu = np.einsum("bski,bskj->bkij", dX, dX), np.sum(dU * dU, axis=1)
    got = _run(cv)
    top = np.max(np.abs(Sig), axis=(2, 3))
    fS = float(np.max(np.max(np.abs(Sig - got["Sigma"][:, 0]), axis=(2, 3)) / top))
    fU = float(np.max(np.abs(vu - got["sigma_u"][:, 0] ** 2)) / np.max(np.abs(vu)))
    print(f"{name}: M = {M} rollouts per scenario; |sampled - Sigma_out| / max |Sigma_k| = {fS:.2e}, sigma_u^2 {fU:.2e} "
          f"(gate {GATE_B:.0e})")
    assert M > 64 or name == "uav5"
    assert fS <= GATE_B and fU <= GATE_B, (name, fS, fU)


def test_gate_c_bitwise_properties():
    """Symmetry, repeatability, case splits, ld = 0 sharing, host against device for every subset of
    the outputs, K NULL against K = 0, the unread triangles, and exact zeros."""
    import torch

    for name in ("race_track_2", "uav5"):
        cv = _cov(name)
        B, s = cv["B"], cv["s"]
        full = _run(cv)
        np.testing.assert_array_equal(full["Sigma"], np.swapaxes(full["Sigma"], -1, -2), err_msg="Sigma_k is symmetric")
        _same(_run(cv), full, f"{name}: two calls")
        for c in range(NC):
            one = _run(cv, S0=cv["dS0"][:, c:c + 1].contiguous(), W=cv["dW"][:, c:c + 1].contiguous())
            for k in OUT:
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
        for k in OUT:
            np.testing.assert_array_equal(zero[k], np.zeros_like(zero[k]), err_msg=f"{name}: S0 = 0, W NULL: {k}")
        # ld = 0: scenario 0's inputs shared by B scenarios, against replicated ones
        d, raw = cv["dev"], cv["pol"]["raw"]
        one = {"p": d["p"][0], "ubar": d["ubar"][0], "Xbar": raw["X"][0], "K": raw["K"][0], "S0": cv["dS0"][0], "W": cv["dW"][0]}
        one = {k: v.contiguous() for k, v in one.items()}
        rep = {k: v.unsqueeze(0).expand(B, *v.shape).contiguous() for k, v in one.items()}
        sh = s.policy_covariance_device(rep["p"], one["ubar"], one["Xbar"], one["K"], one["S0"], W=one["W"], want=OUT)
        rp = s.policy_covariance_device(rep["p"], rep["ubar"], rep["Xbar"], rep["K"], rep["S0"], W=rep["W"], want=OUT)
        torch.cuda.synchronize()
        for k in OUT:
            a, r = sh[k].cpu().numpy(), rp[k].cpu().numpy()
            np.testing.assert_array_equal(a, r, err_msg=f"{name}: ld = 0: {k}")
            np.testing.assert_array_equal(a[0], full[k][0], err_msg=f"{name}: ld = 0 against the batch's scenario 0: {k}")
        # every subset of the outputs, host against device entry point
        for n in range(1, len(OUT) + 1):
            for keys in itertools.combinations(OUT, n):
                host = s.policy_covariance(cv["P"], cv["ubar"], cv["Xbar"], cv["K"], cv["S0"], cv["W"], want=keys)
                dev = _run(cv, want=keys)
                assert set(host) == set(dev) == set(keys), keys
                for k in keys:
                    np.testing.assert_array_equal(host[k], full[k], err_msg=f"{name}: host, outputs {keys}: {k}")
                    np.testing.assert_array_equal(dev[k], full[k], err_msg=f"{name}: device, outputs {keys}: {k}")
        print(f"{name}: symmetry, repeatability, case split, K NULL = K 0, unread triangles, zeros, ld = 0 and host = device: bitwise")


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_c_no_write_outside_the_outputs(name):
    """Output buffers carved out of one tensor of sentinels: every entry of them is written, nothing
    outside them is (uav5: blocks of 5 x 5 and runs of 3 controls)."""
    import torch

    cv = _cov(name)
    B, s = cv["B"], cv["s"]
    pad = 64
    shapes = s._covariance_shapes(B, NC)
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    out, o, spans = {}, pad, []
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = big[o:o + n].view(shp)
        spans.append((o, o + n))
        o += n + pad
    d = cv["dev"]
    res = s.policy_covariance_device(d["p"], d["ubar"], cv["pol"]["raw"]["X"], cv["pol"]["raw"]["K"], cv["dS0"], W=cv["dW"],
                                     out=out)
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in OUT)
    h = big.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for a, b in spans:
        keep[a:b] = False
        assert not np.any(h[a:b] == 7.0)
    assert np.all(h[keep] == 7.0)
    _same({k: v.cpu().numpy() for k, v in res.items()}, _run(cv), f"{name}: carved buffers against own ones")


def test_gate_d_obstacle_variance():
    """obs_var adds exactly under the root, for obstacle rows only; `dynamic` takes its centres from p."""
    for name in ("dynamic", "race_track_2"):
        cv = _cov(name)
        prob, B = cv["prob"], cv["B"]
        nb, nobs = prob.nb, prob.n_obs
        if name == "dynamic":
            assert np.any(np.asarray(prob.obs_y_pidx) >= 0)
        ov = 0.25 + np.random.default_rng(17).random((B, nobs))
        base, got = _run(cv), _run(cv, obs_var=_f64(ov))
        _same(got, base, f"{name}: Sigma and sigma_u do not read obs_var", ("Sigma", "sigma_u"))
        np.testing.assert_array_equal(got["sigma_g"][..., :nb], base["sigma_g"][..., :nb], err_msg="box rows")
        ref = cr.covariance_batch(prob, cv["P"], cv["ubar"], cv["Xbar"], cv["K"], cv["S0"], cv["W"], ov)
        add = got["sigma_g"][..., nb:] ** 2 - base["sigma_g"][..., nb:] ** 2 - ov[:, None, None, :]
        tol = 1e-10 * ref["sg"][..., nb:]
        print(f"{name}: sigma_g^2 with obs_var - without - obs_var: largest {np.max(np.abs(add)):.2e} (scale {ref['sg'][..., nb:].max():.3g})")
        assert np.all(np.abs(add) <= tol)
        assert np.all(np.abs(got["sigma_g"] ** 2 - ref["var_g"]) <= np.maximum(1e-10 * ref["sg"], 100.0 * cv["cspread"]["var_g"]))


def test_gate_e_nan_handling():
    """A NaN in one case's S0 stays in that case; a scenario whose policy is NaN (info != 0: lbx > ubx
    through policy_device) gives NaN Sigma_k (k >= 1) and sigma_u beside bitwise-untouched neighbours."""
    import torch

    cv = _cov("race_track_2")
    spec, s, B, P, bounds, sol = cv["spec"], cv["s"], cv["B"], cv["P"], cv["bounds"], cv["sol"]
    full = _run(cv)
    S0 = cv["dS0"].clone()
    S0[1, 0, 0, 2] = float("nan")  # entry (2, 0): read
    got = _run(cv, S0=S0)
    assert np.all(np.isnan(got["Sigma"][1, 0, 1:]))
    assert np.isnan(got["Sigma"][1, 0, 0, 0, 2]) and np.isnan(got["Sigma"][1, 0, 0, 2, 0])
    assert np.any(np.isnan(got["sigma_u"][1, 0])) and not np.any(np.isnan(got["sigma_u"][1, 1]))
    for k in OUT:
        a, f = got[k].copy(), full[k].copy()
        a[1, 0], f[1, 0] = 0.0, 0.0
        np.testing.assert_array_equal(a, f, err_msg=f"NaN in S0 of (1, 0): {k}")
    # an invalid scenario's policy
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in bounds[:2])
    lb3[5, 1] = ub3[5, 1] + 1.0
    dsol, db, dP, _, _ = _prep(spec, sol, (lb3, ub3, bounds[2], bounds[3]), P, np.zeros((spec.np, 1)), B, 1, keys=(),
                               g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, None)
    torch.cuda.synchronize()
    assert pol["info"].cpu().numpy().tolist() == [0, -11] + [0] * (B - 2)
    got = _run(cv, K=pol["raw"]["K"], Xbar=pol["raw"]["X"])
    assert np.all(np.isnan(got["Sigma"][1, :, 1:])) and np.all(np.isnan(got["sigma_u"][1]))
    for k in OUT:
        np.testing.assert_array_equal(np.delete(got[k], 1, axis=0), np.delete(full[k], 1, axis=0), err_msg=k)


def test_gate_f_argument_validation_on_a_live_handle():
    """Every rule of the header from both entry points, with its full message, before any device call:
    nothing is written, and the handle still works.  Calls that break two rules get the earlier one's."""
    from nmpc_amd import _lib
    from tests.test_gpu_solve_adjoint import _solver

    cv = _cov("race_track_2")
    spec, s, B = cv["spec"], cv["s"], cv["B"]
    N, nu, nx = spec.N, spec.nw // spec.N, spec.nX // (spec.N + 1)
    L = _lib.lib()
    arr = {"p": cv["P"], "ubar": cv["ubar"], "Xbar": cv["Xbar"], "K": np.swapaxes(cv["K"], 2, 3), "S0": cv["S0"],
           "W": cv["W"], "obs_var": np.full((B, spec.n_obs), 0.5)}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    names = tuple(arr)
    lens = dict(zip(names, (spec.np, spec.nw, spec.nX, nu * nx * N, nx * nx * NC, nx * nx * NC, spec.n_obs)))
    shapes = s._covariance_shapes(B, NC)
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
        return L.nmpc_policy_covariance_batch_dev(*args, vp(0)) if dev else L.nmpc_policy_covariance_batch(*args)

    req, ldm = "required pointer is null (p, ubar, Xbar, S0)", "leading dimension smaller than the vector length"
    outs = "Sigma_out, sigma_u_out and sigma_g_out are all null"
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("nc = 0", dict(nc_=0), "nc <= 0"),
                 ("nc < 0", dict(nc_=-1), "nc <= 0"), ("nc too large", dict(nc_=65536), "nc > 65535"),
                 ("every output NULL", dict(null=OUT), outs), ("ld_p negative", dict(ld={"p": -spec.np}), ldm),
                 ("ld_S0 one case", dict(ld={"S0": nx * nx}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in ("p", "ubar", "Xbar", "S0")]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and nc = 0", dict(B_=0, nc_=0), "B <= 0"), ("nc = 0 and p NULL", dict(nc_=0, null=("p",)), "nc <= 0"),
                  ("S0 NULL and no output", dict(null=("S0",) + OUT), req),
                  ("no output and ld_W short", dict(null=OUT, ld={"W": lens["W"] - 1}), outs)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error().decode() == msg, (what, dev, L.nmpc_last_error())
    assert all(np.all(arr[k] == 7.0) for k in OUT)  # nothing ran
    # obs_var on a problem without obstacles
    from nmpc_amd import make_spec

    s0 = _solver(make_spec(None, N=spec.N, T=0.2))
    assert s0.spec.n_obs == 0 and s0.spec.np == spec.np
    for dev in (False, True):
        rc = call(h=s0._h, dev=dev)
        assert rc == -1 and L.nmpc_last_error().decode() == "obs_var given for a problem without obstacles", dev
        assert call(h=s0._h, dev=dev, null=("obs_var",) + OUT) == -1 and L.nmpc_last_error().decode() == outs
    assert all(np.all(arr[k] == 7.0) for k in OUT)
    # and the handle still works: sigma_g alone without K, W or obs_var; then everything
    assert call(null=("K", "W", "obs_var", "Sigma", "sigma_u")) == 0
    assert np.all(np.isfinite(arr["sigma_g"])) and all(np.all(arr[k] == 7.0) for k in ("Sigma", "sigma_u"))
    assert call(null=("obs_var",)) == 0
    full = _run(cv)
    for k in OUT:
        np.testing.assert_array_equal(arr[k], full[k], err_msg=k)


def test_gate_g_python_layer(monkeypatch):
    """policy.covariance completes with Tensor.cpu made to raise; memory_info is unchanged on a handle
    that has run nothing else; policy.covariance with coefficients c equals the checker fed
    ubar = u* + sum_d kff^(d) c_d formed in NumPy; policy.tighten moves the solve's bounds on the device."""
    import torch
    from nmpc_amd import policy
    from tests.test_gpu_solve_adjoint import _solver

    cv = _cov("race_track_2")
    spec, s, B, P, bounds, sol = cv["spec"], cv["s"], cv["B"], cv["P"], cv["bounds"], cv["sol"]
    d, raw = cv["dev"], cv["pol"]["raw"]
    full = _run(cv)
    fresh = _solver(spec)  # a handle that has run nothing else
    mem = fresh.memory_info()
    first = fresh.policy_covariance_device(d["p"], d["ubar"], raw["X"], raw["K"], cv["dS0"], W=cv["dW"], want=OUT)
    torch.cuda.synchronize()
    print(f"memory_info of a fresh handle before and after: {mem} / {fresh.memory_info()}")
    assert fresh.memory_info() == mem
    _same({k: v.cpu().numpy() for k, v in first.items()}, full, "a fresh handle")
    mem = s.memory_info()

    def boom(*a, **k):
        raise AssertionError("a host round trip in policy.covariance")

    dsol = {"x": d["ubar"]}
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        again = policy.covariance(s, cv["pol"], dsol, d["p"], cv["dS0"], W=cv["dW"], out=first, want=OUT)
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    assert all(again[k] is first[k] for k in OUT)
    _same({k: v.cpu().numpy() for k, v in again.items()}, full, "policy.covariance into its own buffers")
    # the feedforward: a parameter move along two directions
    nd = 2
    dp = _dirs(spec, B, nd, 97)
    dsol2, db, dP, dd, _ = _prep(spec, sol, bounds, P, dp, B, nd, keys=(), g=False, rep=False)
    pol = s.policy_device(dsol2, *db, dP, dd)
    coef = 0.05 * np.random.default_rng(99).standard_normal((B, nd))
    Pm = P + np.einsum("bd,pdb->bp", coef, dp)
    got = policy.covariance(s, pol, dsol2, _f64(Pm), cv["dS0"], W=cv["dW"], c=_f64(coef), want=OUT)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    kff = pol["kff"].cpu().numpy()
    ubar = cv["ubar"] + np.einsum("bdn,bd->bn", kff.reshape(B, nd, -1), coef)
    args = (cv["prob"], Pm, ubar, pol["X"].cpu().numpy(), pol["K"].cpu().numpy())
    ref = cr.covariance_batch(*args, cv["S0"], cv["W"])
    rng = np.random.default_rng(4243)
    per = cr.covariance_batch(*args, cv["S0"] * (1.0 + 1e-15 * rng.standard_normal(cv["S0"].shape)),
                              cv["W"] * (1.0 + 1e-15 * rng.standard_normal(cv["W"].shape)))
    figs = _ratios({"Sigma": got["Sigma"], "var_u": got["sigma_u"] ** 2, "var_g": got["sigma_g"] ** 2}, ref,
                   {k: np.abs(per[k] - ref[k]) for k in ("Sigma", "var_u", "var_g")})
    print("policy.covariance with c: error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert all(v <= 1.0 for v in figs.values()), figs
    ol = policy.covariance(s, pol, dsol2, _f64(Pm), cv["dS0"], W=cv["dW"], c=_f64(coef), feedback=False, want=("sigma_u",))
    torch.cuda.synchronize()
    assert torch.all(ol["sigma_u"] == 0.0)
    # tighten on the device: lower <= upper, finite bounds moved by kappa sigma
    cov = {k: _f64(v) for k, v in full.items()}
    nlx, nux, nlg, nug = policy.tighten(d["lbx"], d["ubx"], d["lbg"], d["ubg"], cov, 2.0, case=1)
    torch.cuda.synchronize()
    assert nlx.shape == nux.shape == (B, spec.nw) and nlg.shape == nug.shape == (B, spec.ng)
    assert bool(torch.all(nlx <= nux)) and bool(torch.all(nlg <= nug))
    moved = (nug < d["ubg"]).sum().item()
    print(f"tighten: {moved} of {nug.numel()} upper row bounds moved inwards")
    assert moved > 0
