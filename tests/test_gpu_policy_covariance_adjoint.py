"""nmpc_policy_covariance_adjoint_batch / nmpc_policy_covariance_adjoint_batch_dev
(Solver.policy_covariance_adjoint, policy_covariance_adjoint_device, nmpc_amd.policy.covariance_grad,
nmpc_amd.autograd.policy_covariance): the reverse sweep of the policy covariance, one wavefront per
(scenario, case), against the NumPy checker of tests/covariance_adjoint_ref.py (oracle dyn_jac, dyn_hess
and obstacle_derivs, one case at a time) and against the forward kernel itself.

Cases, policies (policy_device), covariances and helpers are tests/test_gpu_policy_rollout.py's and
tests/test_gpu_policy_covariance.py's: the four solved cases and the synthetic n1 and n63_16obs, so
N = 1, 5, 6, 12, 63, B = 2 ... 4, uav5's 5 x 5 / 3 x 5 blocks, 16 obstacles, and `dynamic`'s centres from p;
nc = 2.  Sigma is the forward kernel's Sigma_out.  The seeds Sb (asymmetric), ub and gb are N(0, 1), seed
811; obs_var is drawn in [0.25, 1.25), seed 17.

Gate (a), against the checker: Lambda_k per entry within max(1e-10 a_k, 100 s) -- the forward gate's
constants -- with a_k the largest entry of |Acl_k|' |Lam_{k+1}| |Acl_k| plus the absolute seed terms at the
checker's own Lam_{k+1}, and s the checker's spread under a relative 1e-15 perturbation of Sigma and the
seeds; K_bar, ubar_bar and Xbar_bar per stage likewise against the absolute-value version of their own
formula; W_bar, obs_var_bar and p_bar against the sum of their stages' absolute terms.  That the rule is
passable is shown on the CPU in the same test: a second fp64 association and long double are each held
to PASSABLE = 0.5 of it.  Where a quantity of a case does not pass that, the kernel is held, for that
quantity of that case, to 3 x the long-double figure instead of 1 (FALLBACK lists them, each with its
measured long-double figure; no other quantity may use it).  Measured: FALLBACK is empty -- the second
order stays <= 7.3e-4 and long double <= 1.2e-3 of the rule (K_bar of n63_16obs; Lambda <= 6.7e-4, the
others <= 1.4e-4), and the kernel lies <= 9.5e-4 from the checker (K_bar of race_track_2; Lambda <= 2.4e-4).
Gate (b), kernel against kernel: <Sb, Sigma_out> + <ub, sigma_u^2> + <gb, sigma_g^2> of the forward launch
against <S0_bar, S0> + <W_bar, W> + <obs_var_bar, obs_var>; the map is linear in the three, so the sides
agree to rounding.  The figure is |difference| / sum of the absolute terms of both sides.  Measured:
<= 7.7e-17 over the 36 (scenario, case) pairs (sums of a few thousand terms with cancellation); the gate is
10 x that.
Gate (c), kernel against kernel: central differences of the forward launch along one direction each
of K and ubar against <K_bar, dK> and <ubar_bar, dubar>, at the CPU test's eps and gates.  Measured: K
<= 2.6e-8 (gate 7.6e-8), ubar <= 1.3e-7 (gate 1.3e-6).
Gates (d) to (g) as their tests' docstrings say.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import covariance_adjoint_ref as ar
from tests import test_covariance_adjoint_capi as cc
from tests import test_gpu_policy_covariance as fc
from tests.test_gpu_policy_covariance import NC, _cov
from tests.test_gpu_policy_rollout import CASES, _f64
from tests.test_gpu_solve_tangent import _prep

pytestmark = pytest.mark.gpu

OUT = ar.OUT
SCALE = {"Lambda": "aL", "K_bar": "aK", "ubar_bar": "aU", "Xbar_bar": "aX", "W_bar": "aW", "obs_var_bar": "aO", "p_bar": "aP"}
PASSABLE = 0.5
# (case, quantity): the long-double figure where the rule of gate (a) is not passable (module docstring)
FALLBACK = {}
GATE_B = 7.7e-16  # 10 x the largest figure measured (module docstring)


@functools.lru_cache(maxsize=None)
def _adj(name):
    """A case of the covariance tests with the forward kernel's result, the seeds, the checker's
    gradient and its spread."""
    cv = _cov(name)
    prob, B = cv["prob"], cv["B"]
    N, nx, nu, m = prob.N, prob.nx, prob.nu, prob.m
    ov = 0.25 + np.random.default_rng(17).random((B, prob.n_obs)) if prob.n_obs else None
    fwd = fc._run(cv, want=fc.OUT, **({} if ov is None else {"obs_var": _f64(ov)}))
    rng = np.random.default_rng(811)
    seeds = {"Sb": rng.standard_normal((B, NC, N + 1, nx, nx)), "ub": rng.standard_normal((B, NC, N, nu)),
             "gb": rng.standard_normal((B, NC, N + 1, m))}
    args = (prob, cv["P"], cv["ubar"], cv["Xbar"], cv["K"])
    ref = ar.adjoint_batch(*args, fwd["Sigma"], seeds["Sb"], seeds["ub"], seeds["gb"])
    rng = np.random.default_rng(4243)
    wob = lambda a: a * (1.0 + 1e-15 * rng.standard_normal(a.shape))  # noqa: E731
    per = ar.adjoint_batch(*args, wob(fwd["Sigma"]), wob(seeds["Sb"]), wob(seeds["ub"]), wob(seeds["gb"]))
    spread = {k: np.abs(per[k] - ref[k]) for k in OUT}
    dev = {"Sigma": _f64(fwd["Sigma"]), "Sb": _f64(seeds["Sb"]), "ub": _f64(seeds["ub"]), "gb": _f64(seeds["gb"])}
    return dict(cv, ov=ov, fwd=fwd, seeds=seeds, aref=ref, aspread=spread, adev=dev, args=args)


def _np(res, prob, B):
    """Device results as NumPy arrays in the checker's shapes."""
    out = {k: v.cpu().numpy() for k, v in res.items()}
    if "K_bar" in out:
        out["K_bar"] = np.ascontiguousarray(np.swapaxes(out["K_bar"], -1, -2))
    if "ubar_bar" in out:
        out["ubar_bar"] = out["ubar_bar"].reshape(B, -1, prob.N, prob.nu)
    return out


def _run(ad, want=OUT, feedback=True, **over):
    """policy_covariance_adjoint_device on a case; NumPy results in the checker's shapes."""
    import torch

    d = dict(ad["dev"], **ad["adev"])
    d.update(over)
    if ad["prob"].n_obs == 0:
        want = tuple(k for k in want if k != "obs_var_bar")
    if not feedback:
        want = tuple(k for k in want if k != "K_bar")
    res = ad["s"].policy_covariance_adjoint_device(
        d["p"], d["ubar"], d.get("Xbar", ad["pol"]["raw"]["X"]), d.get("K", ad["pol"]["raw"]["K"]) if feedback else None,
        d["Sigma"], Sigma_bar=d["Sb"], var_u_bar=d["ub"], var_g_bar=d["gb"], want=want)
    torch.cuda.synchronize()
    return _np(res, ad["prob"], ad["B"])


def _same(a, b, what, keys=None):
    for k in (keys or a.keys()):
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _ratios(got, ref, spread):
    """Largest error / tolerance of every quantity under gate (a)'s rule."""
    figs = {}
    for k, sc in SCALE.items():
        if k not in got:
            continue
        a = ref[sc][..., None, None] if k == "Lambda" else ref[sc]
        tol = np.maximum(1e-10 * a, 100.0 * spread[k])
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref[k])
        r = np.where(err == 0.0, 0.0, err / np.where(tol > 0.0, tol, 1.0) + np.where(tol > 0.0, 0.0, np.inf))
        figs[k] = float(np.max(r, initial=0.0))
    return figs


@pytest.mark.parametrize("name", CASES)
def test_gate_a_against_the_checker(name):
    """Every output of both cases within gate (a)'s rule of the checker's; S0_bar is Lambda's block 0."""
    ad = _adj(name)
    ref, spread = ad["aref"], ad["aspread"]
    sd = ad["seeds"]
    alt = {}
    for what, kw in (("second fp64 order", dict(order=1)), ("long double", dict(dtype=np.longdouble))):
        r = ar.adjoint_batch(*ad["args"], ad["fwd"]["Sigma"], sd["Sb"], sd["ub"], sd["gb"], **kw)
        alt[what] = _ratios(r, ref, spread)
        print(f"{name}: {what} against the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in alt[what].items()))
    limit = {}
    for k in alt["long double"]:
        worst = max(alt["long double"][k], alt["second fp64 order"][k])
        if (name, k) in FALLBACK:
            limit[k] = 3.0 * max(FALLBACK[(name, k)], alt["long double"][k])
            print(f"{name}: {k}: the rule is not passable here (long double {alt['long double'][k]:.2e}); the kernel is held to {limit[k]:.2e}")
            assert worst > PASSABLE, (name, k, "passable after all: take it out of FALLBACK")
        else:
            limit[k] = 1.0
            assert worst <= PASSABLE, (name, k, alt)
    got = _run(ad)
    assert all(np.all(np.isfinite(v)) for v in got.values()), name
    figs = _ratios(got, ref, spread)
    print(f"{name}: kernel against the checker, error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    np.testing.assert_array_equal(got["S0_bar"], got["Lambda"][:, :, 0], err_msg="S0_bar is Lambda's block 0")
    for k, v in figs.items():
        assert v <= limit[k], (name, k, v, limit[k])


def _forward_loss(ad, **over):
    """L per (scenario, case) from one forward launch."""
    kw = {} if ad["ov"] is None else {"obs_var": _f64(ad["ov"])}
    kw.update(over)
    f = fc._run(ad, want=fc.OUT, **kw)
    sd = ad["seeds"]
    terms = (sd["Sb"] * f["Sigma"], sd["ub"] * f["sigma_u"] ** 2, sd["gb"] * f["sigma_g"] ** 2)
    val = sum(t.reshape(t.shape[0], t.shape[1], -1).sum(-1) for t in terms)
    mag = sum(np.abs(t).reshape(t.shape[0], t.shape[1], -1).sum(-1) for t in terms)
    return val, mag


@pytest.mark.parametrize("name", CASES)
def test_gate_b_linear_inputs_kernel_against_kernel(name):
    """The forward launch's loss against <S0_bar, S0> + <W_bar, W> + <obs_var_bar, obs_var>."""
    ad = _adj(name)
    got = _run(ad, want=("S0_bar", "W_bar", "obs_var_bar"))
    lhs, mag = _forward_loss(ad)
    S0, W = ad["S0"], ad["W"]
    terms = [got["S0_bar"] * S0, got["W_bar"] * W]
    if ad["ov"] is not None:
        terms.append(got["obs_var_bar"] * ad["ov"][:, None, :])
    rhs = sum(t.reshape(t.shape[0], t.shape[1], -1).sum(-1) for t in terms)
    mag = mag + sum(np.abs(t).reshape(t.shape[0], t.shape[1], -1).sum(-1) for t in terms)
    fig = np.abs(lhs - rhs) / mag
    print(f"{name}: |forward loss - <gradient, (S0, W, obs_var)>| / sum of absolute terms, per (scenario, case): "
          + " ".join(f"{v:.1e}" for v in fig.ravel()) + f"  (gate {GATE_B:.0e})")
    assert np.all(fig <= GATE_B), (name, fig)


@pytest.mark.parametrize("name", CASES)
def test_gate_c_nonlinear_inputs_kernel_against_kernel(name):
    """Central differences of the forward launch along one direction each of K and ubar against
    <K_bar, dK> and <ubar_bar, dubar>, per scenario (summed over its cases), at the CPU test's gates."""
    import torch

    ad = _adj(name)
    B, prob = ad["B"], ad["prob"]
    got = _run(ad, want=("K_bar", "ubar_bar"))
    rng = np.random.default_rng(913)
    raw = ad["pol"]["raw"]
    dK = rng.standard_normal(ad["K"].shape)             # (B, N, nu, nx)
    du = rng.standard_normal((B, prob.N, prob.nu))
    dKraw = _f64(np.swapaxes(dK, -1, -2))               # the kernel's column-major blocks
    for grp, an in (("K", np.sum(got["K_bar"] * dK[:, None], axis=(1, 2, 3, 4))),
                    ("ubar", np.sum(got["ubar_bar"] * du[:, None], axis=(1, 2, 3)))):
        eps, gate = cc.GATE[grp]
        val = []
        for sgn in (1.0, -1.0):
            over = ({"K": (raw["K"] + sgn * eps * dKraw).contiguous()} if grp == "K"
                    else {"ubar": (ad["dev"]["ubar"] + sgn * eps * _f64(du.reshape(B, -1))).contiguous()})
            val.append(_forward_loss(ad, **over)[0].sum(1))
        torch.cuda.synchronize()
        fd = (val[0] - val[1]) / (2.0 * eps)
        fig = np.abs(fd - an) / np.maximum(np.abs(fd), np.abs(an))
        print(f"{name}: {grp}: |central difference - <gradient, direction>| / larger, per scenario: "
              + " ".join(f"{v:.1e}" for v in fig) + f"  (eps {eps:.0e}, gate {gate:.1e})")
        assert np.all(fig <= gate), (name, grp, fig)


def test_gate_d_bitwise_properties():
    """Symmetry, S0_bar and W_bar against Lambda's blocks, repeatability, case splits, ld = 0 sharing, host
    against device for every subset of the outputs, K NULL against K = 0, the unread triangle, zero
    seeds, and p_bar outside the obstacle centres."""
    import torch

    for name in ("race_track_2", "uav5", "dynamic"):
        ad = _adj(name)
        B, s, prob = ad["B"], ad["s"], ad["prob"]
        keys = tuple(k for k in OUT if not (k == "obs_var_bar" and prob.n_obs == 0))
        full = _run(ad)
        np.testing.assert_array_equal(full["Lambda"], np.swapaxes(full["Lambda"], -1, -2), err_msg="Lambda_k is symmetric")
        np.testing.assert_array_equal(full["S0_bar"], full["Lambda"][:, :, 0], err_msg="S0_bar")
        acc = full["Lambda"][:, :, prob.N].copy()
        for k in range(prob.N - 1, 0, -1):  # the kernel's order: Lam_N, Lam_{N-1}, ..., Lam_1
            acc = acc + full["Lambda"][:, :, k]
        np.testing.assert_array_equal(full["W_bar"], acc, err_msg="W_bar is the sum of Lambda's blocks N ... 1")
        _same(_run(ad), full, f"{name}: two calls")
        d = ad["adev"]
        for c in range(NC):
            one = _run(ad, **{k: d[k][:, c:c + 1].contiguous() for k in d})
            for k in keys:
                np.testing.assert_array_equal(one[k][:, 0], full[k][:, c], err_msg=f"{name}: nc = 1, case {c}: {k}")
        centres = {int(q) for q in list(prob.obs_x_pidx) + list(prob.obs_y_pidx) if q >= 0}
        off = [q for q in range(prob.np_) if q not in centres]
        assert np.all(full["p_bar"][..., off] == 0.0), name
        if name == "dynamic":
            assert centres and np.all(full["p_bar"][..., sorted(centres)] != 0.0)
        if name == "dynamic":
            continue
        nok = tuple(k for k in keys if k != "K_bar")
        _same(_run(ad, want=nok, feedback=False), _run(ad, want=nok, K=torch.zeros_like(ad["pol"]["raw"]["K"])),
              f"{name}: K NULL against K = 0", nok)
        # the blocks are column-major: entry (i, j) with i < j sits at [..., j, i], below the tensor's diagonal
        nx = prob.nx
        low = torch.tril(torch.ones((nx, nx), dtype=torch.bool, device="cuda"), -1)
        Sn = d["Sigma"].clone()
        Sn[..., low] = float("nan")
        _same(_run(ad, Sigma=Sn), full, f"{name}: NaN in the unread triangle of Sigma")
        zero = _run(ad, Sb=torch.zeros_like(d["Sb"]), ub=torch.zeros_like(d["ub"]), gb=torch.zeros_like(d["gb"]))
        for k in keys:
            np.testing.assert_array_equal(zero[k], np.zeros_like(zero[k]), err_msg=f"{name}: zero seeds: {k}")
        # ld = 0: scenario 0's inputs shared by B scenarios, against replicated ones
        dv, raw = ad["dev"], ad["pol"]["raw"]
        one = {"p": dv["p"][0], "ubar": dv["ubar"][0], "Xbar": raw["X"][0], "K": raw["K"][0], "Sigma": d["Sigma"][0],
               "Sb": d["Sb"][0], "ub": d["ub"][0], "gb": d["gb"][0]}
        one = {k: v.contiguous() for k, v in one.items()}
        rep = {k: v.unsqueeze(0).expand(B, *v.shape).contiguous() for k, v in one.items()}
        call = lambda q, p: s.policy_covariance_adjoint_device(p, q["ubar"], q["Xbar"], q["K"], q["Sigma"], Sigma_bar=q["Sb"],  # noqa: E731
                                                               var_u_bar=q["ub"], var_g_bar=q["gb"], want=keys)
        sh, rp = call(one, rep["p"]), call(rep, rep["p"])
        torch.cuda.synchronize()
        sh, rp = _np(sh, prob, B), _np(rp, prob, B)
        for k in keys:
            np.testing.assert_array_equal(sh[k], rp[k], err_msg=f"{name}: ld = 0: {k}")
            np.testing.assert_array_equal(sh[k][0], full[k][0], err_msg=f"{name}: ld = 0 against the batch's scenario 0: {k}")
        # every subset of the outputs, host against device entry point
        sd = ad["seeds"]
        for n in range(1, len(keys) + 1):
            for sub in itertools.combinations(keys, n):
                host = s.policy_covariance_adjoint(ad["P"], ad["ubar"], ad["Xbar"], ad["K"], ad["fwd"]["Sigma"], sd["Sb"],
                                                   sd["ub"], sd["gb"], want=sub)
                host["ubar_bar"] = host["ubar_bar"].reshape(B, NC, prob.N, prob.nu) if "ubar_bar" in host else None
                dev = _run(ad, want=sub)
                assert set(k for k, v in host.items() if v is not None) == set(dev) == set(sub), sub
                for k in sub:
                    np.testing.assert_array_equal(host[k], full[k], err_msg=f"{name}: host, outputs {sub}: {k}")
                    np.testing.assert_array_equal(dev[k], full[k], err_msg=f"{name}: device, outputs {sub}: {k}")
        print(f"{name}: symmetry, S0_bar, W_bar, repeatability, case split, K NULL = K 0, unread triangle, zero seeds, ld = 0 "
              "and host = device: bitwise")


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_d_no_write_outside_the_outputs(name):
    """Output buffers carved out of one tensor of sentinels: every entry of them is written, nothing
    outside them is (uav5: blocks of 5 x 5 and runs of 3 controls)."""
    import torch

    ad = _adj(name)
    B, s, prob = ad["B"], ad["s"], ad["prob"]
    pad = 64
    shapes = {k: v for k, v in s._covariance_adjoint_shapes(B, NC).items() if int(np.prod(v)) > 0}
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    out, o, spans = {}, pad, []
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = big[o:o + n].view(shp)
        spans.append((o, o + n))
        o += n + pad
    d, a = ad["dev"], ad["adev"]
    res = s.policy_covariance_adjoint_device(d["p"], d["ubar"], ad["pol"]["raw"]["X"], ad["pol"]["raw"]["K"], a["Sigma"],
                                             Sigma_bar=a["Sb"], var_u_bar=a["ub"], var_g_bar=a["gb"], out=out, want=())
    torch.cuda.synchronize()
    assert all(res[k] is out[k] for k in shapes)
    h = big.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for lo, hi in spans:
        keep[lo:hi] = False
        assert not np.any(h[lo:hi] == 7.0)
    assert np.all(h[keep] == 7.0)
    _same(_np(res, prob, B), _run(ad), f"{name}: carved buffers against own ones")


def test_gate_e_nan_handling():
    """A NaN in one case's seeds stays in that case; a scenario whose policy is NaN (info != 0: lbx > ubx
    through policy_device) leaves its neighbours bitwise untouched."""
    import torch

    ad = _adj("race_track_2")
    spec, s, B, P, bounds, sol = ad["spec"], ad["s"], ad["B"], ad["P"], ad["bounds"], ad["sol"]
    full = _run(ad)
    gb = ad["adev"]["gb"].clone()
    gb[1, 0, 2, 1] = float("nan")
    got = _run(ad, gb=gb)
    assert np.all(np.isnan(got["S0_bar"][1, 0])) and not np.any(np.isnan(got["S0_bar"][1, 1]))
    for k in OUT:
        a, f = got[k].copy(), full[k].copy()
        a[1, 0], f[1, 0] = 0.0, 0.0
        np.testing.assert_array_equal(a, f, err_msg=f"NaN in gb of (1, 0): {k}")
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in bounds[:2])
    lb3[5, 1] = ub3[5, 1] + 1.0
    dsol, db, dP, _, _ = _prep(spec, sol, (lb3, ub3, bounds[2], bounds[3]), P, np.zeros((spec.np, 1)), B, 1, keys=(),
                               g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, None)
    torch.cuda.synchronize()
    assert pol["info"].cpu().numpy().tolist() == [0, -11] + [0] * (B - 2)
    got = _run(ad, K=pol["raw"]["K"], Xbar=pol["raw"]["X"])
    assert np.all(np.isnan(got["K_bar"][1])) and np.all(np.isnan(got["S0_bar"][1]))
    for k in OUT:
        np.testing.assert_array_equal(np.delete(got[k], 1, axis=0), np.delete(full[k], 1, axis=0), err_msg=k)


def test_gate_f_argument_validation_on_a_live_handle():
    """Every rule of the header from both entry points, with its full message, before any device call:
    nothing is written, and the handle still works.  Calls that break two rules get the earlier one's."""
    from nmpc_amd import _lib, make_spec
    from tests.test_gpu_solve_adjoint import _solver

    ad = _adj("race_track_2")
    spec, s, B, prob = ad["spec"], ad["s"], ad["B"], ad["prob"]
    N, nu, nx = prob.N, prob.nu, prob.nx
    L = _lib.lib()
    sd = ad["seeds"]
    arr = {"p": ad["P"], "ubar": ad["ubar"], "Xbar": ad["Xbar"], "K": np.swapaxes(ad["K"], 2, 3), "Sigma": ad["fwd"]["Sigma"],
           "Sigma_bar": sd["Sb"], "var_u_bar": sd["ub"], "var_g_bar": sd["gb"]}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    names = tuple(arr)
    nS = nx * nx * (N + 1) * NC
    lens = dict(zip(names, (spec.np, spec.nw, spec.nX, nu * nx * N, nS, nS, spec.nw * NC, spec.ng * NC)))
    shapes = s._covariance_adjoint_shapes(B, NC)
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
        if dev:
            return L.nmpc_policy_covariance_adjoint_batch_dev(*args, vp(0))
        return L.nmpc_policy_covariance_adjoint_batch(*args)

    req, ldm = "required pointer is null (p, ubar, Xbar, Sigma)", "leading dimension smaller than the vector length"
    seedm = "every seed pointer is null (Sigma_bar, var_u_bar, var_g_bar)"
    outs = ("S0_bar_out, W_bar_out, Lambda_out, obs_var_bar_out, K_bar_out, ubar_bar_out, Xbar_bar_out and p_bar_out "
            "are all null")
    seeds = ("Sigma_bar", "var_u_bar", "var_g_bar")
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("nc = 0", dict(nc_=0), "nc <= 0"),
                 ("nc < 0", dict(nc_=-1), "nc <= 0"), ("nc too large", dict(nc_=65536), "nc > 65535"),
                 ("every seed NULL", dict(null=seeds), seedm), ("every output NULL", dict(null=OUT), outs),
                 ("K_bar without K", dict(null=("K",)), "K_bar_out needs K"),
                 ("ld_p negative", dict(ld={"p": -spec.np}), ldm), ("ld_Sigma one case", dict(ld={"Sigma": nS // NC}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in ("p", "ubar", "Xbar", "Sigma")]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and nc = 0", dict(B_=0, nc_=0), "B <= 0"), ("nc = 0 and p NULL", dict(nc_=0, null=("p",)), "nc <= 0"),
                  ("Sigma NULL and no seed", dict(null=("Sigma",) + seeds), req),
                  ("no seed and no output", dict(null=seeds + OUT), seedm),
                  ("no output and K NULL", dict(null=OUT + ("K",)), outs),
                  ("K_bar without K and ld_ubar short", dict(null=("K",), ld={"ubar": lens["ubar"] - 1}), "K_bar_out needs K")]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error().decode() == msg, (what, dev, L.nmpc_last_error())
    assert all(np.all(arr[k] == 7.0) for k in OUT)  # nothing ran
    # obs_var_bar_out on a problem without obstacles
    s0 = _solver(make_spec(None, N=spec.N, T=0.2))
    assert s0.spec.n_obs == 0 and s0.spec.np == spec.np
    for dev in (False, True):
        rc = call(h=s0._h, dev=dev)
        assert rc == -1 and L.nmpc_last_error().decode() == "obs_var_bar_out asked for on a problem without obstacles", dev
        assert call(h=s0._h, dev=dev, null=("K",)) == -1 and L.nmpc_last_error().decode() == "K_bar_out needs K"
    assert all(np.all(arr[k] == 7.0) for k in OUT)
    # and the handle still works: S0_bar alone from the seed on Sigma alone, without K; then everything
    only = tuple(k for k in OUT if k != "S0_bar")
    assert call(null=("K", "var_u_bar", "var_g_bar") + only) == 0
    assert np.all(np.isfinite(arr["S0_bar"])) and all(np.all(arr[k] == 7.0) for k in only)
    assert call() == 0
    full = _run(ad)
    arr["K_bar"] = np.swapaxes(arr["K_bar"], -1, -2)
    arr["ubar_bar"] = arr["ubar_bar"].reshape(B, NC, N, nu)
    for k in OUT:
        np.testing.assert_array_equal(arr[k], full[k], err_msg=k)


def test_gate_g_python_layer(monkeypatch):
    """torch.autograd through autograd.policy_covariance and policy.tighten equals the covariance_grad
    route; the S0 gradient has the lower-triangle fold; S0 = 0 with W None gives finite (zero) gradients
    through the square root; nothing is read back (Tensor.cpu made to raise); memory_info is unchanged."""
    import torch
    from nmpc_amd import autograd, policy

    ad = _adj("dynamic")
    s, B, prob = ad["s"], ad["B"], ad["prob"]
    d, raw, pol = ad["dev"], ad["pol"]["raw"], ad["pol"]
    nx = prob.nx
    mem = s.memory_info()
    leaf = {"p": d["p"], "ubar": d["ubar"], "Xbar": raw["X"], "K": raw["K"], "S0": ad["dS0"], "W": ad["dW"], "obs_var": _f64(ad["ov"])}
    leaf = {k: v.clone().requires_grad_(True) for k, v in leaf.items()}
    kappa, case = 2.0, 1
    wS = _f64(np.random.default_rng(5).standard_normal(tuple(ad["dS0"].shape[:2]) + (prob.N + 1, nx, nx)))

    def boom(*a, **k):
        raise AssertionError("a host round trip in the covariance's autograd layer")

    with monkeypatch.context() as mp:
        mp.setattr(torch.Tensor, "cpu", boom)
        Sig, su, sg = autograd.policy_covariance(s, *(leaf[k] for k in ("p", "ubar", "Xbar", "K", "S0", "W", "obs_var")))
        nlx, nux, nlg, nug = policy.tighten(d["lbx"], d["ubx"], d["lbg"], d["ubg"], {"sigma_u": su, "sigma_g": sg}, kappa, case=case)
        loss = nug.sum() - nlg.sum() + 0.5 * (nux ** 2).sum() - nlx.sum() + (wS * Sig).sum()
        grads = torch.autograd.grad(loss, [leaf[k] for k in leaf])
        # the same seeds by hand, through covariance_grad
        cov = {"Sigma": Sig.detach(), "sigma_u": su.detach(), "sigma_g": sg.detach()}
        su2, sg2 = su.detach().clone().requires_grad_(True), sg.detach().clone().requires_grad_(True)
        t = policy.tighten(d["lbx"], d["ubx"], d["lbg"], d["ubg"], {"sigma_u": su2, "sigma_g": sg2}, kappa, case=case)
        sub, sgb = torch.autograd.grad(t[3].sum() - t[2].sum() + 0.5 * (t[1] ** 2).sum() - t[0].sum(), [su2, sg2])
        hand = policy.covariance_grad(s, pol, {"x": d["ubar"]}, d["p"], cov, Sigma_b=wS, sigma_u_b=sub.contiguous(),
                                      sigma_g_b=sgb.contiguous(), want=OUT)
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    g = dict(zip(leaf, (v.cpu().numpy() for v in grads)))
    h = _np(hand, prob, B)
    assert np.any(sub.cpu().numpy() != 0.0) and np.any(sgb.cpu().numpy() != 0.0)
    np.testing.assert_array_equal(g["p"], h["p_bar"].sum(1), err_msg="p")
    np.testing.assert_array_equal(g["ubar"], h["ubar_bar"].sum(1).reshape(B, -1), err_msg="ubar")
    np.testing.assert_array_equal(g["Xbar"], h["Xbar_bar"].sum(1), err_msg="Xbar")
    np.testing.assert_array_equal(g["K"], np.swapaxes(h["K_bar"], -1, -2).sum(1), err_msg="K (the raw column-major blocks)")
    np.testing.assert_array_equal(g["obs_var"], h["obs_var_bar"].sum(1), err_msg="obs_var")
    for k, hb in (("S0", h["S0_bar"]), ("W", h["W_bar"])):
        fold = np.triu(hb + np.swapaxes(hb, -1, -2), 1) + hb * np.eye(nx)
        np.testing.assert_array_equal(g[k], fold, err_msg=f"{k}: the lower-triangle fold")
        assert np.all(np.tril(g[k], -1) == 0.0) and np.any(np.triu(g[k], 1) != 0.0)
    # shared inputs get the sum over the batch
    sh = {k: leaf[k].detach()[0].clone().requires_grad_(True) for k in ("ubar", "Xbar", "K", "S0", "W", "obs_var")}
    pr = d["p"][:1].expand(B, -1).contiguous()
    o1 = autograd.policy_covariance(s, pr, sh["ubar"], sh["Xbar"], sh["K"], sh["S0"], sh["W"], sh["obs_var"])
    gs = torch.autograd.grad(o1[1].sum() + o1[2].sum(), [sh[k] for k in sh])
    rp = {k: v.detach().unsqueeze(0).expand(B, *v.shape).contiguous().requires_grad_(True) for k, v in sh.items()}
    o2 = autograd.policy_covariance(s, pr, rp["ubar"], rp["Xbar"], rp["K"], rp["S0"], rp["W"], rp["obs_var"])
    gr = torch.autograd.grad(o2[1].sum() + o2[2].sum(), [rp[k] for k in rp])
    torch.cuda.synchronize()
    for k, a, b in zip(sh, gs, gr):
        np.testing.assert_array_equal(a.cpu().numpy(), b.sum(0).cpu().numpy(), err_msg=f"shared {k}")
    # S0 = 0, W None: every deviation is exactly 0 and passes no gradient
    z = torch.zeros_like(ad["dS0"]).requires_grad_(True)
    Kz = raw["K"].clone().requires_grad_(True)
    o3 = autograd.policy_covariance(s, d["p"], d["ubar"], raw["X"], Kz, z)
    gz = torch.autograd.grad(o3[1].sum() + o3[2].sum(), [z, Kz])
    torch.cuda.synchronize()
    assert all(torch.all(v == 0.0) for v in gz), "S0 = 0: zero, finite gradients"
    print(f"autograd = covariance_grad bitwise; S0 / W folded onto the read triangle; shared inputs summed; S0 = 0 gives zeros; "
          f"memory_info {mem} unchanged")
