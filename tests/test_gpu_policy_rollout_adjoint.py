"""nmpc_policy_rollout_adjoint_batch / nmpc_policy_rollout_adjoint_batch_dev
(Solver.policy_rollout_adjoint, policy_rollout_adjoint_device, nmpc_amd.autograd.policy_rollout,
nmpc_amd.policy.rollout_grad): the reverse sweep of the policy rollouts, one lane per sample with wave
sums over the samples, against the NumPy checker of tests/rollout_adjoint_ref.py (the oracle's dyn_jac
and stage_cost_derivs, one sample at a time, the samples added in order).

Cases, policies, samples and the clamp box are those of tests/test_gpu_policy_rollout.py (its `_case`
is shared: the four solved cases and the synthetic n1 and n63_16obs, the policy of policy_device, 70
samples of which sample 0 is undisturbed and samples 1 and 2 saturate).  X is policy_rollout_device's
on the same inputs.  M = 3 (a partial block), 64 (a full block) and 70 (two blocks, the second with 58
dead lanes) on race_track_2, uav5 (5 x 3 blocks) and n1 (N = 1); M = 3 on the other cases, n63_16obs
(N = 63, 16 obstacles) among them: its checker takes seconds per block of samples, and nothing in the
kernel depends on N and M together.

Gate (a): every output within max(1e-10 S, 100 s) of the checker's, S being the sum of the absolute
values of the terms that make the entry up (over samples and stages for the reduced outputs, 1 + |value|
for e0_bar and w_bar), s the checker's own spread under a relative 1e-15 perturbation of X; nsat_out
equal to the forward's nsat.  Every figure is printed before it is asserted."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

from tests import policy_ref as pf
from tests import rollout_adjoint_ref as ra
from tests.test_gpu_policy_rollout import _case, _f64, _run

pytestmark = pytest.mark.gpu

CASES = tuple(pf.SOLVED) + ("n1", "n63_16obs")
MS_FULL = (3, 64, 70)
MS = {"race_track_2": MS_FULL, "uav5": MS_FULL, "n1": MS_FULL}
OUT = ("ubar_bar", "K_bar", "Xbar_bar", "p_bar", "e0_bar", "w_bar", "nsat")
DBL = OUT[:6]
H = 5e-7       # the CPU gate's step (tests/test_rollout_adjoint_capi.py says why not 1e-6)
BOUND = 1e-5   # ... and its bound, of sum |g_i| |d_i|


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@functools.lru_cache(maxsize=None)
def _acase(name):
    """Everything a case's tests share, computed once and left unchanged: the forward launch's X, U
    and nsat on the case's samples, the seeds, the checker's result and its spread."""
    import torch

    c = _case(name)
    M = max(MS.get(name, (3,)))
    B, prob = c["B"], c["prob"]
    N, nu, nx = prob.N, prob.nu, prob.nx
    fwd = _run(c, slice(0, M), want=("J", "nsat", "X", "U"))
    rng = np.random.default_rng(77)
    seeds = {"Jb": rng.standard_normal((B, M)), "Xb": rng.standard_normal((B, M, N + 1, nx)),
             "Ub": rng.standard_normal((B, M, N, nu))}
    args = (prob, c["P"], c["ubar"], c["Xbar"], c["K"])
    kw = dict(Jb=seeds["Jb"], Xb=seeds["Xb"], Ub=seeds["Ub"], lbx=c["cb"][0], ubx=c["cb"][1])
    ref = ra.adjoint_batch(*args, fwd["X"], **kw)
    per = ra.adjoint_batch(*args, fwd["X"] * (1.0 + 1e-15 * np.random.default_rng(4243).standard_normal(fwd["X"].shape)), **kw)
    dev = dict(c["dev"], X=_f64(fwd["X"]), **{k: _f64(v) for k, v in seeds.items()})
    torch.cuda.synchronize()
    return {"c": c, "M": M, "fwd": fwd, "seeds": seeds, "ref": ref, "per": per, "dev": dev}


def _adj(a, sl=None, want=OUT, feedback=True, clamp=True, use=("Jb", "Xb", "Ub"), out=None, **over):
    """policy_rollout_adjoint_device on the samples `sl` of a case; NumPy results."""
    import torch

    c, d = a["c"], dict(a["dev"], **over)
    sl = slice(0, a["M"]) if sl is None else sl
    raw = c["pol"]["raw"]
    res = c["s"].policy_rollout_adjoint_device(
        d["p"], d["ubar"], raw["X"], d.get("K", raw["K"]) if feedback else None, d["X"][:, sl].contiguous(),
        **{k: d[k][:, sl].contiguous() if k in use else None for k in ("Jb", "Xb", "Ub")},
        lbx=d["lbx"] if clamp else None, ubx=d["ubx"] if clamp else None, want=want, out=out)
    torch.cuda.synchronize()
    return _np(res)


def _same(x, y, what, keys=OUT):
    for k in keys:
        np.testing.assert_array_equal(x[k], y[k], err_msg=f"{what}: {k}")


def _against(name, a, got, M):
    """Gate (a) at the first M samples; returns the largest error / tolerance per output."""
    ref, per = ra.reduce_samples(a["ref"], M), ra.reduce_samples(a["per"], M)
    B = a["c"]["B"]
    figs = {}
    for k in DBL:
        g = got[k]
        if k == "K_bar":
            g = np.swapaxes(g, -1, -2)  # the kernel's column-major blocks
        r = ref[k].reshape(g.shape)
        sp = np.abs(per[k].reshape(g.shape) - r)
        S = ref["S"][k].reshape(g.shape) if k in ra.REDUCED else 1.0 + np.abs(r)
        tol = np.maximum(1e-10 * S, 100.0 * sp)
        err = np.abs(g - r)
        exact = tol == 0.0  # no term at all: exactly 0 on both sides
        np.testing.assert_array_equal(g[exact], r[exact], err_msg=f"{name} M = {M}: structural zeros of {k}")
        figs[k] = float(np.max(err[~exact] / tol[~exact], initial=0.0))
    print(f"{name} M = {M}: error / tolerance " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items())
          + f"; nsat 0 to {a['fwd']['nsat'][:, :M].max()}")
    np.testing.assert_array_equal(got["nsat"], a["fwd"]["nsat"][:, :M], err_msg=f"{name} M = {M}: nsat against the forward's")
    np.testing.assert_array_equal(got["nsat"], ref["nsat"], err_msg=f"{name} M = {M}: nsat against the checker's")
    for k, v in figs.items():
        assert v <= 1.0, (name, M, k, v)
    assert B == got["p_bar"].shape[0]
    return figs


@pytest.mark.parametrize("name", CASES)
def test_gate_a_every_output_against_the_checker(name):
    """M = 3, 64, 70 (the small cases) or 3: every output within tolerance, nsat the forward's, the
    entries of p_bar that nothing reads (obstacle centres, the target's third entry, tail entries) and
    stage N of Xbar_bar exactly 0."""
    a = _acase(name)
    prob = a["c"]["prob"]
    for M in MS.get(name, (3,)):
        got = _adj(a, slice(0, M))
        _against(name, a, got, M)
        unread = np.setdiff1d(np.arange(got["p_bar"].shape[1]), ra.read_entries(prob))
        assert unread.size > 0 and np.all(got["p_bar"][:, unread] == 0.0), (name, M)
        assert np.all(got["Xbar_bar"][:, -1] == 0.0), (name, M)
        assert np.all(np.isfinite(got["p_bar"])) and np.any(got["K_bar"] != 0.0)
    if name == "n63_16obs":
        assert prob.N == 63 and prob.n_obs == 16


def _loss(fw, seeds, sl):
    return (np.sum(seeds["Jb"][:, sl] * fw["J"], axis=1) + np.sum(seeds["Xb"][:, sl] * fw["X"], axis=(1, 2, 3))
            + np.sum(seeds["Ub"][:, sl] * fw["U"], axis=(1, 2, 3)))


def _faces(U, lo, hi):
    return (U == lo.reshape(1, 1, *U.shape[2:])) | (U == hi.reshape(1, 1, *U.shape[2:]))


def test_gate_b_kernel_against_kernel_directional_derivative():
    """(L(+h d) - L(-h d)) / 2h through the forward entry point against <gradient, d> of the new one,
    per scenario, on race_track_2 with M = 4: the CPU gate's step, bound and condition -- both
    difference points have the base point's clamp set, read from the forward's U on the box faces.
    The direction is the first of a short list of seeds at which that condition holds and the
    differences at h and h / 2 agree to 1e-6 of the scale (the difference's own error; neither
    condition looks at the gradient)."""
    a = _acase("race_track_2")
    c, sl = a["c"], slice(0, 4)
    B, prob, s = c["B"], c["prob"], c["s"]
    N, nu, nx = prob.N, prob.nu, prob.nx
    lo, hi = (v.reshape(N, nu) for v in c["cb"][:2])
    raw = c["pol"]["raw"]
    g = _adj(a, sl)
    base = _faces(a["fwd"]["U"][:, sl], lo, hi)
    Kraw = raw["K"].cpu().numpy()  # (B, N, nx, nu)

    def forward(t, d):
        dv = c["dev"]
        res = s.policy_rollout_device(_f64(c["P"] + t * d["p"]), _f64(c["ubar"] + t * d["ubar"]),
                                      _f64(c["Xbar"] + t * d["Xbar"]), _f64(Kraw + t * d["K"]),
                                      _f64(c["e0"][:, sl] + t * d["e0"]), w=_f64(c["w"][:, sl] + t * d["w"]),
                                      lbx=dv["lbx"], ubx=dv["ubx"], want=("J", "X", "U"))
        return _np(res)

    found = None
    for seed in (21, 22, 23, 24, 25, 26, 27, 28):
        rng = np.random.default_rng(seed)
        d = {"p": np.zeros_like(c["P"]), "ubar": rng.standard_normal(c["ubar"].shape),
             "Xbar": rng.standard_normal(c["Xbar"].shape), "K": rng.standard_normal(Kraw.shape) * np.max(np.abs(Kraw)),
             "e0": rng.standard_normal((B, 4, nx)), "w": rng.standard_normal((B, 4, N, nx))}
        d["p"][:, ra.read_entries(prob)] = rng.standard_normal((B, len(ra.read_entries(prob))))
        fp, fm, fp2, fm2 = forward(H, d), forward(-H, d), forward(H / 2, d), forward(-H / 2, d)
        same = all(np.array_equal(_faces(f["U"], lo, hi), base) for f in (fp, fm))
        fd = (_loss(fp, a["seeds"], sl) - _loss(fm, a["seeds"], sl)) / (2 * H)
        fd2 = (_loss(fp2, a["seeds"], sl) - _loss(fm2, a["seeds"], sl)) / H
        pairs = ((g["p_bar"], d["p"]), (g["ubar_bar"], d["ubar"]), (g["Xbar_bar"], d["Xbar"]), (g["K_bar"], d["K"]),
                 (g["e0_bar"], d["e0"]), (g["w_bar"], d["w"]))
        gd = sum(np.sum((x * y).reshape(B, -1), axis=1) for x, y in pairs)
        scale = sum(np.sum(np.abs(x * y).reshape(B, -1), axis=1) for x, y in pairs)
        own = np.max(np.abs(fd - fd2) / scale)
        print(f"direction seed {seed}: clamp sets unchanged {same}, |fd(h) - fd(h / 2)| / scale {own:.1e}")
        if same and own <= 1e-6:
            found = seed
            break
    assert found is not None, "no direction of the list keeps the clamp sets"
    fig = np.abs(fd - gd) / scale
    print(f"race_track_2, M = 4, h = {H:g}: |fd - <g, d>| / sum |g||d| per scenario " + ", ".join(f"{v:.1e}" for v in fig)
          + "; relative to |<g, d>| " + ", ".join(f"{v:.1e}" for v in np.abs(fd - gd) / np.abs(gd)) + f" (bound {BOUND:.0e})")
    assert np.any(a["fwd"]["nsat"][:, sl] > 0) and np.any(a["fwd"]["nsat"][:, sl] == 0)
    assert np.all(fig <= BOUND), fig


def test_gate_b_a_gradient_step_lowers_the_mean_cost():
    """ubar - eta ubar_bar with Jb = 1 / M lowers the mean J over the same samples by 0.5 to 1.5 times
    eta |ubar_bar|^2, per scenario.  eta starts at 1e-3 / max |ubar_bar| of the scenario (a largest
    control move of 1e-3) and is halved until the forward's clamp set is the base point's."""
    import torch

    a = _acase("race_track_2")
    c, M = a["c"], a["M"]
    B, prob, s, dv = c["B"], c["prob"], c["s"], c["dev"]
    lo, hi = (v.reshape(prob.N, prob.nu) for v in c["cb"][:2])
    raw = c["pol"]["raw"]
    Jb = torch.full((B, M), 1.0 / M, dtype=torch.float64, device="cuda")
    g = _np(s.policy_rollout_adjoint_device(dv["p"], dv["ubar"], raw["X"], raw["K"], a["dev"]["X"], Jb=Jb, lbx=dv["lbx"],
                                            ubx=dv["ubx"], want=("ubar_bar",)))["ubar_bar"]
    base = _faces(a["fwd"]["U"], lo, hi)
    J0 = a["fwd"]["J"].mean(axis=1)
    eta = 1e-3 / np.max(np.abs(g), axis=1)
    for halvings in range(16):
        fw = _np(s.policy_rollout_device(dv["p"], _f64(c["ubar"] - eta[:, None] * g), raw["X"], raw["K"], dv["e0"][:, :M].contiguous(),
                                         w=dv["w"][:, :M].contiguous(), lbx=dv["lbx"], ubx=dv["ubx"], want=("J", "U")))
        if np.array_equal(_faces(fw["U"], lo, hi), base):
            break
        eta = eta / 2
    else:
        raise AssertionError("no step of the list keeps the clamp set")
    dec = J0 - fw["J"].mean(axis=1)
    pred = eta * np.sum(g * g, axis=1)
    print(f"race_track_2, M = {M}: eta {eta} after {halvings} halvings, mean J {J0} -> decrease {dec}, "
          f"eta |ubar_bar|^2 {pred}, ratio {dec / pred}")
    assert np.all(pred > 0) and np.all(dec >= 0.5 * pred) and np.all(dec <= 1.5 * pred), dec / pred


def test_gate_c_bitwise_repeats_sharing_and_the_host_entry_point():
    """All bitwise: two identical calls; ld = 0 sharing against replicated inputs; the host entry point
    against the device one for several output subsets."""
    import torch

    a = _acase("race_track_2")
    c, M = a["c"], a["M"]
    B, s = c["B"], c["s"]
    full = _adj(a)
    _same(full, _adj(a), "two identical calls")
    # ld = 0: scenario 0's p, plan, policy, trajectories and seeds shared by B scenarios
    d, raw = a["dev"], c["pol"]["raw"]
    one = {k: d[k][0].contiguous() for k in ("p", "ubar", "X", "Jb", "Xb", "Ub")}
    one.update(Xbar=raw["X"][0].contiguous(), K=raw["K"][0].contiguous(), lbx=d["lbx"], ubx=d["ubx"])
    rep = {k: v.unsqueeze(0).expand(B, *v.shape).contiguous() for k, v in one.items()}

    def call(v, p):
        return _np(s.policy_rollout_adjoint_device(p, v["ubar"], v["Xbar"], v["K"], v["X"], Jb=v["Jb"], Xb=v["Xb"],
                                                   Ub=v["Ub"], lbx=v["lbx"], ubx=v["ubx"], want=OUT))

    shared, repl = call(one, rep["p"]), call(rep, rep["p"])
    torch.cuda.synchronize()
    _same(shared, repl, "ld = 0 against replicated inputs")
    for k in OUT:
        np.testing.assert_array_equal(shared[k][0], full[k][0], err_msg=f"ld = 0 against the batch's scenario 0: {k}")
        for j in range(1, B):
            np.testing.assert_array_equal(shared[k][j], shared[k][0], err_msg=k)
    # output subsets, host against device entry point
    X = a["fwd"]["X"]
    for keys in (OUT, ("ubar_bar",), ("p_bar", "nsat"), ("K_bar", "Xbar_bar"), ("e0_bar", "w_bar"), ("w_bar",),
                 ("ubar_bar", "K_bar", "e0_bar", "nsat")):
        host = s.policy_rollout_adjoint(c["P"], c["ubar"], c["Xbar"], c["K"], X, a["seeds"]["Jb"], a["seeds"]["Xb"],
                                        a["seeds"]["Ub"], c["cb"][0], c["cb"][1], want=keys)
        dev = _adj(a, want=keys)
        assert set(host) == set(dev) == set(keys), keys
        for k in keys:
            h = np.swapaxes(host[k], -1, -2) if k == "K_bar" else host[k]
            np.testing.assert_array_equal(h, full[k], err_msg=f"host, outputs {keys}: {k}")
            np.testing.assert_array_equal(dev[k], full[k], err_msg=f"device, outputs {keys}: {k}")


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_c_blocks_dead_lanes_and_open_loop(name):
    """The dead-lane and block-order contract, bitwise: the reduced outputs at M = 70 equal fl(the
    result at the first 64 samples + the result at the last 6), in that order, and the per-sample
    outputs are the two calls' side by side.  K NULL equals K = 0 on ubar_bar, p_bar, e0_bar, w_bar."""
    import torch

    a = _acase(name)
    assert a["M"] == 70
    full, first, last = _adj(a), _adj(a, slice(0, 64)), _adj(a, slice(64, 70))
    for k in ra.REDUCED:
        np.testing.assert_array_equal(full[k], first[k] + last[k], err_msg=f"{name}: {k} at M = 70 against 64 + 6")
        assert np.any(last[k] != 0.0), k
    for k in ra.PER_SAMPLE + ("nsat",):
        np.testing.assert_array_equal(full[k], np.concatenate([first[k], last[k]], axis=1), err_msg=f"{name}: {k}")
    keys = ("ubar_bar", "p_bar", "e0_bar", "w_bar", "nsat")
    ol = _adj(a, feedback=False, want=keys)
    zero = _adj(a, K=torch.zeros_like(a["c"]["pol"]["raw"]["K"]), want=keys)
    _same(ol, zero, f"{name}: K = None against K = 0", keys)


@pytest.mark.parametrize("name", ["race_track_2", "uav5"])
def test_gate_c_no_write_outside_the_outputs(name):
    """Output buffers carved out of one tensor of sentinels, M = 70: every entry of them is written,
    nothing outside them is (uav5: blocks of 5 states and 3 controls)."""
    import torch

    a = _acase(name)
    c, M = a["c"], a["M"]
    B, s = c["B"], c["s"]
    shapes = s._rollout_adjoint_shapes(B, M)
    if name == "uav5":
        assert shapes["K_bar"][-2:] == (5, 3)
    pad = 64
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    ibig = torch.full((B * M + 2 * pad,), 77, dtype=torch.int32, device="cuda")
    out, o, spans = {"nsat": ibig[pad:pad + B * M].view(B, M)}, pad, []
    for k in DBL:
        n = int(np.prod(shapes[k]))
        out[k] = big[o:o + n].view(shapes[k])
        spans.append((o, o + n))
        o += n + pad
    got = _adj(a, out=out)
    h, hi = big.cpu().numpy(), ibig.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for x, y in spans:
        keep[x:y] = False
        assert not np.any(h[x:y] == 7.0)
    assert np.all(h[keep] == 7.0)
    assert np.all(hi[:pad] == 77) and np.all(hi[pad + B * M:] == 77) and not np.any(hi[pad:pad + B * M] == 77)
    _same(got, _adj(a), f"{name}: carved buffers against own ones")


def test_gate_d_seeds_and_nan():
    """Each seed alone equals the call with the other seeds zero (w_bar, e0_bar and the reduced outputs
    within rounding: a zero seed adds +0); the three single-seed gradients add up to the joint one.  A
    NaN in one sample's X poisons that sample's e0_bar and w_bar and the reduced outputs of its own
    scenario; everything else is bitwise untouched."""
    import torch

    a = _acase("race_track_2")
    c, M = a["c"], a["M"]
    B = c["B"]
    full = _adj(a)
    parts = [_adj(a, use=(k,)) for k in ("Jb", "Xb", "Ub")]
    S = ra.reduce_samples(a["ref"], M)["S"]
    for k in DBL:
        tot = parts[0][k] + parts[1][k] + parts[2][k]
        if k in ra.REDUCED:  # gate (a)'s scale: the checker's absolute-term sums
            scale = (np.swapaxes(S[k], -1, -2) if k == "K_bar" else S[k]).reshape(tot.shape)
        else:
            scale = 1.0 + np.abs(parts[0][k]) + np.abs(parts[1][k]) + np.abs(parts[2][k])
        assert np.all(np.abs(tot - full[k]) <= 1e-10 * scale), k
    for i, k in enumerate(("Jb", "Xb", "Ub")):
        zeros = {j: torch.zeros_like(a["dev"][j]) for j in ("Jb", "Xb", "Ub") if j != k}
        z = _adj(a, **zeros)
        for o in DBL:
            assert np.all(np.abs(z[o] - parts[i][o]) <= 1e-13 * (1.0 + np.abs(z[o]))), (k, o)
        np.testing.assert_array_equal(z["nsat"], parts[i]["nsat"])
    only_J = parts[0]
    assert np.all(only_J["w_bar"][:, :, -1] == 0.0)  # lam_N = Xb_N = 0: nothing reaches the last disturbance
    # NaN in X of scenario 1, sample 5
    X = a["dev"]["X"].clone()
    X[1, 5, 2, 0] = float("nan")
    got = _adj(a, X=X)
    assert np.all(np.isnan(got["e0_bar"][1, 5])) and np.all(np.isnan(got["w_bar"][1, 5]))
    read = ra.read_entries(c["prob"])
    assert np.all(np.isnan(got["ubar_bar"][1])) and np.all(np.isnan(got["K_bar"][1])) and np.all(np.isnan(got["p_bar"][1, read]))
    assert np.all(np.isnan(got["Xbar_bar"][1, :-1])) and np.all(got["Xbar_bar"][1, -1] == 0.0)
    rows = np.ones((B, M), bool)
    rows[1, 5] = False
    for k in ra.PER_SAMPLE:
        np.testing.assert_array_equal(got[k][rows], full[k][rows], err_msg=k)
    for k in ra.REDUCED:
        np.testing.assert_array_equal(np.delete(got[k], 1, axis=0), np.delete(full[k], 1, axis=0), err_msg=k)
    assert np.all(np.isfinite(np.concatenate([full[k].ravel() for k in DBL])))


def test_gate_e_argument_validation_on_a_live_handle():
    """B <= 0, M <= 0, a NULL p, ubar, Xbar or X, every seed NULL, every double output NULL, K_bar or
    Xbar_bar without K, and a leading dimension that is neither 0 nor >= the vector length return
    NMPC_E_INVALID from both entry points before any device call, each with the full message of its
    rule, in the order of the forward pair's checks: nothing is written, and the handle still works."""
    from nmpc_amd import _lib

    a = _acase("race_track_2")
    c = a["c"]
    spec, s, B = c["spec"], c["s"], c["B"]
    N, nu, nx = spec.N, spec.nw // spec.N, spec.nX // (spec.N + 1)
    L = _lib.lib()
    M = 5
    arr = {"p": c["P"], "ubar": c["ubar"], "Xbar": c["Xbar"], "K": np.swapaxes(c["K"], 2, 3),
           "lbx": np.repeat(c["cb"][0][None], B, 0), "ubx": np.repeat(c["cb"][1][None], B, 0), "X": a["fwd"]["X"][:, :M],
           "Jb": a["seeds"]["Jb"][:, :M], "Xb": a["seeds"]["Xb"][:, :M], "Ub": a["seeds"]["Ub"][:, :M]}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    names = tuple(arr)
    lens = dict(zip(names, (spec.np, spec.nw, spec.nX, nu * nx * N, spec.nw, spec.nw, spec.nX * M, M, spec.nX * M,
                            spec.nw * M)))
    shapes = s._rollout_adjoint_shapes(B, M)
    arr.update({k: np.full(shapes[k], 7.0) for k in DBL})
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
        args += [g(k) for k in DBL] + [gi]
        return (L.nmpc_policy_rollout_adjoint_batch_dev(*args, vp(0)) if dev
                else L.nmpc_policy_rollout_adjoint_batch(*args))

    req, ldm = "required pointer is null (p, ubar, Xbar, X)", "leading dimension smaller than the vector length"
    seeds = "every seed pointer is null (Jb, Xb, Ub)"
    outs = "ubar_bar_out, K_bar_out, Xbar_bar_out, p_bar_out, e0_bar_out and w_bar_out are all null"
    needk = "K_bar_out and Xbar_bar_out need K"
    allseeds = ("Jb", "Xb", "Ub")
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("M = 0", dict(M_=0), "M <= 0"),
                 ("M < 0", dict(M_=-1), "M <= 0"), ("M too large", dict(M_=64 * 65535 + 1), "M > 64 x 65535"),
                 ("no seed", dict(null=allseeds), seeds), ("no output", dict(null=DBL), outs),
                 ("K NULL with K_bar", dict(null=("K", "Xbar_bar")), needk),
                 ("K NULL with Xbar_bar", dict(null=("K", "K_bar")), needk),
                 ("ld_p negative", dict(ld={"p": -spec.np}), ldm), ("ld_X one sample", dict(ld={"X": spec.nX}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), req) for k in ("p", "ubar", "Xbar", "X")]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        # two rules at once: the earlier one in the order of the checks answers
        cases += [("B = 0 and M = 0", dict(B_=0, M_=0), "B <= 0"), ("M = 0 and p NULL", dict(M_=0, null=("p",)), "M <= 0"),
                  ("X NULL and no seed", dict(null=("X",) + allseeds), req),
                  ("no seed and no output", dict(null=allseeds + DBL), seeds),
                  ("no output and no K", dict(null=DBL + ("K",)), outs),
                  ("K NULL with K_bar and ld_Ub short", dict(null=("K",), ld={"Ub": lens["Ub"] - 1}), needk)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error() and L.nmpc_last_error().decode() == msg, (what, dev, L.nmpc_last_error())
    assert all(np.all(arr[k] == 7.0) for k in DBL) and np.all(nsat == 99)  # nothing ran
    # and the handle still works: open loop with Jb alone; then everything
    assert call(null=("K", "lbx", "ubx", "Xb", "Ub", "K_bar", "Xbar_bar", "e0_bar", "w_bar")) == 0
    assert np.all(np.isfinite(arr["ubar_bar"])) and np.all(nsat == 0) and all(np.all(arr[k] == 7.0) for k in ("K_bar", "w_bar"))
    assert call() == 0
    full = _adj(a, slice(0, M))
    for k in DBL:
        np.testing.assert_array_equal(arr[k], full[k], err_msg=k)
    np.testing.assert_array_equal(nsat, full["nsat"])


def test_gate_f_autograd_nothing_read_back_nothing_allocated(monkeypatch):
    """autograd.policy_rollout, then (J.mean() + (X * a).sum() + (U * b).sum()).backward(): the .grad of
    p, ubar, Xbar, K, e0 and w equal the direct device call's outputs bitwise; the whole pass completes
    with torch.Tensor.cpu made to raise; on a handle that has run nothing before, memory_info is unchanged
    at M <= 64 and at M = 70 without a summed output.  policy.rollout_grad with coefficients c returns
    c_bar = <kff, ubar_bar>."""
    import torch
    from nmpc_amd import autograd, policy

    from tests.test_gpu_solve_adjoint import _solver

    a = _acase("race_track_2")
    c = a["c"]
    B, dv, raw = c["B"], c["dev"], c["pol"]["raw"]
    M = 64
    # a handle of its own, which has run nothing yet: the case's shared one has grown its workspace
    # in the M = 70 calls of the tests above, and would hide a workspace request at M <= 64
    s = _solver(c["spec"])
    mem = s.memory_info()
    print(f"fresh handle: {mem}")
    leaves = {k: t.clone().requires_grad_(True) for k, t in
              (("p", dv["p"]), ("ubar", dv["ubar"]), ("Xbar", raw["X"]), ("K", raw["K"]),
               ("e0", dv["e0"][:, :M].contiguous()), ("w", dv["w"][:, :M].contiguous()))}
    wa, wb = a["dev"]["Xb"][:, :M].contiguous(), a["dev"]["Ub"][:, :M].contiguous()
    torch.cuda.synchronize()

    def boom(*x, **k):
        raise AssertionError("a host round trip in autograd.policy_rollout")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        J, X, U = autograd.policy_rollout(s, leaves["p"], leaves["ubar"], leaves["Xbar"], leaves["K"], leaves["e0"],
                                          leaves["w"], dv["lbx"], dv["ubx"])
        (J.mean() + (X * wa).sum() + (U * wb).sum()).backward()
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    Jb = torch.full((B, M), 1.0 / (B * M), dtype=torch.float64, device="cuda")
    direct = _np(s.policy_rollout_adjoint_device(dv["p"], dv["ubar"], raw["X"], raw["K"], X.detach(), Jb=Jb, Xb=wa, Ub=wb,
                                                 lbx=dv["lbx"], ubx=dv["ubx"], want=DBL))
    assert s.memory_info() == mem
    # M = 70 with the per-sample outputs alone writes no partial sums and needs no workspace either;
    # with a summed output the workspace covers the two blocks' partial sums
    s.policy_rollout_adjoint_device(dv["p"], dv["ubar"], raw["X"], raw["K"], a["dev"]["X"], Jb=a["dev"]["Jb"],
                                    lbx=dv["lbx"], ubx=dv["ubx"], want=("e0_bar", "w_bar", "nsat"))
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    s.policy_rollout_adjoint_device(dv["p"], dv["ubar"], raw["X"], raw["K"], a["dev"]["X"], Jb=a["dev"]["Jb"],
                                    lbx=dv["lbx"], ubx=dv["ubx"], want=("ubar_bar",))
    torch.cuda.synchronize()
    shp = s._rollout_adjoint_shapes(1, 1)
    nred = sum(int(np.prod(shp[k])) for k in ra.REDUCED)
    assert s.memory_info()["ws_bytes"] >= max(mem["ws_bytes"], B * 2 * nred * 8)
    np.testing.assert_array_equal(X.detach().cpu().numpy(), a["fwd"]["X"][:, :M])
    for k, o in (("p", "p_bar"), ("ubar", "ubar_bar"), ("Xbar", "Xbar_bar"), ("K", "K_bar"), ("e0", "e0_bar"), ("w", "w_bar")):
        assert leaves[k].grad is not None, k
        np.testing.assert_array_equal(leaves[k].grad.cpu().numpy(), direct[o], err_msg=f"autograd: {k}.grad against {o}")
    # only what requires grad is formed; the bounds get none
    p2 = dv["p"].clone().requires_grad_(True)
    lbx2 = dv["lbx"].clone().requires_grad_(True)
    J2, _, _ = autograd.policy_rollout(s, p2, dv["ubar"], raw["X"], raw["K"], leaves["e0"].detach(), None, lbx2, dv["ubx"])
    J2.sum().backward()
    assert p2.grad is not None and lbx2.grad is None
    # policy.rollout_grad: c_bar by one einsum
    from tests.test_gpu_solve_tangent import _dirs, _prep

    nd = 2
    dp = _dirs(c["spec"], B, nd, 97)
    dsol, db, dP, dd, _ = _prep(c["spec"], c["sol"], c["bounds"], c["P"], dp, B, nd, keys=(), g=False, rep=False)
    pol = s.policy_device(dsol, *db, dP, dd)
    coef = _f64(0.05 * np.random.default_rng(99).standard_normal((B, nd)))
    fw = policy.rollout(s, pol, dsol, dP, dv["e0"][:, :3].contiguous(), c=coef, lbx=dv["lbx"], ubx=dv["ubx"], want=("J", "X"))
    Jb3 = torch.full((B, 3), 1.0 / 3, dtype=torch.float64, device="cuda")
    r = policy.rollout_grad(s, pol, dsol, dP, fw["X"], Jb=Jb3, c=coef, lbx=dv["lbx"], ubx=dv["ubx"], want=("p_bar",))
    torch.cuda.synchronize()
    kff = pol["kff"].cpu().numpy().reshape(B, nd, -1)
    np.testing.assert_allclose(r["c_bar"].cpu().numpy(), np.einsum("bdn,bn->bd", kff, r["ubar_bar"].cpu().numpy()),
                               rtol=1e-13, atol=1e-13)
    assert set(r) == {"p_bar", "ubar_bar", "c_bar"}
