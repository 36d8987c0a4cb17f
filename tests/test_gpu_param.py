"""nmpc_param_products_batch / nmpc_param_products_batch_dev (Solver.param_products,
param_products_device, param_jacobian, param_cross, sensitivity(tangent="exact")): the exact
products with dg/dp, d_p grad_w L and dX/dp and the gradient grad_p L at given points, on the
GPU, against the oracle's dense forms (tests/param_ref.py: directions, scales, tolerance)."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest

from tests import eval_ref as er
from tests import kkt_ref as kr
from tests import param_ref as qr
from tests import products_ref as pr

pytestmark = pytest.mark.gpu

KEYS = ("jp", "hp", "dXp", "gp")


def _solver(spec):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)


def _t(dp):
    """(B, nd, np) -> Solver.param_products' (np, nd, B)."""
    return np.ascontiguousarray(np.transpose(dp, (2, 1, 0)))


def _pp(s, d, sel=slice(None), sigma=1.0, lam=True, dp=None):
    dp = _t(d["dp"][sel]) if dp is None else dp
    return s.param_products(d["w"][sel].T, d["p"][sel].T, dp, lam_g=d["lam_g"][sel].T if lam else None,
                            obj_factor=sigma)


def _scn(res, b):
    return {k: (res[k][:, b] if k == "gp" else res[k][:, :, b].T) for k in res}


def _equal(a, b, what=""):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_param_products_match_the_checker(name):
    """jp, hp, dXp and gp of every case (both models, N = 1 / 63, 16 obstacles, obstacle
    coordinates and cost weights from p), nd = 3, for (obj_factor, lam_g) = (1, random),
    (0.37, random), (0, random), (1, NULL): within 1e-10 of the checker's relative to the scales
    of tests/param_ref.py."""
    spec, d, ref = qr.reference(name)
    s = _solver(spec)
    B = er.CASES[name]
    for combo in qr.COMBOS:
        res = _pp(s, d, sigma=combo[0], lam=combo[1])
        assert res["jp"].shape == (spec.ng, qr.ND, B) and res["hp"].shape == (spec.nw, qr.ND, B)
        assert res["dXp"].shape == (spec.nX, qr.ND, B) and res["gp"].shape == (spec.np, B)
        for b in range(B):
            qr.check_against(_scn(res, b), ref[combo][b], f"{name} {combo} scenario {b}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_dense_param_jacobian_and_cross(name):
    """Solver.param_jacobian / param_cross (identity directions shared by the batch,
    ld_dp = 0) against the checker's matrices, each column relative to its own largest entry.
    The column of an entry of p that nothing reads is exactly 0."""
    spec, d, _ = qr.reference(name)
    _, _, evs = pr.evals(name)
    s = _solver(spec)
    B = er.CASES[name]
    Jp = s.param_jacobian(d["w"].T, d["p"].T)
    Cm = s.param_cross(d["w"].T, d["p"].T, lam_g=d["lam_g"].T, obj_factor=1.0)
    assert Jp.shape == (spec.ng, spec.np, B) and Cm.shape == (spec.nw, spec.np, B)
    eye = np.eye(spec.np)
    for b in range(B):
        ref = qr.cpu_products(evs[b], eye, 1.0, d["lam_g"][b])
        qr.check_against({"jp": Jp[:, :, b].T, "hp": Cm[:, :, b].T}, ref, f"{name} dense scenario {b}")
    for i, kind in enumerate(qr.entry_kinds(er.problem_of(spec))):
        if kind is None:
            assert np.all(Jp[:, i] == 0.0) and np.all(Cm[:, i] == 0.0), i


def test_gp_is_minus_lam_p_of_a_solve():
    """race_track_2, N = 6, four scenarios, seed 7: grad_p L at the solve's (x, lam_g) with
    obj_factor 1 equals -lam_p of that solve within 1e-10 of the gradient's absolute scale
    (the two are formed by different code: the solve's epilogue on its scaled multipliers)."""
    from nmpc_amd import draw_scenarios
    from oracle import nmpc_oracle as orc

    spec = er.case_spec("race_track_2")
    prob = er.problem_of(spec)
    s = _solver(spec)
    B = 4
    P = draw_scenarios(spec, B, seed=7)
    lbx, ubx, lbg, ubg = spec.bounds()
    sol = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    assert np.all(np.isin(s.stats()["status_code"], (0, 1)))
    gp = s.param_products(sol["x"], P.T, None, lam_g=sol["lam_g"])["gp"].T  # nd = 0
    assert gp.shape == (B, spec.np)
    for b in range(B):
        dn = qr.dense(orc.SSEval(prob, sol["x"][:, b], P[b]), 1.0, sol["lam_g"][:, b])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(dn["gp_scale"] > 0, np.abs(gp[b] + sol["lam_p"][:, b]) / (qr.TOL * dn["gp_scale"]),
                         np.where(gp[b] == 0, 0.0, np.inf))
            c = np.where(dn["gp_scale"] > 0, np.abs(gp[b] - dn["gp"]) / (qr.TOL * dn["gp_scale"]), 0.0)
        print(f"scenario {b}: |gp + lam_p| / bound {float(np.max(q)):.2e}, |gp - checker| / bound {float(np.max(c)):.2e}")
        assert np.all(q <= 1.0), (b, q)
        assert gp[b][10] == 0.0  # the target's third entry: nothing reads it


def test_structure_stage_zero_and_exact_zeros():
    """dXp's stage 0 is dp[0:nx] bitwise (both models); a direction that is zero wherever it is
    read -- NaN where it is not -- gives exactly 0 in every directional output."""
    for name in ("race_track_2", "uav5", "dynamic"):
        spec, d, _ = qr.reference(name)
        s = _solver(spec)
        nx = spec.nX // (spec.N + 1)
        res = _pp(s, d)
        np.testing.assert_array_equal(res["dXp"][:nx], _t(d["dp"])[:nx], err_msg=name)
        kinds = qr.entry_kinds(er.problem_of(spec))
        z = np.array([0.0 if k is not None else np.nan for k in kinds])
        zero = s.param_products(d["w"].T, d["p"].T, z, lam_g=d["lam_g"].T)
        for k in ("jp", "hp", "dXp"):
            assert np.all(zero[k] == 0.0), (name, k)
        np.testing.assert_array_equal(zero["gp"], res["gp"])


def test_batch_plumbing(monkeypatch):
    """All bitwise: nd = 3 equals three nd = 1 calls; a per-scenario copy of shared directions
    equals the broadcast (ld_dp = 0); host and device entry points agree for every subset of the
    outputs; nd = 0 with gp alone works; a NaN entry of one direction leaves the other directions
    and gp unchanged; a NaN in an entry of dp that nothing reads (the target's third entry; a
    tail entry no index names, on `dynamic` with one more entry of p) changes nothing; the
    number of wavefronts a scenario's directions are dealt to does not change the results."""
    import torch

    spec = er.case_spec("race_track_2")
    prob = er.problem_of(spec)
    s = _solver(spec)
    B, nd = 66, 3
    d = er.draw_point(spec, B, seed=81)
    d["dp"] = qr.draw_directions(prob, d["p"], nd, seed=82)
    full = _pp(s, d, sigma=0.37)
    assert all(np.all(np.isfinite(full[k])) for k in KEYS)
    for b in (0, 65):
        _equal(_scn(_pp(s, d, slice(b, b + 1), sigma=0.37), 0), _scn(full, b), f"scenario {b}")
    # directions are independent
    for dd in range(nd):
        single = _pp(s, d, sigma=0.37, dp=_t(d["dp"][:, dd:dd + 1]))
        for k in KEYS[:3]:
            np.testing.assert_array_equal(single[k][:, 0], full[k][:, dd], err_msg=f"{k} direction {dd}")
        np.testing.assert_array_equal(single["gp"], full["gp"])
    # shared directions: broadcast against a copy per scenario; one direction as a vector
    d0 = np.ascontiguousarray(d["dp"][0].T)  # (np, nd)
    shared = _pp(s, d, sigma=0.37, dp=d0)
    _equal(shared, _pp(s, d, sigma=0.37, dp=np.ascontiguousarray(np.repeat(d0[:, :, None], B, axis=2))), "ld_dp = 0")
    one_d = _pp(s, d, sigma=0.37, dp=d0[:, 0])
    for k in KEYS[:3]:
        np.testing.assert_array_equal(one_d[k][:, 0], shared[k][:, 0], err_msg=k)
    # a NaN entry poisons its own direction only
    dn = d["dp"].copy()
    dn[:, 1, 3] = np.nan  # theta_0's tangent of direction 1, every scenario
    poisoned = _pp(s, d, sigma=0.37, dp=_t(dn))
    for k in KEYS[:3]:
        np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=k)
        assert np.all(np.any(np.isnan(poisoned[k][:, 1]), axis=0)), k
    np.testing.assert_array_equal(poisoned["gp"], full["gp"])
    # ... and none at all where nothing reads it
    dn = d["dp"].copy()
    dn[:, :, 10] = np.nan
    _equal(_pp(s, d, sigma=0.37, dp=_t(dn)), full, "NaN in the target's third entry")
    # the chunk count: this class's workspace holds two slices of the kernel's 7,424 doubles
    # (Cap<20, 15>: 15.4k), so B = 66 runs on 2 wavefronts per scenario by default, "1" on one,
    # and "3" is held to 2
    assert s.memory_info()["ws_per_scenario"] // (8 * 7424) == 2
    for chunks in ("1", "2", "3"):
        monkeypatch.setenv("NMPC_PRODUCTS_CHUNKS", chunks)
        _equal(_pp(s, d, sigma=0.37), full, f"{chunks} chunks")
    monkeypatch.delenv("NMPC_PRODUCTS_CHUNKS")
    # device entry point: every subset of the outputs, then gp alone with nd = 0
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "dp")}
    shapes = {"jp": (B, nd, spec.ng), "hp": (B, nd, spec.nw), "dXp": (B, nd, spec.nX), "gp": (B, spec.np)}

    def run(keys, dp=dev["dp"]):
        out = {k: torch.full(shapes[k], float("nan"), **f64) for k in keys}
        s.param_products_device(dev["w"], dev["p"], dp, out, lam_g=dev["lam_g"], obj_factor=0.37)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    want = {k: (full[k].T if k == "gp" else np.transpose(full[k], (2, 1, 0))) for k in KEYS}
    for n in range(1, 5):
        for keys in itertools.combinations(KEYS, n):
            got = run(keys)
            for k in keys:
                np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k} of {keys}")
    np.testing.assert_array_equal(run(("gp",), dp=None)["gp"], want["gp"])
    host0 = s.param_products(d["w"].T, d["p"].T, None, lam_g=d["lam_g"].T, obj_factor=0.37)
    assert list(host0) == ["gp"]
    np.testing.assert_array_equal(host0["gp"], full["gp"])
    # a tail entry of p that no obstacle or weight index names
    spec2 = dataclasses.replace(er.case_spec("dynamic"), np=18).validate()
    s2 = _solver(spec2)
    d2 = er.draw_point(er.case_spec("dynamic"), 3, seed=83)
    d2["p"] = np.concatenate([d2["p"], np.full((3, 1), 5.0)], axis=1)
    d2["dp"] = qr.draw_directions(er.problem_of(spec2), d2["p"], nd, seed=84)
    ref2 = _pp(s2, d2)
    assert np.all(ref2["gp"][17] == 0.0) and np.all(ref2["gp"][11:17] != 0.0)
    dn = d2["dp"].copy()
    dn[:, :, 17] = np.nan
    dn[:, :, 10] = np.nan
    _equal(_pp(s2, d2, dp=_t(dn)), ref2, "NaN in an unnamed tail entry")


def test_param_products_device_does_not_synchronise():
    """nmpc_param_products_batch_dev only enqueues (the pattern of
    tests/test_gpu_products.py::test_products_device_does_not_synchronise): behind a spinning
    kernel on a side stream the call returns while the stream is still busy, and the results
    equal an unobstructed run's.  After a solve of the same B it allocates nothing."""
    import time
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, nd = 64, 3
    d = er.draw_point(spec, B, seed=9)
    d["dp"] = qr.draw_directions(er.problem_of(spec), d["p"], nd, seed=10)
    s(x0=np.zeros(spec.nw), lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], p=d["p"].T)  # a solve of the same B
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "dp")}
    st = torch.cuda.Stream()

    def outs():
        return {"jp": torch.empty(B, nd, spec.ng, **f64), "hp": torch.empty(B, nd, spec.nw, **f64),
                "dXp": torch.empty(B, nd, spec.nX, **f64), "gp": torch.empty(B, spec.np, **f64)}

    def go(o):
        s.param_products_device(dev["w"], dev["p"], dev["dp"], o, lam_g=dev["lam_g"], stream=st)

    ref = outs()
    go(ref)
    torch.cuda.synchronize()
    assert s.memory_info() == mem  # the solve's workspace covers the products
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st); torch.cuda._sleep(1 << 22); e1.record(st)
    torch.cuda.synchronize()
    per_cycle_ms = e0.elapsed_time(e1) / (1 << 22)
    cycles = int(min(max(400.0 / max(per_cycle_ms, 1e-12), float(1 << 22)), float(1 << 34)))  # ~0.4 s
    o = outs()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(st):
        e0.record(st)
        torch.cuda._sleep(cycles)
        e1.record(st)
    t0 = time.perf_counter()
    go(o)
    call_ms = (time.perf_counter() - t0) * 1e3
    busy = not st.query()
    torch.cuda.synchronize()
    spin_ms = e0.elapsed_time(e1)
    print(f"param_products_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info() == mem
    for k in o:
        np.testing.assert_array_equal(o[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=k)


def test_argument_validation_on_a_live_handle():
    from nmpc_amd import _lib

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    L = _lib.lib()
    B, nd = 2, 2
    d = er.draw_point(spec, B, seed=5)
    dp_t = C.POINTER(C.c_double)
    w, p, lg = (np.ascontiguousarray(d[k]) for k in ("w", "p", "lam_g"))
    dp = qr.draw_directions(er.problem_of(spec), p, nd, seed=6)
    out = {"jp": np.full((B, nd, spec.ng), 7.0), "hp": np.full((B, nd, spec.nw), 7.0),
           "dXp": np.full((B, nd, spec.nX), 7.0), "gp": np.full((B, spec.np), 7.0)}
    ptr = lambda a: a.ctypes.data_as(dp_t)  # noqa: E731
    outs = [ptr(out[k]) for k in KEYS]

    def call(B_=B, nd_=nd, x=ptr(w), ld_x=spec.nw, p_=ptr(p), ld_p=spec.np, lam=ptr(lg), ld_lam=spec.ng, d_=ptr(dp),
             ld_dp=spec.np * nd, o=outs, dev=False, h=s._h):
        a = (h, B_, nd_, x, ld_x, p_, ld_p, lam, ld_lam, 1.0, d_, ld_dp, *o)
        # on the device entry point the checks return before anything reads a pointer
        return L.nmpc_param_products_batch_dev(*a, None) if dev else L.nmpc_param_products_batch(*a)

    gp_only = [None, None, None, outs[3]]
    # the full message of every rule, on both entry points; the last four break two rules at
    # once: the earlier one in the order of the checks answers
    nd0 = "nd = 0 takes gp_out alone (dp and the directional outputs must be null)"
    for dev in (False, True):
        for what, kw, msg in (
                ("null handle", dict(h=None), "null handle"), ("B = 0", dict(B_=0), "B <= 0"),
                ("nd < 0", dict(nd_=-1), "nd < 0"), ("x NULL", dict(x=None), "required pointer is null (x, p)"),
                ("no output", dict(o=[None] * 4), "every output pointer is null"),
                ("hp with nd = 0", dict(nd_=0, d_=None, o=[None, outs[1], None, None]), nd0),
                ("dp with nd = 0", dict(nd_=0, o=gp_only), nd0),
                ("directional output, dp NULL", dict(d_=None), "required pointer is null (dp with nd > 0)"),
                ("ld_dp short", dict(ld_dp=spec.np * nd - 1), "leading dimension smaller than the vector length"),
                ("B = 0 and nd < 0", dict(B_=0, nd_=-1), "B <= 0"),
                ("nd < 0 and p NULL", dict(nd_=-1, p_=None), "nd < 0"),
                ("no output and dp NULL", dict(o=[None] * 4, d_=None), "every output pointer is null"),
                ("dp NULL and ld_x short", dict(d_=None, ld_x=spec.nw - 1),
                 "required pointer is null (dp with nd > 0)")):
            assert call(dev=dev, **kw) == -1, (what, dev)
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    for what, rc in (("B = 0", call(B_=0)), ("B < 0", call(B_=-3)), ("nd < 0", call(nd_=-1)),
                     ("x NULL", call(x=None)), ("p NULL", call(p_=None)), ("no output", call(o=[None] * 4)),
                     ("jp with nd = 0", call(nd_=0, d_=None, o=[outs[0], None, None, outs[3]])),
                     ("hp with nd = 0", call(nd_=0, d_=None, o=[None, outs[1], None, None])),
                     ("dXp with nd = 0", call(nd_=0, d_=None, o=[None, None, outs[2], None])),
                     ("dp with nd = 0", call(nd_=0, o=gp_only)),
                     ("directional output, dp NULL", call(d_=None)),
                     ("gp alone, nd > 0, dp NULL", call(d_=None, o=gp_only)),
                     ("ld_x short", call(ld_x=spec.nw - 1)), ("ld_p short", call(ld_p=spec.np - 1)),
                     ("ld_lam_g short", call(ld_lam=spec.ng - 1)), ("ld_dp short", call(ld_dp=spec.np * nd - 1)),
                     ("ld_dp one direction", call(ld_dp=spec.np)), ("ld_x negative", call(ld_x=-spec.nw))):
        assert rc == -1, (what, rc)  # NMPC_E_INVALID
        assert L.nmpc_last_error(), what
    call(o=[None] * 4)
    assert "output" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(nd_=-1))
    assert all(np.all(out[k] == 7.0) for k in KEYS)  # nothing ran
    # the same checks on the device entry point (null device pointers are never dereferenced)
    vp = C.c_void_p
    z = [vp(0), 0]
    assert L.nmpc_param_products_batch_dev(s._h, 2, 2, *z, *z, *z, 1.0, *z, vp(0), vp(0), vp(0), vp(0), vp(0)) == -1
    assert L.nmpc_param_products_batch_dev(None, 2, 2, *z, *z, *z, 1.0, *z, vp(0), vp(0), vp(0), vp(0), vp(0)) == -1
    # and the handle still works: nd = 0 with gp alone; leading dimension 0 shares x, p, lam_g and dp
    assert call(nd_=0, d_=None, ld_dp=0, o=gp_only) == 0
    assert np.all(np.isfinite(out["gp"])) and all(np.all(out[k] == 7.0) for k in KEYS[:3])
    assert call(ld_x=0, ld_p=0, ld_lam=0, ld_dp=0) == 0
    assert all(np.all(np.isfinite(out[k])) for k in KEYS)
    for k in KEYS:
        np.testing.assert_array_equal(out[k][0], out[k][1])


def _parent_sensitivity(s, sol, lbx, ubx, lbg, ubg, p, dp, fd_step=1e-3):
    """Solver.sensitivity as it stood before the exact tangent existed: central differences of
    evaluate, then the delta ladder."""
    d = np.asarray(dp, dtype=np.float64)
    x = np.asarray(sol["x"], dtype=np.float64).reshape(s.nw, -1)
    lam = np.asarray(sol["lam_g"], dtype=np.float64).reshape(s.ng, -1)
    B, nd = x.shape[1], d.shape[1]
    P = np.asarray(p, dtype=np.float64).reshape(s.np, -1) * np.ones((1, B))
    d = np.repeat(d[:, :, None], B, axis=2)
    sx, ss = s.barrier_weights(sol, lbx, ubx, lbg, ubg)
    dgl, dg = np.empty((s.nw, nd, B)), np.empty((s.ng, nd, B))
    for j in range(nd):
        ep = s.evaluate(x, P + fd_step * d[:, j, :], lam_g=lam)
        em = s.evaluate(x, P - fd_step * d[:, j, :], lam_g=lam)
        dgl[:, j, :] = (ep["grad_l"] - em["grad_l"]) / (2 * fd_step)
        dg[:, j, :] = (ep["g"] - em["g"]) / (2 * fd_step)
    first, inc_first, inc, dmax = s._perturb
    delta = np.zeros(B)
    while True:
        r = s.kkt_solve(x, P, r_w=-dgl, r_g=-(ss[:, None, :] * dg), lam_g=lam, sigma_x=sx, sigma_s=ss, delta=delta)
        retry = r["info"] == 1
        nxt = np.where(delta == 0.0, first, np.where(delta == first, inc_first * delta, inc * delta))
        retry &= nxt <= dmax
        if not np.any(retry):
            break
        delta = np.where(retry, nxt, delta)
    return {"dx": r["dw"], "dlam_g": ss[:, None, :] * (r["jdw"] + dg), "info": r["info"], "delta": delta}


def test_exact_sensitivity_of_a_solution():
    """race_track_2, N = 6, four scenarios, seed 7, d/dx0 in 8 directions (the case of
    tests/test_gpu_kkt.py::test_sensitivity_of_a_solution).  sensitivity(tangent="exact")
    against the same formula evaluated densely on the oracle with the checker's analytic
    d_p grad_w L and dg/dp and the same delta: normwise residual rho <= 1e-10.  Its distance to
    tangent="fd" at the default step is printed, not bounded tightly (the differences'
    truncation).  The default call is bitwise the formula as it stood before."""
    from nmpc_amd import draw_scenarios
    from oracle import nmpc_oracle as orc

    spec = er.case_spec("race_track_2")
    prob = er.problem_of(spec)
    s = _solver(spec)
    B, nd = 4, 8
    P = draw_scenarios(spec, B, seed=7)
    lbx, ubx, lbg, ubg = spec.bounds()
    sol = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    assert np.all(np.isin(s.stats()["status_code"], (0, 1)))
    dp = np.eye(spec.np)[:, :nd]
    got = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="exact")
    assert got["dx"].shape == (spec.nw, nd, B) and got["dlam_g"].shape == (spec.ng, nd, B)
    print(f"exact sensitivity: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    same = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, fd_step=123.0, tangent="exact")  # fd_step is ignored
    _equal({k: got[k] for k in got}, same, "fd_step ignored")
    fd = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp)
    for b in range(B):
        x, lam, lx = sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b]
        ev = orc.SSEval(prob, x, P[b])
        dn = qr.dense(ev, 1.0, lam)
        sx = kr.barrier_weights(x, lx, lbx, ubx)
        ss = kr.barrier_weights(ev.g, lam, lbg, ubg)
        free = np.isfinite(sx)
        M = kr.dense_M(ev, ev.hessian(1.0, lam), np.where(free, sx, 0.0), ss, got["delta"][b])
        Mf = M[np.ix_(free, free)]
        dgl, dg = (dn["C"] @ dp).T, (dn["Jp"] @ dp).T  # (nd, nw), (nd, ng)
        rhs = -dgl - (ss * dg) @ ev.J
        dx = got["dx"][:, :, b].T
        assert np.all(dx[:, ~free] == 0.0)
        r = max(kr.rho(Mf, dx[j, free], rhs[j, free]) for j in range(nd))
        ref_dx = np.zeros((nd, spec.nw))
        ref_dx[:, free] = np.linalg.solve(Mf, rhs[:, free].T).T
        ref_dl = ss * (ref_dx @ ev.J.T + dg)
        f = float(np.max(np.abs(dx - ref_dx)) / np.max(np.abs(ref_dx)))
        fl = float(np.max(np.abs(got["dlam_g"][:, :, b].T - ref_dl)) / max(np.max(np.abs(ref_dl)), 1e-300))
        to_fd = float(np.max(np.abs(dx - fd["dx"][:, :, b].T)) / np.max(np.abs(dx)))
        print(f"exact sensitivity scenario {b}: rho {r:.2e} (bound {kr.TOL:.0e}), forward dx {f:.2e}, dlam_g {fl:.2e}, "
              f"cond {float(np.linalg.cond(Mf)):.1e}; distance to tangent='fd' (step 1e-3) {to_fd:.2e} of max |dx|")
        assert r <= kr.TOL, (b, r)
    # the default path is what it was
    _equal(fd, _parent_sensitivity(s, sol, lbx, ubx, lbg, ubg, P.T, dp), "default path")
    with pytest.raises(ValueError):
        s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="analytic")
