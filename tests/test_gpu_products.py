"""nmpc_products_batch / nmpc_products_batch_dev (Solver.products, products_device, jacobian,
hessian): J_g v, the Lagrangian Hessian times v and the rollout's tangent at given points, on
the GPU, against the oracle's SSEval (tests/products_ref.py: directions, scales, tolerance)."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_ref as er
from tests import products_ref as pr

pytestmark = pytest.mark.gpu

KEYS = ("jv", "hv", "dX")


def _solver(spec):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)


def _vt(v):
    """(B, nv, nw) -> Solver.products' (nw, nv, B)."""
    return np.ascontiguousarray(np.transpose(v, (2, 1, 0)))


def _products(s, d, sel=slice(None), sigma=1.0, lam=True, v=None):
    v = _vt(d["v"][sel]) if v is None else v
    return s.products(d["w"][sel].T, d["p"][sel].T, v, lam_g=d["lam_g"][sel].T if lam else None, obj_factor=sigma)


def _scn(res, b):
    return {k: res[k][:, :, b].T for k in res}


@pytest.mark.parametrize("name", list(er.CASES))
def test_products_match_the_oracle(name):
    """jv, hv and dX of every case (both models, N = 1 / 63, 16 obstacles, obstacle
    coordinates and cost weights from p), nv = 3, for (obj_factor, lam_g) = (1, random),
    (0.37, random), (0, random), (1, NULL): within 1e-10 of the oracle's relative to the
    absolute-product scales of tests/products_ref.py."""
    spec, d, ref = pr.reference(name)
    s = _solver(spec)
    B = er.CASES[name]
    for combo in pr.COMBOS:
        res = _products(s, d, sigma=combo[0], lam=combo[1])
        assert res["jv"].shape == (spec.ng, pr.NV, B) and res["hv"].shape == (spec.nw, pr.NV, B)
        assert res["dX"].shape == (spec.nX, pr.NV, B)
        for b in range(B):
            pr.check_against(_scn(res, b), ref[combo][b], f"{name} {combo} scenario {b}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_dense_jacobian_and_hessian(name):
    """Solver.jacobian / hessian (identity directions shared by the batch, ld_v = 0) against
    SSEval.J and SSEval.hessian, each column relative to its own absolute scale.  W is
    symmetric within the tolerance (W_ij is a result of column j, W_ji of column i, each within
    TOL of its column's scale).  Exactly 0.0: J's stage-0 rows; J's entries of stage k with
    respect to u_j, j >= k; the tangent of stages <= j for direction e_{u_j}; and, with N = 1
    and no multipliers, all of W."""
    spec, d, _ = pr.reference(name)
    _, _, evs = pr.evals(name)
    s = _solver(spec)
    B, nw, N, m = er.CASES[name], spec.nw, spec.N, spec.ng // (spec.N + 1)
    nu, nx = nw // N, spec.nX // (N + 1)
    J = s.jacobian(d["w"].T, d["p"].T)
    W = s.hessian(d["w"].T, d["p"].T, lam_g=d["lam_g"].T, obj_factor=1.0)
    assert J.shape == (spec.ng, nw, B) and W.shape == (nw, nw, B)
    eye = np.eye(nw)
    dX = s.products(d["w"].T, d["p"].T, eye)["dX"]
    assert dX.shape == (spec.nX, nw, B)
    for b in range(B):
        ref = pr.cpu_products(evs[b], eye, 1.0, d["lam_g"][b])
        pr.check_against({"jv": J[:, :, b].T, "hv": W[:, :, b].T, "dX": dX[:, :, b].T}, ref,
                         f"{name} dense scenario {b}")
        sc = ref["scale"]["hv"]
        asym = np.abs(W[:, :, b] - W[:, :, b].T)
        bound = pr.TOL * (sc[:, None] + sc[None, :])
        print(f"{name} scenario {b}: asymmetry / bound {float(np.max(asym / np.maximum(bound, 1e-300))):.2e}")
        assert np.all(asym <= bound)
    assert np.all(J[:m] == 0.0)
    for k in range(1, N + 1):
        assert np.all(J[k * m:(k + 1) * m, k * nu:] == 0.0), k
    for j in range(N):
        assert np.all(dX[:(j + 1) * nx, j * nu:(j + 1) * nu] == 0.0), j
    if N == 1:
        W0 = s.hessian(d["w"].T, d["p"].T)
        assert np.all(W0 == 0.0)
        assert np.any(W != 0.0)  # the last stage's row curvature is the only contribution


def test_consistency_with_the_evaluation():
    """Without the oracle's derivatives: central differences (h = 1e-4) of Solver.evaluate's
    grad_l (lam_x absent) and g along v against hv (obj_factor 1) and jv.  The difference
    quotient's own truncation error is measured on SSEval alone -- the same quotient of its
    gradients against its own W v and J v -- and the GPU's discrepancy may be up to 10x that
    (the rounding of a different operation order) plus TOL * scale."""
    from oracle import nmpc_oracle as orc

    name, h = "race_track_2", 1e-4
    spec, d, ref = pr.reference(name)
    prob = er.problem_of(spec)
    s = _solver(spec)
    B = er.CASES[name]
    res = _products(s, d)
    for dd in range(pr.NV):
        step = h * d["v"][:, dd, :]
        ep = s.evaluate((d["w"] + step).T, d["p"].T, lam_g=d["lam_g"].T)
        em = s.evaluate((d["w"] - step).T, d["p"].T, lam_g=d["lam_g"].T)
        for b in range(B):
            cp_, cm = orc.SSEval(prob, d["w"][b] + step[b], d["p"][b]), orc.SSEval(prob, d["w"][b] - step[b], d["p"][b])
            lg = d["lam_g"][b]
            r = ref[pr.COMBOS[0]][b]
            for key, gp, gm, op, om in (("hv", ep["grad_l"][:, b], em["grad_l"][:, b], cp_.gradF + cp_.J.T @ lg,
                                         cm.gradF + cm.J.T @ lg),
                                        ("jv", ep["g"][:, b], em["g"][:, b], cp_.g, cm.g)):
                own = float(np.max(np.abs((op - om) / (2 * h) - r[key][dd])))
                got = float(np.max(np.abs((gp - gm) / (2 * h) - res[key][:, dd, b])))
                bound = 10.0 * own + pr.TOL * r["scale"][key][dd]
                print(f"{key} direction {dd} scenario {b}: GPU quotient vs GPU product {got:.2e}, oracle quotient vs "
                      f"oracle product {own:.2e}, bound {bound:.2e}")
                assert got <= bound, (key, dd, b, got, bound)


def test_batch_plumbing():
    """All bitwise: a scenario of a batch of 130 equals its B = 1 call; a per-scenario copy of
    shared directions equals the broadcast; nv = 3 equals three nv = 1 calls (and a NaN in
    direction 1 leaves directions 0 and 2 finite and unchanged); an absent output leaves the
    others unchanged; host and device entry points agree."""
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, nv = 130, 3
    d = er.draw_point(spec, B, seed=78)
    d["v"] = pr.draw_directions(spec, nv, B, seed=79)
    full = _products(s, d, sigma=0.37)
    assert all(np.all(np.isfinite(full[k])) for k in KEYS)
    for b in (0, 64, 129):
        one = _products(s, d, slice(b, b + 1), sigma=0.37)
        for k in KEYS:
            np.testing.assert_array_equal(one[k][:, :, 0], full[k][:, :, b], err_msg=f"{k} scenario {b}")
    # shared directions: broadcast (ld_v = 0) against a copy per scenario
    v0 = np.ascontiguousarray(d["v"][0].T)  # (nw, nv)
    shared = _products(s, d, sigma=0.37, v=v0)
    tiled = _products(s, d, sigma=0.37, v=np.ascontiguousarray(np.repeat(v0[:, :, None], B, axis=2)))
    for k in KEYS:
        np.testing.assert_array_equal(shared[k], tiled[k], err_msg=k)
    one_d = _products(s, d, sigma=0.37, v=v0[:, 0])  # a single direction as a vector
    for k in KEYS:
        np.testing.assert_array_equal(one_d[k][:, 0], shared[k][:, 0], err_msg=k)
    # directions are independent
    for dd in range(nv):
        single = _products(s, d, sigma=0.37, v=_vt(d["v"][:, dd:dd + 1]))
        for k in KEYS:
            np.testing.assert_array_equal(single[k][:, 0], full[k][:, dd], err_msg=f"{k} direction {dd}")
    vn = d["v"].copy()
    vn[:, 1, 0] = np.nan  # the first control of direction 1, every scenario
    poisoned = _products(s, d, sigma=0.37, v=_vt(vn))
    for k in KEYS:
        np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=k)
        assert np.all(np.any(np.isnan(poisoned[k][:, 1]), axis=0)), k
    # device entry point: everything, then subsets of the outputs
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "v")}
    shapes = {"jv": (B, nv, spec.ng), "hv": (B, nv, spec.nw), "dX": (B, nv, spec.nX)}

    def run(keys):
        out = {k: torch.full(shapes[k], float("nan"), **f64) for k in keys}
        s.products_device(dev["w"], dev["p"], dev["v"], out, lam_g=dev["lam_g"], obj_factor=0.37)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    for keys in (KEYS, ("jv",), ("hv",), ("dX",), ("jv", "dX")):
        got = run(keys)
        for k in keys:
            np.testing.assert_array_equal(got[k], np.transpose(full[k], (2, 1, 0)), err_msg=f"{k} of {keys}")


def test_products_device_does_not_synchronise():
    """nmpc_products_batch_dev only enqueues (the pattern of
    tests/test_gpu_eval.py::test_evaluate_device_does_not_synchronise): behind a spinning
    kernel on a side stream the call returns while the stream is still busy, and the results
    equal an unobstructed run's.  After a solve of the same B it allocates nothing."""
    import time
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, nv = 64, 3
    d = er.draw_point(spec, B, seed=9)
    d["v"] = pr.draw_directions(spec, nv, B, seed=10)
    s(x0=np.zeros(spec.nw), lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], p=d["p"].T)  # a solve of the same B
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "v")}
    st = torch.cuda.Stream()

    def outs():
        return {"jv": torch.empty(B, nv, spec.ng, **f64), "hv": torch.empty(B, nv, spec.nw, **f64),
                "dX": torch.empty(B, nv, spec.nX, **f64)}

    def go(o):
        s.products_device(dev["w"], dev["p"], dev["v"], o, lam_g=dev["lam_g"], stream=st)

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
    print(f"products_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
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
    B, nv = 2, 2
    d = er.draw_point(spec, B, seed=5)
    dp = C.POINTER(C.c_double)
    w, p, lg = (np.ascontiguousarray(d[k]) for k in ("w", "p", "lam_g"))
    v = pr.draw_directions(spec, nv, B, seed=6)
    out = {"jv": np.full((B, nv, spec.ng), 7.0), "hv": np.full((B, nv, spec.nw), 7.0),
           "dX": np.full((B, nv, spec.nX), 7.0)}
    ptr = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    outs = [ptr(out[k]) for k in KEYS]

    def call(B_=B, nv_=nv, x=ptr(w), ld_x=spec.nw, p_=ptr(p), ld_p=spec.np, lam=ptr(lg), ld_lam=spec.ng, v_=ptr(v),
             ld_v=spec.nw * nv, o=outs, dev=False, h=s._h):
        if dev:  # the checks return before anything reads a pointer
            return L.nmpc_products_batch_dev(h, B_, nv_, x, ld_x, p_, ld_p, lam, ld_lam, 1.0, v_, ld_v, *o, None)
        return L.nmpc_products_batch(h, B_, nv_, x, ld_x, p_, ld_p, lam, ld_lam, 1.0, v_, ld_v, *o)

    # the full message of every rule, on both entry points; the last four break two rules at
    # once: the earlier one in the order of the checks answers
    for dev in (False, True):
        for what, kw, msg in (
                ("null handle", dict(h=None), "null handle"), ("B = 0", dict(B_=0), "B <= 0"),
                ("nv = 0", dict(nv_=0), "nv <= 0"), ("v NULL", dict(v_=None), "required pointer is null (x, p, v)"),
                ("x NULL", dict(x=None), "required pointer is null (x, p, v)"),
                ("no output", dict(o=[None] * 3), "every output pointer is null"),
                ("ld_v short", dict(ld_v=spec.nw * nv - 1), "leading dimension smaller than the vector length"),
                ("B = 0 and nv = 0", dict(B_=0, nv_=0), "B <= 0"),
                ("nv = 0 and p NULL", dict(nv_=0, p_=None), "nv <= 0"),
                ("v NULL and no output", dict(v_=None, o=[None] * 3), "required pointer is null (x, p, v)"),
                ("no output and ld_x short", dict(o=[None] * 3, ld_x=spec.nw - 1), "every output pointer is null")):
            assert call(dev=dev, **kw) == -1, (what, dev)
            assert L.nmpc_last_error().decode() == msg, (what, dev)

    for what, rc in (("B = 0", call(B_=0)), ("B < 0", call(B_=-3)), ("nv = 0", call(nv_=0)), ("nv < 0", call(nv_=-1)),
                     ("x NULL", call(x=None)), ("p NULL", call(p_=None)), ("v NULL", call(v_=None)),
                     ("no output", call(o=[None] * 3)),
                     ("ld_x short", call(ld_x=spec.nw - 1)), ("ld_p short", call(ld_p=spec.np - 1)),
                     ("ld_lam_g short", call(ld_lam=spec.ng - 1)), ("ld_v short", call(ld_v=spec.nw * nv - 1)),
                     ("ld_v one direction", call(ld_v=spec.nw)), ("ld_x negative", call(ld_x=-spec.nw))):
        assert rc == -1, (what, rc)  # NMPC_E_INVALID
        assert L.nmpc_last_error(), what
    call(o=[None] * 3)
    assert "output" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(nv_=0))
    assert all(np.all(out[k] == 7.0) for k in KEYS)  # nothing ran
    # the same checks on the device entry point (null device pointers are never dereferenced)
    vp = C.c_void_p
    assert L.nmpc_products_batch_dev(s._h, 2, 2, vp(0), 0, vp(0), 0, vp(0), 0, 1.0, vp(0), 0, vp(0), vp(0), vp(0),
                                     vp(0)) == -1
    assert L.nmpc_products_batch_dev(None, 2, 2, vp(0), 0, vp(0), 0, vp(0), 0, 1.0, vp(0), 0, vp(0), vp(0), vp(0),
                                     vp(0)) == -1
    # and the handle still works: leading dimension 0 shares x, p, lam_g and v
    assert call(ld_x=0, ld_p=0, ld_lam=0, ld_v=0) == 0
    assert all(np.all(np.isfinite(out[k])) for k in KEYS)
    for k in KEYS:
        np.testing.assert_array_equal(out[k][0], out[k][1])
