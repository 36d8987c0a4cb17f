"""nmpc_kkt_solve_batch / nmpc_kkt_solve_batch_dev (Solver.kkt_solve, kkt_solve_device,
barrier_weights, sensitivity): solves with the condensed KKT matrix at given points, on the GPU,
against the dense matrix of the oracle's SSEval (tests/kkt_ref.py: weights, delta, right-hand
sides, the residual gate and its bound)."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_ref as er
from tests import kkt_ref as kr

pytestmark = pytest.mark.gpu

KEYS = ("dw", "dX", "jdw")


def _solver(spec):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)


def _t(a):
    """(B, nr, n) -> Solver.kkt_solve's (n, nr, B)."""
    return np.ascontiguousarray(np.transpose(a, (2, 1, 0)))


def _solve(s, inp, sel=slice(None), **over):
    a = {"r_w": _t(inp["r_w"][sel]), "r_g": _t(inp["r_g"][sel]), "lam_g": inp["lam_g"][sel].T,
         "obj_factor": inp["obj_factor"], "sigma_x": inp["sigma_x"][sel].T, "sigma_s": inp["sigma_s"][sel].T,
         "delta": inp["delta"][sel]}
    a.update(over)
    return s.kkt_solve(inp["x"][sel].T, inp["p"][sel].T, **a)


def _all_nan(res, b):
    return all(np.all(np.isnan(res[k][:, :, b])) for k in KEYS)


@pytest.mark.parametrize("regime", kr.REGIMES)
@pytest.mark.parametrize("name", list(er.CASES))
def test_steps_match_the_dense_matrix(name, regime):
    """Every case (both models, N = 1 / 63, 16 obstacles, obstacle coordinates and cost weights
    from p) in both weight regimes, three right-hand sides (r_w alone, r_g alone, both), for
    (obj_factor, lam_g) = (1, random) and (0.37, random), delta from the checker: info = 0, the
    residual against the dense M within 1e-10, the forward error within 1e-6 in the mild
    regime, and dX, J dw equal to the oracle's Z and J applied to the GPU's own dw."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, regime, combo)
        s = _solver(spec)
        B = er.CASES[name]
        res = _solve(s, inp)
        assert res["dw"].shape == (spec.nw, kr.NR, B) and res["dX"].shape == (spec.nX, kr.NR, B)
        assert res["jdw"].shape == (spec.ng, kr.NR, B) and res["info"].shape == (B,)
        print(f"{name} {regime} obj {combo[0]}: info {res['info']}, delta {inp['delta']}")
        assert np.all(res["info"] == 0)
        for b in range(B):
            what = f"{name} {regime} obj {combo[0]} scenario {b}"
            dw = res["dw"][:, :, b].T
            kr.check_solution(dw, per[b], regime, what)
            kr.check_steps(evs[b], dw, res["dX"][:, :, b].T, res["jdw"][:, :, b].T, what)
        m = spec.ng // (spec.N + 1)
        nx = spec.nX // (spec.N + 1)
        assert np.all(res["jdw"][:m] == 0.0) and np.all(res["dX"][:nx] == 0.0)  # stage 0: exactly 0


@pytest.mark.parametrize("name", ["race_track_2", "nmpc_tt", "dynamic"])
def test_inertia_verdict(name):
    """sigma = 0, delta = 0, lam_g random: every scenario whose dense M has lambda_min below
    -1e-3 max|M| reports 1 with all-NaN outputs (scenarios inside the margin are not judged; the
    positive definite side is the parity test's info = 0)."""
    spec, inp, ratio = kr.indefinite_cases(name)
    s = _solver(spec)
    res = s.kkt_solve(inp["x"].T, inp["p"].T, r_w=np.ones(spec.nw), lam_g=inp["lam_g"].T)
    judged = ratio < -kr.INDEF
    print(f"{name}: lambda_min / max|M| {ratio}, info {res['info']}")
    assert np.any(judged)
    for b in np.flatnonzero(judged):
        assert res["info"][b] == 1 and _all_nan(res, b), b
    for b in np.flatnonzero(res["info"] == 0):
        assert ratio[b] > -kr.INDEF and np.all(np.isfinite(res["dw"][:, :, b]))


def test_fixed_variables_leave_the_system():
    """sigma_x = +inf on the gimbal rates of every stage and on random other entries: those dw
    are exactly 0, the rest meets the residual gate on the reduced dense system."""
    name, regime = "race_track_2", "mild"
    spec, inp, per, evs = kr.reference(name, regime, kr.COMBOS[0])
    s = _solver(spec)
    B, nw = er.CASES[name], spec.nw
    rng = np.random.default_rng(11)
    fx = rng.uniform(size=(B, nw)) < 0.15
    fx[:, np.arange(nw) % 6 >= 3] = True
    fx[0, :6] = True  # a whole stage
    sx = np.where(fx, np.inf, inp["sigma_x"])
    res = _solve(s, inp, sigma_x=sx.T)
    assert np.all(res["info"] == 0)
    for b in range(B):
        dw = res["dw"][:, :, b].T
        assert np.all(dw[:, fx[b]] == 0.0), b
        fr = ~fx[b]
        M, rhs = per[b]["M"][np.ix_(fr, fr)], per[b]["rhs"][:, fr]
        r = max(kr.rho(M, dw[c, fr], rhs[c]) for c in range(kr.NR))
        ref = np.linalg.solve(M, rhs.T).T
        f = float(np.max(np.abs(dw[:, fr] - ref) / np.max(np.abs(ref), axis=1, keepdims=True)))
        print(f"{name} fixed scenario {b}: {int(fx[b].sum())} of {nw} fixed, rho {r:.2e}, forward {f:.2e}")
        assert r <= kr.TOL and f <= kr.FWD_TOL
        kr.check_steps(evs[b], dw, res["dX"][:, :, b].T, res["jdw"][:, :, b].T, f"{name} fixed scenario {b}")


def test_invalid_weights_end_their_scenario_only():
    """A negative sigma, a NaN delta or an infinite sigma_s in one scenario gives -11 and NaN
    outputs there; every other scenario's results are bitwise unchanged.  Stage 0's rows are
    never read: anything there changes nothing."""
    name = "race_track_2"
    spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
    s = _solver(spec)
    B, m = er.CASES[name], spec.ng // (spec.N + 1)
    clean = _solve(s, inp)
    assert np.all(clean["info"] == 0)
    sx, ss, dl = inp["sigma_x"].copy(), inp["sigma_s"].copy(), inp["delta"].copy()
    sx[1, 7] = -1e-3
    dl[3] = np.nan
    ss[4, m + 2] = np.inf
    sx[6, 0] = np.nan
    ss[6, spec.ng - 1] = -1.0
    bad = [1, 3, 4, 6]
    res = _solve(s, inp, sigma_x=sx.T, sigma_s=ss.T, delta=dl)
    print(f"invalid weights: info {res['info']}")
    for b in range(B):
        if b in bad:
            assert res["info"][b] == -11 and _all_nan(res, b), b
        else:
            assert res["info"][b] == 0
            for k in KEYS:
                np.testing.assert_array_equal(res[k][:, :, b], clean[k][:, :, b], err_msg=f"{k} scenario {b}")
    neg = _solve(s, inp, delta=np.full(B, -1e-8))
    assert np.all(neg["info"] == -11)
    # stage 0's rows: weights and right-hand sides without effect, never formed
    ss0, rg0 = inp["sigma_s"].copy(), inp["r_g"].copy()
    ss0[:, :m] = np.nan
    rg0[:, :, :m] = np.nan
    res0 = _solve(s, inp, sigma_s=ss0.T, r_g=_t(rg0))
    assert np.all(res0["info"] == 0)
    for k in KEYS:
        np.testing.assert_array_equal(res0[k], clean[k], err_msg=k)


def test_right_hand_sides_are_independent_and_batch_plumbing():
    """All bitwise: a NaN right-hand side poisons its own column only; nr = 3 equals three
    nr = 1 calls; ld = 0 sharing (right-hand sides, weights, delta) equals the replicated call;
    an absent right-hand side equals a zero one; a scenario of the batch equals its B = 1
    call; absent outputs leave the others unchanged; host and device entry points agree."""
    import torch

    name = "race_track_2"
    spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
    s = _solver(spec)
    B, nr = er.CASES[name], kr.NR
    full = _solve(s, inp)
    rw = inp["r_w"].copy()
    rw[:, 1, 3] = np.nan
    rg = inp["r_g"].copy()
    rg[:, 1, -1] = np.nan
    for over in ({"r_w": _t(rw)}, {"r_g": _t(rg)}):
        poisoned = _solve(s, inp, **over)
        assert np.all(poisoned["info"] == 0)
        for k in KEYS:
            np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=k)
        assert np.all(np.any(np.isnan(poisoned["dw"][:, 1]), axis=0))
    for c in range(nr):
        one = _solve(s, inp, r_w=_t(inp["r_w"][:, c:c + 1]), r_g=_t(inp["r_g"][:, c:c + 1]))
        for k in KEYS:
            np.testing.assert_array_equal(one[k][:, 0], full[k][:, c], err_msg=f"{k} column {c}")
    # column 0 has r_g = 0 and column 1 r_w = 0: an absent right-hand side is a zero one
    only_w = _solve(s, inp, r_w=_t(inp["r_w"][:, 0:1]), r_g=None)
    only_g = _solve(s, inp, r_w=None, r_g=_t(inp["r_g"][:, 1:2]))
    for k in KEYS:
        np.testing.assert_array_equal(only_w[k][:, 0], full[k][:, 0], err_msg=k)
        np.testing.assert_array_equal(only_g[k][:, 0], full[k][:, 1], err_msg=k)
    # shared (leading dimension 0) against replicated
    big = float(np.max(inp["delta"])) + 1.0
    sh = {"r_w": inp["r_w"][0].T, "r_g": inp["r_g"][0].T, "sigma_x": inp["sigma_x"][0], "sigma_s": inp["sigma_s"][0],
          "delta": big}
    rep = {"r_w": _t(np.repeat(inp["r_w"][:1], B, axis=0)), "r_g": _t(np.repeat(inp["r_g"][:1], B, axis=0)),
           "sigma_x": np.repeat(inp["sigma_x"][:1], B, axis=0).T, "sigma_s": np.repeat(inp["sigma_s"][:1], B, axis=0).T,
           "delta": np.full(B, big)}
    a, b_ = _solve(s, inp, **sh), _solve(s, inp, **rep)
    assert np.array_equal(a["info"], b_["info"])
    for k in KEYS:
        np.testing.assert_array_equal(a[k], b_[k], err_msg=k)
    for b in (0, B - 1):
        one = _solve(s, inp, slice(b, b + 1))
        for k in KEYS:
            np.testing.assert_array_equal(one[k][:, :, 0], full[k][:, :, b], err_msg=f"{k} scenario {b}")
    # device entry point: everything, then subsets of the outputs
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(inp[k]), **f64)
           for k in ("x", "p", "lam_g", "sigma_x", "sigma_s", "delta", "r_w", "r_g")}
    shapes = {"dw": (B, nr, spec.nw), "dX": (B, nr, spec.nX), "jdw": (B, nr, spec.ng)}

    def run(keys, info=True):
        out = {k: torch.full(shapes[k], 7.0, **f64) for k in keys}
        if info:
            out["info"] = torch.full((B,), 9, dtype=torch.int32, device="cuda")
        s.kkt_solve_device(dev["x"], dev["p"], out, r_w=dev["r_w"], r_g=dev["r_g"], lam_g=dev["lam_g"],
                           obj_factor=inp["obj_factor"], sigma_x=dev["sigma_x"], sigma_s=dev["sigma_s"],
                           delta=dev["delta"])
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    for keys, info in ((KEYS, True), (("dw",), False), (("dX",), True), (("jdw",), False), (("dw", "jdw"), True)):
        got = run(keys, info)
        for k in keys:
            np.testing.assert_array_equal(got[k], np.transpose(full[k], (2, 1, 0)), err_msg=f"{k} of {keys}")
        if info:
            np.testing.assert_array_equal(got["info"], full["info"])


def test_kkt_solve_device_does_not_synchronise():
    """nmpc_kkt_solve_batch_dev only enqueues (the pattern of
    tests/test_gpu_products.py::test_products_device_does_not_synchronise): behind a spinning
    kernel the call returns while the stream is still busy, and the results equal an
    unobstructed run's.  After a solve of the same B it allocates nothing: every solver
    class's workspace holds the KKT kernel's slice."""
    import time
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, nr = 64, 2
    d = er.draw_point(spec, B, seed=9)
    rng = np.random.default_rng(12)
    s(x0=np.zeros(spec.nw), lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], p=d["p"].T)  # a solve of the same B
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g")}
    dev["r_w"] = torch.tensor(rng.standard_normal((B, nr, spec.nw)), **f64)
    dev["sigma_x"] = torch.tensor(10.0 ** rng.uniform(-3, 3, spec.nw), **f64)
    dev["delta"] = torch.tensor([50.0], **f64)
    st = torch.cuda.Stream()

    def outs():
        return {"dw": torch.empty(B, nr, spec.nw, **f64), "dX": torch.empty(B, nr, spec.nX, **f64),
                "jdw": torch.empty(B, nr, spec.ng, **f64), "info": torch.empty(B, dtype=torch.int32, device="cuda")}

    def go(o):
        s.kkt_solve_device(dev["w"], dev["p"], o, r_w=dev["r_w"], lam_g=dev["lam_g"], sigma_x=dev["sigma_x"],
                           delta=dev["delta"], stream=st)

    ref = outs()
    go(ref)
    torch.cuda.synchronize()
    assert s.memory_info() == mem  # the solve's workspace covers the KKT solves
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
    print(f"kkt_solve_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info() == mem
    assert int((ref["info"] == 0).sum()) > 0
    for k in o:
        np.testing.assert_array_equal(o[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=k)


def test_argument_validation_on_a_live_handle():
    from nmpc_amd import _lib

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    L = _lib.lib()
    B, nr = 2, 2
    d = er.draw_point(spec, B, seed=5)
    rng = np.random.default_rng(6)
    dp = C.POINTER(C.c_double)
    w, p, lg = (np.ascontiguousarray(d[k]) for k in ("w", "p", "lam_g"))
    sx, ss, dl = np.ones((B, spec.nw)), np.ones((B, spec.ng)), np.full(B, 1e6)
    rw, rg = rng.standard_normal((B, nr, spec.nw)), rng.standard_normal((B, nr, spec.ng))
    out = {"dw": np.full((B, nr, spec.nw), 7.0), "dX": np.full((B, nr, spec.nX), 7.0),
           "jdw": np.full((B, nr, spec.ng), 7.0)}
    info = np.full(B, 9, dtype=np.int32)
    ptr = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    outs = [ptr(out[k]) for k in KEYS]
    nw, ng = spec.nw, spec.ng

    def call(B_=B, nr_=nr, x=ptr(w), ld_x=nw, p_=ptr(p), ld_p=spec.np, lam=ptr(lg), ld_lam=ng, sx_=ptr(sx), ld_sx=nw,
             ss_=ptr(ss), ld_ss=ng, dl_=ptr(dl), ld_dl=1, rw_=ptr(rw), ld_rw=nw * nr, rg_=ptr(rg), ld_rg=ng * nr, o=outs,
             dev=False, h=s._h):
        a = (h, B_, nr_, x, ld_x, p_, ld_p, lam, ld_lam, 1.0, sx_, ld_sx, ss_, ld_ss, dl_, ld_dl, rw_, ld_rw, rg_,
             ld_rg, *o, info.ctypes.data_as(C.POINTER(C.c_int32)))
        # on the device entry point the checks return before anything reads a pointer
        return L.nmpc_kkt_solve_batch_dev(*a, None) if dev else L.nmpc_kkt_solve_batch(*a)

    # the full message of every rule, on both entry points; the last four break two rules at
    # once: the earlier one in the order of the checks answers
    for dev in (False, True):
        for what, kw, msg in (
                ("null handle", dict(h=None), "null handle"), ("B = 0", dict(B_=0), "B <= 0"),
                ("nr = 0", dict(nr_=0), "nr <= 0"), ("p NULL", dict(p_=None), "required pointer is null (x, p)"),
                ("both right-hand sides NULL", dict(rw_=None, rg_=None), "both right-hand sides are null (r_w, r_g)"),
                ("no output", dict(o=[None] * 3), "every output pointer is null (dw, dX, jdw)"),
                ("ld_r_g short", dict(ld_rg=ng * nr - 1), "leading dimension smaller than the vector length"),
                ("ld_delta negative", dict(ld_dl=-1), "leading dimension smaller than the vector length"),
                ("B = 0 and nr = 0", dict(B_=0, nr_=0), "B <= 0"),
                ("nr = 0 and x NULL", dict(nr_=0, x=None), "nr <= 0"),
                ("no right-hand side and no output", dict(rw_=None, rg_=None, o=[None] * 3),
                 "both right-hand sides are null (r_w, r_g)"),
                ("no output and ld_x short", dict(o=[None] * 3, ld_x=nw - 1),
                 "every output pointer is null (dw, dX, jdw)")):
            assert call(dev=dev, **kw) == -1, (what, dev)
            assert L.nmpc_last_error().decode() == msg, (what, dev)

    for what, rc in (("B = 0", call(B_=0)), ("B < 0", call(B_=-3)), ("nr = 0", call(nr_=0)), ("nr < 0", call(nr_=-1)),
                     ("x NULL", call(x=None)), ("p NULL", call(p_=None)), ("both right-hand sides NULL", call(rw_=None, rg_=None)),
                     ("no output", call(o=[None] * 3)),
                     ("ld_x short", call(ld_x=nw - 1)), ("ld_p short", call(ld_p=spec.np - 1)),
                     ("ld_lam_g short", call(ld_lam=ng - 1)), ("ld_sigma_x short", call(ld_sx=nw - 1)),
                     ("ld_sigma_s short", call(ld_ss=ng - 1)), ("ld_delta negative", call(ld_dl=-1)),
                     ("ld_r_w short", call(ld_rw=nw * nr - 1)), ("ld_r_w one column", call(ld_rw=nw)),
                     ("ld_r_g short", call(ld_rg=ng * nr - 1)), ("ld_x negative", call(ld_x=-nw))):
        assert rc == -1, (what, rc)  # NMPC_E_INVALID
        assert L.nmpc_last_error(), what
    call(rw_=None, rg_=None)
    assert "right-hand" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(nr_=0))
    assert all(np.all(out[k] == 7.0) for k in KEYS) and np.all(info == 9)  # nothing ran
    # the same checks on the device entry point (null device pointers are never dereferenced)
    vp = C.c_void_p
    z = vp(0)
    for h in (s._h, None):
        assert L.nmpc_kkt_solve_batch_dev(h, 2, 2, z, 0, z, 0, z, 0, 1.0, z, 0, z, 0, z, 0, z, 0, z, 0, z, z, z, z,
                                          z) == -1
    # and the handle still works: leading dimension 0 shares everything
    assert call(ld_x=0, ld_p=0, ld_lam=0, ld_sx=0, ld_ss=0, ld_dl=0, ld_rw=0, ld_rg=0) == 0
    assert np.all(info == 0) and all(np.all(np.isfinite(out[k])) for k in KEYS)
    for k in KEYS:
        np.testing.assert_array_equal(out[k][0], out[k][1])
    # a missing right-hand side or output is fine
    assert call(rg_=None, o=[outs[0], None, None]) == 0 and call(rw_=None, o=[None, None, outs[2]]) == 0


def test_sensitivity_of_a_solution():
    """race_track_2, N = 6, the smoke-sized batch.  Solver.sensitivity against the same formula
    evaluated densely on the oracle (the same difference step) under the residual gate, and to
    1e-6 forward where cond(M) <= 1e8.  Then end to end: the quotient (x+ - x-) / 2 eps of
    solves at p +- eps e_j over the initial-state entries; a scenario is skipped only if a
    status or an active set (|lam| > 1e-6) differs between two such solves, at most half of
    them; the GPU's distance to the quotient is within 10x the dense formula's own (both
    differ from the quotient by the solves' 1e-8 tolerance over eps, not by the linear algebra).

    Measured on an MI355X (seed 7, fd_step 1e-3, eps 1e-3): see DESIGN.md 14."""
    from nmpc_amd import draw_scenarios
    from nmpc_amd.nlpsol import Solver

    spec = er.case_spec("race_track_2")
    prob = er.problem_of(spec)
    s = _solver(spec)
    B, nd, eps = 4, 8, 1e-3
    step = 1e-3
    import inspect
    assert inspect.signature(Solver.sensitivity).parameters["fd_step"].default == step
    P = draw_scenarios(spec, B, seed=7)
    lbx, ubx, lbg, ubg = spec.bounds()
    x0 = np.zeros(spec.nw)

    def solve(Pm):
        sol = s(x0=x0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=Pm.T)
        return sol, s.stats()["status_code"].copy()

    sol, st = solve(P)
    assert np.all(np.isin(st, (0, 1))), st
    dp = np.eye(spec.np)[:, :nd]
    got = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp)
    assert got["dx"].shape == (spec.nw, nd, B) and got["dlam_g"].shape == (spec.ng, nd, B)
    print(f"sensitivity: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    dense = []
    for b in range(B):
        dn = kr.dense_sensitivity(prob, sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b], P[b], dp.T, lbx, ubx,
                                  lbg, ubg, step, got["delta"][b])
        dense.append(dn)
        dx = got["dx"][:, :, b].T
        fr = dn["free"]
        assert np.all(dx[:, ~fr] == 0.0)
        r = max(kr.rho(dn["M"], dx[j, fr], dn["rhs"][j]) for j in range(nd))
        f = float(np.max(np.abs(dx - dn["dx"])) / np.max(np.abs(dn["dx"])))
        fl = float(np.max(np.abs(got["dlam_g"][:, :, b].T - dn["dlam_g"])) / max(np.max(np.abs(dn["dlam_g"])), 1e-300))
        print(f"sensitivity scenario {b}: rho {r:.2e} (bound {kr.TOL:.0e}), forward dx {f:.2e}, dlam_g {fl:.2e}, "
              f"cond {dn['cond']:.1e}, active rows {int(np.sum(np.abs(sol['lam_g'][:, b]) > 1e-6))}, "
              f"active bounds {int(np.sum(np.abs(sol['lam_x'][:, b]) > 1e-6))}")
        assert r <= kr.TOL, (b, r)
        if dn["cond"] <= 1e8:
            assert f <= kr.FWD_TOL, (b, f)
    # end to end
    quot = np.zeros((B, nd, spec.nw))
    keep = np.ones(B, bool)
    for j in range(nd):
        e = np.zeros(spec.np)
        e[j] = eps
        (sp, stp), (sm_, stm) = solve(P + e), solve(P - e)
        quot[:, j, :] = ((sp["x"] - sm_["x"]) / (2 * eps)).T
        for b in range(B):
            same = stp[b] == stm[b] == st[b]
            for k in ("lam_g", "lam_x"):
                same = same and np.array_equal(np.abs(sp[k][:, b]) > 1e-6, np.abs(sm_[k][:, b]) > 1e-6)
            keep[b] &= bool(same)
    print(f"end to end: scenarios kept {keep}")
    assert np.sum(~keep) <= B // 2
    for b in np.flatnonzero(keep):
        scale = float(np.max(np.abs(quot[b])))
        dg = float(np.max(np.abs(got["dx"][:, :, b].T - quot[b]))) / scale
        dd = float(np.max(np.abs(dense[b]["dx"] - quot[b]))) / scale
        print(f"end to end scenario {b}: GPU to quotient {dg:.2e}, dense formula to quotient {dd:.2e} (of max |quotient| "
              f"{scale:.2e})")
        assert dg <= 10.0 * dd, (b, dg, dd)
    # the feedback gain of the NMPC law: d u0* / d x0
    gain = got["dx"][:6, :, :]
    print(f"feedback gain d u0 / d x0, scenario 0:\n{np.array2string(gain[:, :, 0], precision=3)}")
