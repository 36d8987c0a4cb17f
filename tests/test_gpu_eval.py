"""nmpc_eval_batch / nmpc_eval_batch_dev (Solver.evaluate, evaluate_device, certify): the NLP's
function layer and the KKT certificate at given points, on the GPU, against the oracle's
SSEval and the certificate of tests/test_gpu_reference_runs.py restated in tests/eval_ref.py
(tolerances: its docstring)."""
import ctypes as C

import numpy as np
import pytest

from tests import eval_ref as er

pytestmark = pytest.mark.gpu

KEYS = ("f", "g", "X", "grad_f", "grad_l", "kkt")


def _solver(spec):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)


def _evaluate(s, d, sel=slice(None), **kw):
    a = dict(lam_g=d["lam_g"][sel].T, lam_x=d["lam_x"][sel].T, lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"])
    a.update(kw)
    return s.evaluate(d["w"][sel].T, d["p"][sel].T, **a)


def _col(res, b):
    return {k: (res[k][:, b] if k != "f" else res[k][0, b]) for k in res}


@pytest.mark.parametrize("name", list(er.CASES))
def test_function_layer_matches_the_oracle(name):
    """f, g, X, grad_f, grad_l and the five certificate numbers of every case
    (both models, N = 1 / 63, 16 obstacles, obstacle coordinates and cost weights from p)
    within 1e-10 of the oracle's, in the forms of tests/eval_ref.py."""
    spec, d, ref = er.reference(name)
    res = _evaluate(_solver(spec), d)
    B = er.CASES[name]
    assert res["f"].shape == (1, B) and res["g"].shape == (spec.ng, B) and res["X"].shape == (spec.nX, B)
    assert res["grad_f"].shape == res["grad_l"].shape == (spec.nw, B) and res["kkt"].shape == (5, B)
    for b in range(B):
        er.check_against(_col(res, b), ref[b], b, name)
    if name == "n1":  # stage 0 is constant in w: no term of grad_f exists
        assert np.all(res["grad_f"] == 0.0)


def test_batch_plumbing():
    """B = 1 and B = 65; a scenario's results do not depend on its place or its neighbours;
    leading dimension 0 broadcasts; absent multipliers give grad_l == grad_f; absent outputs
    leave the others unchanged; host and device entry points agree.  All bitwise."""
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B = 65
    d = er.draw_point(spec, B, seed=77)
    full = _evaluate(s, d)
    assert all(np.all(np.isfinite(full[k])) for k in KEYS)
    for b in (0, 37, 64):  # alone (B = 1), first / middle / last (the 65th: a second block of 64)
        one = _evaluate(s, d, slice(b, b + 1))
        for k in KEYS:
            np.testing.assert_array_equal(one[k][:, 0], full[k][:, b], err_msg=f"{k} scenario {b}")
    rev = _evaluate(s, d, slice(None, None, -1))
    for k in KEYS:
        np.testing.assert_array_equal(rev[k][:, ::-1], full[k], err_msg=k)
    # one shared p (and the bounds, shared throughout) against the same p repeated
    dp = dict(d, p=np.repeat(d["p"][:1], B, axis=0))
    tiled = _evaluate(s, dp)
    shared = s.evaluate(d["w"].T, d["p"][0], lam_g=d["lam_g"].T, lam_x=d["lam_x"].T, lbx=d["lbx"], ubx=d["ubx"],
                        lbg=np.repeat(d["lbg"][:, None], B, axis=1), ubg=d["ubg"])
    for k in KEYS:
        np.testing.assert_array_equal(shared[k], tiled[k], err_msg=k)
    # no multipliers
    nol = s.evaluate(d["w"].T, d["p"].T)
    assert "kkt" not in nol
    np.testing.assert_array_equal(nol["grad_l"], nol["grad_f"])
    for k in ("f", "g", "X", "grad_f"):
        np.testing.assert_array_equal(nol[k], full[k], err_msg=k)
    # device entry point: everything, then subsets of the outputs
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "lam_x", "lbx", "ubx",
                                                                       "lbg", "ubg")}
    shapes = {"f": (B,), "g": (B, spec.ng), "X": (B, spec.nX), "grad_f": (B, spec.nw), "grad_l": (B, spec.nw),
              "kkt": (B, 5)}

    def run(keys):
        out = {k: torch.full(shapes[k], float("nan"), **f64) for k in keys}
        s.evaluate_device(dev["w"], dev["p"], out, lam_g=dev["lam_g"], lam_x=dev["lam_x"], lbx=dev["lbx"],
                          ubx=dev["ubx"], lbg=dev["lbg"], ubg=dev["ubg"])
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}

    for keys in (KEYS, ("g", "grad_l"), ("kkt",), ("f",), ("X", "grad_f")):
        got = run(keys)
        for k in keys:
            want = full[k].T if k != "f" else full[k][0]
            np.testing.assert_array_equal(got[k], want, err_msg=f"{k} of {keys}")


def test_argument_validation_on_a_live_handle():
    from nmpc_amd import _lib

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    L = _lib.lib()
    d = er.draw_point(spec, 2, seed=5)
    dp = C.POINTER(C.c_double)
    w, p = np.ascontiguousarray(d["w"]), np.ascontiguousarray(d["p"])
    f, kkt = np.full(2, 7.0), np.full((2, 5), 7.0)
    ptr = lambda a: a.ctypes.data_as(dp)  # noqa: E731
    bnd = [ptr(d[k]) for k in ("lbx", "ubx", "lbg", "ubg")]

    def call(B, bounds, outs, dev=False, x=ptr(w), ld_x=spec.nw, h=s._h):
        ins = [x, ld_x, ptr(p), spec.np, None, 0, None, 0]
        for q in bounds:
            ins += [q, 0]
        if dev:  # the checks return before anything reads a pointer
            return L.nmpc_eval_batch_dev(h, B, *ins, *outs, None)
        return L.nmpc_eval_batch(h, B, *ins, *outs)

    none6 = [None] * 6
    # the full message of every rule, on both entry points; the last four break two rules at
    # once: the earlier one in the order of the checks answers
    f1, k1 = [ptr(f)] + none6[1:], none6[:5] + [ptr(kkt)]
    for dev in (False, True):
        for what, kw, msg in (
                ("null handle", dict(B=2, bounds=bnd, outs=f1, h=None), "null handle"),
                ("B = 0", dict(B=0, bounds=bnd, outs=f1), "B <= 0"),
                ("x NULL", dict(B=2, bounds=bnd, outs=f1, x=None), "required pointer is null (x, p)"),
                ("no output", dict(B=2, bounds=bnd, outs=none6), "every output pointer is null"),
                ("kkt without ubg", dict(B=2, bounds=bnd[:3] + [None], outs=k1),
                 "kkt_out needs lbx, ubx, lbg and ubg"),
                ("ld_x short", dict(B=2, bounds=bnd, outs=f1, ld_x=spec.nw - 1),
                 "leading dimension smaller than the vector length"),
                ("null handle and B = 0", dict(B=0, bounds=bnd, outs=f1, h=None), "null handle"),
                ("B = 0 and x NULL", dict(B=0, bounds=bnd, outs=f1, x=None), "B <= 0"),
                ("x NULL and no output", dict(B=2, bounds=bnd, outs=none6, x=None),
                 "required pointer is null (x, p)"),
                ("kkt without ubg and ld_x short", dict(B=2, bounds=bnd[:3] + [None], outs=k1, ld_x=spec.nw - 1),
                 "kkt_out needs lbx, ubx, lbg and ubg")):
            assert call(dev=dev, **kw) == -1, (what, dev)
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    for what, rc in (("B = 0", call(0, bnd, [ptr(f)] + none6[1:])), ("B < 0", call(-3, bnd, [ptr(f)] + none6[1:])),
                     ("no output", call(2, bnd, none6)),
                     ("kkt without ubg", call(2, bnd[:3] + [None], none6[:5] + [ptr(kkt)])),
                     ("kkt without lbx", call(2, [None] + bnd[1:], none6[:5] + [ptr(kkt)]))):
        assert rc == -1, (what, rc)  # NMPC_E_INVALID
        assert L.nmpc_last_error(), what
    msgs = []
    for outs in (none6, none6[:5] + [ptr(kkt)]):
        call(2, bnd[:3] + [None], outs)
        msgs.append(L.nmpc_last_error().decode())
    assert "output" in msgs[0] and "kkt_out" in msgs[1], msgs
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(0, bnd, [ptr(f)] + none6[1:]))
    assert np.all(f == 7.0) and np.all(kkt == 7.0)  # nothing ran
    # the same checks on the device entry point (null device pointers are never dereferenced)
    vp = C.c_void_p
    assert L.nmpc_eval_batch_dev(s._h, 2, *([vp(0), 0] * 8), *([vp(0)] * 6), vp(0)) == -1
    # and the handle still evaluates
    assert call(2, bnd, [ptr(f)] + none6[1:]) == 0 and np.all(np.isfinite(f)) and np.all(f != 7.0)


@pytest.fixture(scope="module")
def solved():
    """The smoke() case: race_track_2, N = 8, T = 0.2, 4 scenarios from u = 0."""
    from nmpc_amd import make_spec, draw_scenarios

    spec = make_spec("race_track_2", N=8, T=0.2)
    P = draw_scenarios(spec, 4, seed=7)
    bnd = spec.bounds()
    s = _solver(spec)
    sol = s(x0=np.zeros(spec.nw), lbx=bnd[0], ubx=bnd[1], lbg=bnd[2], ubg=bnd[3], p=P.T)
    return spec, s, P, bnd, sol, s.stats()["status_code"].copy()


def _cpu_certificate(spec, P, bnd, x, lg, lx, opts_tol=(1.0, 1e-4, 1e-4)):
    """tests/test_gpu_reference_runs.py:355-378 on the oracle, per scenario: (kkt (5,B), ok (B,))."""
    prob = er.problem_of(spec)
    K, OK = [], []
    for b in range(P.shape[0]):
        r = er.cpu_eval(prob, x[:, b], P[b], lg[:, b], lx[:, b], *bnd)
        stat, gmax, viol, cpl, lmax = r["kkt"]
        K.append(r)
        OK.append(stat <= opts_tol[0] and stat <= 1e-4 * (1 + gmax) and viol <= opts_tol[1]
                  and cpl <= opts_tol[2] * (1 + lmax))
    return K, np.array(OK)


def test_agreement_with_the_solver(solved):
    """evaluate at a solve's x reproduces the solve's own f, g, X; certify reports ok for every
    Solve_Succeeded scenario, with the CPU certificate's numbers."""
    spec, s, P, bnd, sol, st = solved
    assert np.any(st == 0), st
    ev = s.evaluate(sol["x"], P.T)
    for k in ("f", "g", "X"):
        err = float(np.max(np.abs(ev[k] - sol[k]) / (1 + np.abs(sol[k]))))
        print(f"{k}: evaluate vs solve, relative {err:.2e}")
        assert err <= 1e-12, (k, err)
    cert = s.certify(sol, *bnd, P.T)
    ref, ok_cpu = _cpu_certificate(spec, P, bnd, sol["x"], sol["lam_g"], sol["lam_x"])
    print("status", st, "ok", cert["ok"], "cpu ok", ok_cpu, "stat", cert["stat"], "viol", cert["viol"], "compl",
          cert["compl"])
    assert np.all(cert["ok"][st == 0]) and np.all(ok_cpu[st == 0])
    full = s.evaluate(sol["x"], P.T, lam_g=sol["lam_g"], lam_x=sol["lam_x"], lbx=bnd[0], ubx=bnd[1], lbg=bnd[2],
                      ubg=bnd[3])
    for b in range(P.shape[0]):
        er.check_against(_col(full, b), ref[b], b, "solution")
        np.testing.assert_array_equal(cert["kkt"][:, b], full["kkt"][:, b])
        kk = full["kkt"][:, b]
        assert cert["stat"][b] == kk[0] and cert["viol"][b] == kk[2]
        assert cert["stat_rel"][b] == kk[0] / (1 + kk[1]) and cert["compl"][b] == kk[3] / (1 + kk[4])
        assert bool(cert["ok"][b]) == bool(ok_cpu[b])


def test_the_certificate_has_teeth(solved):
    """Each mutation of a certified solution must turn ok false on every scenario -- on the CPU
    certificate as on the GPU's, so the condition is the checker's:
      * lam_g: 1e-3 (1 + |lam|) added to the multiplier of the last stage's z row;
      * bound: one control moved 1e-3 past its bound;
      * zero:  x replaced by the zero start.
    The multiplier mutation is NOT placed on an active row.  At these four solutions the only
    active rows are theta rows (scenarios 0 and 3; scenarios 1 and 2 have none), whose Jacobian
    rows are T = 0.2 in size: the mutation moves the dual infeasibility to 3.3e-4 .. 4.0e-4,
    below the acceptance threshold 1e-4 (1 + |grad f|_inf) = 4.5e-4 .. 1.1e-3, and the gap of an
    active row is ~1e-9, so neither the CPU certificate nor any correct one can flag it
    (measured on the oracle's own solutions).  The last stage's z row has the largest Jacobian
    row (~T^2 v N): there the same mutation moves the dual infeasibility to 4.1e-3, above the
    threshold in every scenario.  The active-row mutation is still applied below ("active"),
    where the GPU's verdict and numbers must equal the CPU certificate's."""
    spec, s, P, bnd, sol, st = solved
    ubx = bnd[1]
    base = s.certify(sol, *bnd, P.T)
    keep = np.flatnonzero(base["ok"])
    assert keep.size > 0
    B = P.shape[0]

    def mutated(which):
        m = {k: sol[k].copy() for k in ("x", "lam_g", "lam_x")}
        for b in range(B):
            if which == "active":  # the row with the largest multiplier (stage 0's rows do not depend on w)
                lg = np.abs(m["lam_g"][:, b]).copy()
                lg[:spec.m] = -1.0
                r = int(np.argmax(lg))
                m["lam_g"][r, b] += 1e-3 * (1 + abs(m["lam_g"][r, b]))
            elif which == "lam_g":
                r = spec.N * spec.m
                m["lam_g"][r, b] += 1e-3 * (1 + abs(m["lam_g"][r, b]))
            elif which == "bound":
                m["x"][1, b] = ubx[1] + 1e-3
            else:
                m["x"][:, b] = 0.0
        return m

    for which in ("active", "lam_g", "bound", "zero"):
        m = mutated(which)
        cert = s.certify(m, *bnd, P.T)
        ref, ok_cpu = _cpu_certificate(spec, P, bnd, m["x"], m["lam_g"], m["lam_x"])
        print(which, "ok", cert["ok"], "cpu ok", ok_cpu, "stat", cert["stat"], "stat_rel", cert["stat_rel"], "viol",
              cert["viol"], "compl", cert["compl"])
        np.testing.assert_array_equal(cert["ok"], ok_cpu, err_msg=which)
        full = s.evaluate(m["x"], P.T, lam_g=m["lam_g"], lam_x=m["lam_x"], lbx=bnd[0], ubx=bnd[1], lbg=bnd[2],
                          ubg=bnd[3])
        for b in range(B):
            er.check_against(_col(full, b), ref[b], b, which)
        if which != "active":
            assert not np.any(ok_cpu[keep]), which
            assert not np.any(cert["ok"][keep]), which


def test_evaluate_device_does_not_synchronise():
    """nmpc_eval_batch_dev only enqueues (the pattern of
    test_dev_entry_points_do_not_synchronise): behind a spinning kernel on a side stream the
    call returns while the stream is still busy, and the results equal an unobstructed run's."""
    import time
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B = 64
    d = er.draw_point(spec, B, seed=9)
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g", "lam_x", "lbx", "ubx",
                                                                       "lbg", "ubg")}
    st = torch.cuda.Stream()

    def outs():
        return {"f": torch.empty(B, **f64), "g": torch.empty(B, spec.ng, **f64), "X": torch.empty(B, spec.nX, **f64),
                "grad_f": torch.empty(B, spec.nw, **f64), "grad_l": torch.empty(B, spec.nw, **f64),
                "kkt": torch.empty(B, 5, **f64)}

    def go(o):
        s.evaluate_device(dev["w"], dev["p"], o, lam_g=dev["lam_g"], lam_x=dev["lam_x"], lbx=dev["lbx"], ubx=dev["ubx"],
                          lbg=dev["lbg"], ubg=dev["ubg"], stream=st)

    ref = outs()
    go(ref)  # sizes the workspace (an allocation may synchronise; a sized handle only enqueues)
    torch.cuda.synchronize()
    ws = s.memory_info()["ws_bytes"]
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
    print(f"evaluate_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info()["ws_bytes"] == ws  # nothing allocated by the second call
    for k in o:
        np.testing.assert_array_equal(o[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=k)
