"""nmpc_solve_policy_batch / nmpc_solve_policy_batch_dev (Solver.policy_fused, policy_device,
nmpc_amd.policy.apply): the feedback policy along a solution's plan as one launch -- stage gains
K_k, feedforward kff_k per parameter direction, the stage matrices A_k, B_k and X* -- against the
checker of tests/policy_ref.py (gate (a), the policy identity against the dense matrix; gate (c),
K_0), against the fused forward-mode launch (gate (b)) and the oracle's A, B and X."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import eval_ref as er
from tests import policy_ref as pf
from tests.test_gpu_solve_adjoint import _bnd, _solved, _solver, _ulps  # the solved cases are shared
from tests.test_gpu_solve_tangent import _dirs, _prep

pytestmark = pytest.mark.gpu

OUT = ("K", "kff", "A", "B", "X")
MAIN = ("K", "kff", "A", "B")
ALL = OUT + ("info", "delta")


def _dims(spec):
    N = spec.N
    return N, spec.nw // N, spec.nX // (N + 1)


def _unit_dirs(spec, B, seed):
    """(np, np + 2, B): dp = I and two N(0, 1) directions."""
    return np.ascontiguousarray(np.transpose(pf.directions(spec, B, seed), (2, 1, 0)))


def _host(s, sol, bounds, P, dp, g=True):
    so = sol if g else {k: v for k, v in sol.items() if k != "g"}
    return s.policy_fused(so, *bounds, P.T, dp)


def _device(s, spec, sol, bounds, P, dp, B, g=True, rep=True, out=None):
    """Solver.policy_device on host data (tests/test_gpu_solve_tangent._prep), results as NumPy."""
    import torch

    nd = 0 if dp is None else dp.shape[1]
    dsol, db, dP, dd, _ = _prep(spec, sol, bounds, P, dp if nd else np.zeros((spec.np, 1, B)), B, max(nd, 1), keys=(),
                                g=g, rep=rep)
    pol = s.policy_device(dsol, *db, dP, dd if nd else None, out=out)
    torch.cuda.synchronize()
    return {k: (None if pol[k] is None else pol[k].cpu().numpy()) for k in ALL}


def _same(a, b, what, keys=ALL):
    """Bitwise equality of two results (NaN equal to NaN)."""
    for k in keys:
        if a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, (what, k)
            continue
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _dpb(dp, b):
    return dp[:, :, b].T if dp.ndim == 3 else dp.T


def _gates(name, s, spec, got, sol, bounds, P, dp, B, g=None, tangent=None):
    """Gate (a) for every scenario with info 0 against the checker at the returned delta, A and B
    against the oracle's, and, with `tangent` (sensitivity_fused's result on the same inputs),
    gate (b).  Every figure is printed before it is asserted.  Returns the checker's results."""
    prob = er.problem_of(spec)
    N, nu, nx = _dims(spec)
    refs = []
    for b in range(B):
        if got["info"][b] != 0:
            refs.append(None)
            continue
        d = _dpb(dp, b)
        ref = pf.dense_policy(prob, sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b], P[b],
                              [_bnd(v, b) for v in bounds], d, delta=got["delta"][b], g=None if g is None else g[:, b])
        one = {k: got[k][b] for k in MAIN}
        fixed = ~ref["tan"]["free"].reshape(N, nu)
        assert np.all(one["K"][fixed] == 0.0) and np.all(one["kff"][:, fixed] == 0.0), (name, b)
        fa = pf.gate_a(one, ref, d)
        fAB = max(float(np.max(np.abs(one[k] - ref[k]) / (pf.TOL_B * (1.0 + np.abs(ref[k]))))) for k in ("A", "B"))
        msg = (f"{name} scenario {b}: delta {got['delta'][b]:.3g}, gate (a) {fa:.2e} (bound {pf.TOL_A:.0e}), "
               f"A, B error / bound {fAB:.2e}")
        fb = 0.0
        if tangent is not None:
            dx = tangent["dx"][:, :, b].T.reshape(-1, N, nu)
            dX = tangent["dX"][:, :, b].T.reshape(-1, N + 1, nx)
            a = pf.scale_a(one["K"], ref["k"], ref["xi"], dX)
            err = np.abs(dx - (np.einsum("kij,dkj->dki", one["K"], dX[:, :N]) + one["kff"]))
            assert np.all(err[a == 0] == 0.0), (name, b)
            fb = float(np.max(err[a > 0] / (pf.TOL_B * a[a > 0]), initial=0.0))
            msg += f", gate (b) error / bound {fb:.2e}"
        print(msg)
        assert fa <= pf.TOL_A, (name, b, fa)
        assert fAB <= 1.0, (name, b, fAB)
        assert fb <= 1.0, (name, b, fb)
        refs.append(ref)
    return refs


@pytest.mark.parametrize("name", list(pf.SOLVED))
def test_policy_matches_the_checker_the_tangent_launch_and_the_oracle(name):
    """Solved cases, dp = I and two N(0, 1) directions.
    (a) the policy identity against the dense M at the returned delta (tests/policy_ref.gate_a), with
        the GPU's own A and B;
    (b) |dx_k - (K_k dX_k + kff_k)| <= adjoint_ref.TOL a_k per entry with dx, dX of
        sensitivity_fused, and K_0 + kff_0 over the x0 unit directions against feedback_gain_device
        within the same scale;
    A, B within TOL (1 + |entry|) of SSEval's; X within TOL of evaluate's (ulps printed)."""
    import torch

    spec, s, B, P, bounds, sol = _solved(name)
    N, nu, nx = _dims(spec)
    dp = _unit_dirs(spec, B, 95)
    nd = dp.shape[1]
    got = _host(s, sol, bounds, P, dp)
    assert got["K"].shape == (B, N, nu, nx) and got["kff"].shape == (B, nd, N, nu)
    assert got["A"].shape == (B, N, nx, nx) and got["B"].shape == (B, N, nx, nu) and got["X"].shape == (B, N + 1, nx)
    print(f"{name}: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    tan = s.sensitivity_fused(sol, *bounds, P.T, dp)
    np.testing.assert_array_equal(tan["delta"], got["delta"])
    refs = _gates(name, s, spec, got, sol, bounds, P, dp, B, g=sol["g"], tangent=tan)
    # X
    X = s.evaluate(sol["x"], P.T)["X"].T.reshape(B, N + 1, nx)
    print(f"{name}: X against evaluate's, largest difference {_ulps(got['X'], X):.1f} ulps")
    assert np.all(np.abs(got["X"] - X) <= pf.TOL_B * (1.0 + np.abs(X)))
    # the law's gain
    dsol, db, dP, _, _ = _prep(spec, sol, bounds, P, np.zeros((spec.np, 1)), B, 1, keys=(), rep=False)
    Kfb, info = s.feedback_gain_device(dsol, *db, dP)
    torch.cuda.synchronize()
    Kfb = Kfb.cpu().numpy()
    for b in range(B):
        mine = got["K"][b, 0] + got["kff"][b, :nx, 0].T  # (nu, nx): column j is direction e_j
        a0 = np.abs(got["K"][b, 0]) @ (2.0 * np.eye(nx)) + np.abs(refs[b]["k"][:nx, 0].T)
        err = np.abs(mine - Kfb[b])
        assert np.all(err[a0 == 0] == 0.0), (name, b)
        fig = float(np.max(err[a0 > 0] / (pf.TOL_B * a0[a0 > 0]), initial=0.0))
        print(f"{name} scenario {b}: K_0 + kff_0 against feedback_gain_device, error / bound {fig:.2e}")
        assert fig <= 1.0, (name, b, fig)


def test_gate_c_the_stage_0_gain():
    """On handles with first_hessian_perturbation = 1e-12, the x0 unit directions: wherever the
    returned delta <= 1e-10, max |kff_0| <= 10 delta (tests/policy_ref.py: the checker measures
    0.26 delta, the stored K_0 of the other kernels 1.2e-8 to 8.9e-7).  At most 3 of the 13
    scenarios may lie outside delta <= 1e-10."""
    outside = total = 0
    for name in pf.SOLVED:
        spec, s0, B, P, bounds, sol = _solved(name)
        N, nu, nx = _dims(spec)
        s = _solver(spec, first_hessian_perturbation=1e-12)
        got = _host(s, sol, bounds, P, np.eye(spec.np)[:, :nx])
        assert np.all(got["info"] == 0), (name, got["info"])
        for b in range(B):
            total += 1
            fc, dl = pf.gate_c(got["kff"][b], nx), got["delta"][b]
            print(f"{name} scenario {b}: delta {dl:.3g}, max|kff_0| {fc:.2e} ({fc / dl:.2f} delta; "
                  f"bound {pf.C_FACTOR:.0f} delta)")
            if not dl <= pf.C_DELTA:
                outside += 1
                continue
            assert fc <= pf.C_FACTOR * dl, (name, b, fc, dl)
    print(f"gate (c): {total - outside} of {total} scenarios at delta <= {pf.C_DELTA:.0e}")
    assert total == 13 and outside <= 3, (total, outside)


@pytest.mark.parametrize("name", ["n1", "n63_16obs"])
def test_synthetic_points_on_the_smallest_and_largest_shape(name):
    """Random x inside the bounds and random signed multipliers (tests/eval_ref.draw_point), N = 1
    and N = 63 with 16 obstacles (every lane, every row slot), two N(0, 1) directions and the x0
    unit directions, g NULL: gates (a) and (b) with the ladder climbing on n63_16obs."""
    spec = er.case_spec(name)
    s = _solver(spec)
    B = er.CASES[name]
    N, nu, nx = _dims(spec)
    d = er.draw_point(spec, B, seed=31)
    bounds = (d["lbx"], d["ubx"], d["lbg"], d["ubg"])
    P = d["p"]
    sol = {"x": d["w"].T, "lam_g": d["lam_g"].T, "lam_x": d["lam_x"].T}
    dp = np.concatenate([_dirs(spec, B, 2, 83), np.repeat(np.eye(spec.np)[:, :nx, None], B, axis=2)], axis=1)
    got = _host(s, sol, bounds, P, dp, g=False)
    print(f"{name}: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0), got["info"]
    if name == "n63_16obs":
        assert np.max(got["delta"]) > 1e-4  # the ladder climbed
    tan = s.sensitivity_fused(sol, *bounds, P.T, dp)
    np.testing.assert_array_equal(tan["delta"], got["delta"])
    _gates(name, s, spec, got, sol, bounds, P, dp, B, tangent=tan)


def test_fixed_controls_and_invalid_scenarios():
    """A third of the controls fixed through lbx == ubx, a whole stage among them: those rows of
    every K_k and entries of kff are exactly 0.0 and the gates hold on the rest.  An equality row,
    lbx > ubx and a NaN multiplier give info -11, delta 0 and NaN beside a bitwise-untouched
    neighbour; max_hessian_perturbation = 1e-6 gives info 1 and NaN where the default ladder
    climbs past it.  The host wrapper raises on equality rows."""
    spec, s, B, P, bounds, sol = _solved("race_track_2")
    lbx, ubx, lbg, ubg = bounds
    N, nu, nx = _dims(spec)
    dp = _dirs(spec, B, 2, 84)
    rng = np.random.default_rng(78)
    fx = rng.uniform(size=(spec.nw, B)) < 1.0 / 3.0
    fx[:nu, 0] = True  # a whole stage
    lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb2[fx], ub2[fx] = sol["x"][fx], sol["x"][fx]
    b2 = (lb2, ub2, lbg, ubg)
    got = _host(s, sol, b2, P, dp)
    print(f"fixed controls: {fx.sum(axis=0)} of {spec.nw}, info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    for b in range(B):
        f = fx[:, b].reshape(N, nu)
        assert np.all(got["K"][b][f] == 0.0) and not np.any(np.signbit(got["K"][b][f])), b
        assert np.all(got["kff"][b][:, f] == 0.0), b
    tan = s.sensitivity_fused(sol, *b2, P.T, dp)
    refs = _gates("fixed controls", s, spec, got, sol, b2, P, dp, B, g=sol["g"], tangent=tan)
    assert all(np.array_equal(r["tan"]["free"], ~fx[:, b]) for b, r in enumerate(refs))
    # invalid scenarios
    full = _device(s, spec, sol, bounds, P, dp, B)
    lg2, ug2 = (np.repeat(v[:, None], B, axis=1) for v in (lbg, ubg))
    lg2[spec.ng // 2, 0] = ug2[spec.ng // 2, 0]
    lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb3[5, 1] = ub3[5, 1] + 1.0
    sol3 = dict(sol, lam_g=sol["lam_g"].copy())
    sol3["lam_g"][3, 2] = np.nan
    got = _device(s, spec, sol3, (lb3, ub3, lg2, ug2), P, dp, B)
    print(f"invalid scenarios: info {got['info']}, delta {got['delta']}")
    np.testing.assert_array_equal(got["info"], [-11, -11, -11, 0])
    np.testing.assert_array_equal(got["delta"][:3], 0.0)
    for k in OUT:
        assert np.all(np.isnan(got[k][:3])), k
        np.testing.assert_array_equal(got[k][3], full[k][3], err_msg=k)
    assert got["delta"][3] == full["delta"][3]
    with pytest.raises(ValueError):
        s.policy_fused(sol, lbx, ubx, lg2, ug2, P.T, dp)
    # no rung allowed: scenario 0 with its last stage fixed at the solution factorises at delta = 0
    lb4, ub4 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
    lb4[-nu:, 0] = ub4[-nu:, 0] = sol["x"][-nu:, 0]
    b4 = (lb4, ub4, lbg, ubg)
    ref = _host(s, sol, b4, P, dp)
    cut = _solver(spec, max_hessian_perturbation=1e-6)
    got = _host(cut, sol, b4, P, dp)
    print(f"max_hessian_perturbation 1e-6: info {got['info']}, delta {got['delta']}; default ladder: delta {ref['delta']}")
    stuck = ref["delta"] > 1e-6
    assert np.any(stuck) and not np.all(stuck)
    np.testing.assert_array_equal(got["info"], np.where(stuck, 1, 0))
    for k in OUT:
        assert np.all(np.isnan(got[k][stuck])), k
        np.testing.assert_array_equal(got[k][~stuck], ref[k][~stuck], err_msg=k)


def test_uav5_shapes_and_no_write_past_the_model_s_dimensions():
    """The no-gimbal model: blocks of (3, 5), (5, 5), (5, 3), kff (nd, N, 3), X (N + 1, 5); with the
    output buffers carved out of one larger tensor of sentinels, nothing outside them is written."""
    import torch

    spec, s, B, P, bounds, sol = _solved("uav5")
    N, nu, nx = _dims(spec)
    assert (nu, nx) == (3, 5)
    nd = 2
    dp = _dirs(spec, B, nd, 96)
    shapes = {"K": (B, N, nx, nu), "kff": (B, nd, N, nu), "A": (B, N, nx, nx), "B": (B, N, nu, nx), "X": (B, N + 1, nx)}
    pad = 64
    big = torch.full((sum(int(np.prod(v)) + pad for v in shapes.values()) + pad,), 7.0, dtype=torch.float64, device="cuda")
    out, o, spans = {}, pad, []
    for k, shp in shapes.items():
        n = int(np.prod(shp))
        out[k] = big[o:o + n].view(shp)
        spans.append((o, o + n))
        o += n + pad
    got = _device(s, spec, sol, bounds, P, dp, B, out=out)
    assert got["K"].shape == (B, N, 3, 5) and got["A"].shape == (B, N, 5, 5) and got["B"].shape == (B, N, 5, 3)
    assert got["kff"].shape == (B, nd, N, 3) and got["X"].shape == (B, N + 1, 5)
    assert np.all(got["info"] == 0)
    h = big.cpu().numpy()
    keep = np.ones(h.shape, bool)
    for a, b in spans:
        keep[a:b] = False
        assert np.all(np.isfinite(h[a:b])) and not np.any(h[a:b] == 7.0)
    assert np.all(h[keep] == 7.0)
    _same(got, _host(s, sol, bounds, P, dp), "uav5, device against host entry point")


def test_batch_plumbing():
    """All bitwise: nd = 3 equals three nd = 1 calls; nd = 0 gives the same K, A, B, X and no kff;
    leading dimension 0 for the bounds, p and the directions equals the replicated call; the host
    and the device entry point agree, for every subset of the outputs; a NaN in one direction
    poisons that direction's kff only."""
    import torch
    from nmpc_amd import _lib

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    N, nu, nx = _dims(spec)
    nd = 3
    dp = _dirs(spec, B, nd, 87)
    full = _host(s, sol, bounds, P, dp)
    assert np.all(full["info"] == 0)
    _same(_device(s, spec, sol, bounds, P, dp, B), full, "device against host entry point")
    for j in range(nd):
        one = _host(s, sol, bounds, P, dp[:, j:j + 1])
        np.testing.assert_array_equal(one["kff"][:, 0], full["kff"][:, j], err_msg=f"kff direction {j}")
        _same(one, full, f"direction {j}", ("K", "A", "B", "X", "info", "delta"))
    for none in (_host(s, sol, bounds, P, None), _device(s, spec, sol, bounds, P, None, B)):
        assert none["kff"] is None
        _same(none, full, "nd = 0", ("K", "A", "B", "X", "info", "delta"))
    # leading dimension 0: shared bounds, p and directions against replicated ones
    sh = np.ascontiguousarray(dp[:, :, 0])
    P1 = np.repeat(P[:1], B, axis=0)
    sol1 = {k: np.repeat(v[:, :1], B, axis=1) for k, v in sol.items()}
    rep = _device(s, spec, sol1, bounds, P1, np.repeat(sh[:, :, None], B, axis=2), B, rep=True)
    dsol, db, dP, dd, _ = _prep(spec, sol1, bounds, P1, sh, B, nd, keys=(), rep=False)
    pol = s.policy_device(dsol, *db, dP[0].contiguous(), dd)
    torch.cuda.synchronize()
    shared = {k: pol[k].cpu().numpy() for k in ALL}
    _same(shared, rep, "ld = 0")
    _same(shared, _host(s, sol1, bounds, P1, sh), "ld = 0, host entry point")
    for b in range(1, B):
        for k in OUT:
            np.testing.assert_array_equal(shared[k][b], shared[k][0], err_msg=k)
    # every subset of the outputs, host against device entry point, through the C-ABI
    L = _lib.lib()
    names = ("x", "p", "lam_g", "lam_x", "g", "lbx", "ubx", "lbg", "ubg")
    lens = dict(zip(names, (spec.nw, spec.np, spec.ng, spec.nw, spec.ng, spec.nw, spec.nw, spec.ng, spec.ng)))
    harr = {"x": sol["x"].T, "p": P, "lam_g": sol["lam_g"].T, "lam_x": sol["lam_x"].T, "g": sol["g"].T}
    harr.update({k: np.repeat(v[None], B, 0) for k, v in zip(("lbx", "ubx", "lbg", "ubg"), bounds)})
    harr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in harr.items()}
    hdp = np.ascontiguousarray(np.transpose(dp, (2, 1, 0)))
    darr = {k: torch.tensor(v, device="cuda") for k, v in harr.items()}
    ddp = torch.tensor(hdp, device="cuda")
    raw = {"K": (B, N, nx, nu), "kff": (B, nd, N, nu), "A": (B, N, nx, nx), "B": (B, N, nu, nx), "X": (B, N + 1, nx),
           "delta": (B,)}
    want = {k: (np.ascontiguousarray(np.swapaxes(full[k], 2, 3)) if k in ("K", "A", "B") else full[k]) for k in raw}
    dpt, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    for n in range(1, len(OUT) + 1):
        for keys in itertools.combinations(OUT, n):
            if not set(keys) & set(MAIN):
                continue
            keys = keys + (("delta",) if n % 2 else ())
            ho = {k: np.full(raw[k], 7.0) for k in keys}
            do = {k: torch.full(raw[k], 7.0, dtype=torch.float64, device="cuda") for k in keys}
            hi, di = np.full(B, 99, dtype=np.int32), torch.full((B,), 99, dtype=torch.int32, device="cuda")
            ha, da = [s._h, B, nd], [s._h, B, nd]
            for k in names:
                ha += [harr[k].ctypes.data_as(dpt), lens[k]]
                da += [vp(darr[k].data_ptr()), lens[k]]
            ha += [hdp.ctypes.data_as(dpt), nd * spec.np]
            da += [vp(ddp.data_ptr()), nd * spec.np]
            order = OUT + ("info", "delta")
            for k in order:
                if k == "info":
                    ha.append(hi.ctypes.data_as(ip))
                    da.append(vp(di.data_ptr()))
                else:
                    ha.append(ho[k].ctypes.data_as(dpt) if k in ho else None)
                    da.append(vp(do[k].data_ptr()) if k in do else vp(0))
            assert L.nmpc_solve_policy_batch(*ha) == 0, keys
            assert L.nmpc_solve_policy_batch_dev(*da, vp(0)) == 0, keys
            torch.cuda.synchronize()
            for k in keys:
                np.testing.assert_array_equal(ho[k], want[k], err_msg=f"host, outputs {keys}: {k}")
                np.testing.assert_array_equal(do[k].cpu().numpy(), want[k], err_msg=f"device, outputs {keys}: {k}")
            assert np.all(hi == 0) and np.all(di.cpu().numpy() == 0)
    # a NaN entry poisons its own direction only
    bad = dp.copy()
    bad[3, 1, :] = np.nan
    poisoned = _host(s, sol, bounds, P, bad)
    np.testing.assert_array_equal(poisoned["kff"][:, [0, 2]], full["kff"][:, [0, 2]])
    assert np.all(np.any(np.isnan(poisoned["kff"][:, 1].reshape(B, -1)), axis=1))
    _same(poisoned, full, "NaN in a direction", ("K", "A", "B", "X", "info", "delta"))


def test_argument_validation_on_a_live_handle():
    """B <= 0, nd < 0, a NULL required pointer, a NULL dp with nd > 0, a dp or kff_out with nd = 0,
    K, kff, A and B all NULL and a leading dimension that is neither 0 nor >= the vector length
    return NMPC_E_INVALID from both entry points before any device call: nothing is written, and
    the handle still works."""
    from nmpc_amd import _lib

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    N, nu, nx = _dims(spec)
    L = _lib.lib()
    nd = 2
    nw, ng, npp = spec.nw, spec.ng, spec.np
    arr = {"x": sol["x"].T, "p": P, "lam_g": sol["lam_g"].T, "lam_x": sol["lam_x"].T, "g": sol["g"].T,
           "lbx": np.repeat(bounds[0][None], B, 0), "ubx": np.repeat(bounds[1][None], B, 0),
           "lbg": np.repeat(bounds[2][None], B, 0), "ubg": np.repeat(bounds[3][None], B, 0),
           "dp": np.transpose(_dirs(spec, B, nd, 89), (2, 1, 0))}
    arr = {k: np.ascontiguousarray(v, dtype=np.float64) for k, v in arr.items()}
    arr.update(K=np.full((B, N, nx, nu), 7.0), kff=np.full((B, nd, N, nu), 7.0), A=np.full((B, N, nx, nx), 7.0),
               B=np.full((B, N, nu, nx), 7.0), X=np.full((B, N + 1, nx), 7.0), delta=np.full(B, 7.0))
    info = np.full(B, 99, dtype=np.int32)
    names = ("x", "p", "lam_g", "lam_x", "g", "lbx", "ubx", "lbg", "ubg", "dp")
    lens = dict(zip(names, (nw, npp, ng, nw, ng, nw, nw, ng, ng, npp * nd)))
    dpt, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)

    def call(B_=B, nd_=nd, null=(), ld=None, dev=False):
        ld = dict(lens, **(ld or {}))
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k not in null else vp(0)  # noqa: E731
            gi = vp(info.ctypes.data)
        else:
            g = lambda k: arr[k].ctypes.data_as(dpt) if k not in null else None  # noqa: E731
            gi = info.ctypes.data_as(ip)
        args = [s._h, B_, nd_]
        for k in names:
            args += [g(k), ld[k]]
        args += [g(k) for k in OUT] + [gi, g("delta")]
        return L.nmpc_solve_policy_batch_dev(*args, vp(0)) if dev else L.nmpc_solve_policy_batch(*args)

    # each with the full message of its rule; the last four break two rules at once: the earlier
    # one in the order of the checks answers
    req, ldm = "required pointer is null (x, p, lam_g, lam_x, lbx, ubx, lbg, ubg)", "leading dimension smaller than the vector length"
    nd0, outs, nodp = "dp and kff_out must be null with nd = 0", "K_out, kff_out, A_out and B_out are all null", "dp is null with nd > 0"
    for dev in (False, True):
        cases = [("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"), ("nd < 0", dict(nd_=-1), "nd < 0"),
                 ("nd = 0 with dp and kff", dict(nd_=0), nd0), ("nd = 0 with dp", dict(nd_=0, null=("kff",)), nd0),
                 ("nd = 0 with kff", dict(nd_=0, null=("dp",)), nd0), ("K, kff, A, B NULL", dict(null=MAIN), outs),
                 ("ld_x negative", dict(ld={"x": -nw}), ldm), ("ld_dp one direction", dict(ld={"dp": npp}), ldm)]
        cases += [(f"{k} NULL", dict(null=(k,)), nodp if k == "dp" else req) for k in names if k != "g"]
        cases += [(f"ld_{k} short", dict(ld={k: lens[k] - 1}), ldm) for k in names]
        cases += [("B = 0 and nd < 0", dict(B_=0, nd_=-1), "B <= 0"), ("nd < 0 and x NULL", dict(nd_=-1, null=("x",)), "nd < 0"),
                  ("ubg NULL and dp NULL", dict(null=("ubg", "dp")), req),
                  ("dp NULL and no output", dict(null=("dp",) + tuple(MAIN)), nodp),
                  ("no output and ld_p short", dict(null=MAIN, ld={"p": npp - 1}), outs)]
        for what, kw, msg in cases:
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error(), what
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    call(null=MAIN)
    assert "K_out" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(nd_=-1))
    assert all(np.all(arr[k] == 7.0) for k in OUT + ("delta",)) and np.all(info == 99)  # nothing ran
    # and the handle still works: g NULL, K alone; nd = 0; leading dimension 0 shares everything
    assert call(null=("g", "kff", "A", "B", "X", "delta")) == 0
    assert np.all(np.isfinite(arr["K"])) and np.all(info == 0) and all(np.all(arr[k] == 7.0) for k in ("kff", "A", "B", "X"))
    assert call(nd_=0, null=("dp", "kff")) == 0 and np.all(np.isfinite(arr["A"])) and np.all(arr["kff"] == 7.0)
    assert call(ld={k: 0 for k in names}) == 0
    for k in OUT:
        assert np.all(np.isfinite(arr[k]))
        for b in range(1, B):
            np.testing.assert_array_equal(arr[k][0], arr[k][b])


def test_policy_device_reads_nothing_back_and_allocates_nothing(monkeypatch):
    """With torch.Tensor.cpu made to raise policy_device still completes, into preallocated
    buffers; the handle's memory_info is unchanged by the call (a solve's workspace covers it)."""
    import torch

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    nd = 2
    dp = _dirs(spec, B, nd, 88)
    ref = _device(s, spec, sol, bounds, P, dp, B)
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    dsol, db, dP, dd, _ = _prep(spec, sol, bounds, P, dp, B, nd, keys=())
    first = s.policy_device(dsol, *db, dP, dd)
    torch.cuda.synchronize()

    def boom(*a, **k):
        raise AssertionError("a host round trip in policy_device")

    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "cpu", boom)
        pol = s.policy_device(dsol, *db, dP, dd, out=first["raw"])
    torch.cuda.synchronize()
    assert s.memory_info() == mem
    assert all(pol["raw"][k] is first["raw"][k] for k in ALL)
    _same({k: pol[k].cpu().numpy() for k in ALL}, ref, "policy_device into its own buffers")


def test_policy_apply_equals_the_formula_and_clamps():
    """nmpc_amd.policy.apply against u*_k + K_k (x - X*_k) + sum_d kff_k^(d) c_d in NumPy, with and
    without coefficients, clamped to the control bounds when they are given, NaN where info != 0."""
    import torch
    from nmpc_amd import policy

    spec, s, B, P, bounds, sol = _solved("race_track_2")
    N, nu, nx = _dims(spec)
    nd = 2
    dp = _dirs(spec, B, nd, 97)
    f64 = dict(dtype=torch.float64, device="cuda")
    sol3 = dict(sol, lam_x=sol["lam_x"].copy())
    sol3["lam_x"][2, 1] = np.nan  # scenario 1: info -11
    dsol, db, dP, dd, _ = _prep(spec, sol3, bounds, P, dp, B, nd, keys=(), rep=False)
    pol = s.policy_device(dsol, *db, dP, dd)
    torch.cuda.synchronize()
    h = {k: pol[k].cpu().numpy() for k in ALL}
    assert h["info"].tolist() == [0, -11] + [0] * (B - 2)
    rng = np.random.default_rng(98)
    xm = h["X"][:, :, :] + 0.5 * rng.standard_normal((B, N + 1, nx))
    c = rng.standard_normal((B, nd))
    for k in (0, N // 2, N - 1):
        want = sol["x"].T[:, k * nu:(k + 1) * nu] + np.einsum("bij,bj->bi", h["K"][:, k], xm[:, k] - h["X"][:, k])
        got = policy.apply(pol, dsol, k, torch.tensor(xm[:, k], **f64)).cpu().numpy()
        assert np.all(np.isnan(got[1]))
        ok = h["info"] == 0
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-13, atol=1e-13)
        want = want + np.einsum("bdi,bd->bi", h["kff"][:, :, k], c)
        got = policy.apply(pol, dsol, k, torch.tensor(xm[:, k], **f64), c=torch.tensor(c, **f64)).cpu().numpy()
        np.testing.assert_allclose(got[ok], want[ok], rtol=1e-13, atol=1e-13)
        lo, hi = bounds[0][k * nu:(k + 1) * nu], bounds[1][k * nu:(k + 1) * nu]
        got = policy.apply(pol, dsol, k, torch.tensor(xm[:, k], **f64), c=torch.tensor(c, **f64), lbx=db[0], ubx=db[1])
        got = got.cpu().numpy()
        np.testing.assert_allclose(got[ok], np.clip(want[ok], lo, hi), rtol=1e-13, atol=1e-13)
        assert np.all(np.isnan(got[1]))
    big = policy.apply(pol, dsol, 0, torch.tensor(xm[:, 0] + 1e3, **f64), lbx=db[0], ubx=db[1]).cpu().numpy()
    ok = h["info"] == 0
    assert np.all(big[ok] >= bounds[0][:nu]) and np.all(big[ok] <= bounds[1][:nu])
    assert np.any((big[ok] == bounds[0][:nu]) | (big[ok] == bounds[1][:nu]))  # it did clamp
