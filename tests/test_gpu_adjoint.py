"""nmpc_adjoint_products_batch / nmpc_adjoint_products_batch_dev (Solver.adjoint_products,
adjoint_products_device, sensitivity_adjoint, nmpc_amd.autograd.solve): the exact transposed
products J' y + W z + (dX/dw)' Xb and (dg/dp)' y + (d_p grad_w L)' z + (dX/dp)' Xb at given
points, on the GPU, against the transposes of the oracle's dense forms (tests/adjoint_ref.py:
seeds, scales, tolerance), against the GPU's own forward entry points, and the reverse-mode
solution sensitivity built on them."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest

from tests import adjoint_ref as ar
from tests import eval_ref as er
from tests import kkt_ref as kr
from tests import param_ref as qr
from tests import products_ref as pr

pytestmark = pytest.mark.gpu

KEYS = ar.KEYS
SUBSETS = [c for n in (1, 2, 3) for c in itertools.combinations(ar.SEEDS, n)]


def _solver(spec, opts=None):
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    return nlpsol("solver", "ipopt", spec, REFERENCE_OPTS if opts is None else opts)


def _t(a):
    """(B, na, n) -> the Solver methods' (n, na, B)."""
    return np.ascontiguousarray(np.transpose(a, (2, 1, 0)))


def _ap(s, d, sel=slice(None), sigma=1.0, lam=True, seeds=ar.SEEDS, over=None, want=KEYS):
    """Solver.adjoint_products on the seeds named, taken from d (B, na, n) or from `over`."""
    src = dict(d, **(over or {}))
    kw = {("Xbar" if k == "Xb" else k): (_t(src[k][sel]) if src[k].ndim == 3 else src[k]) for k in seeds}
    return s.adjoint_products(d["w"][sel].T, d["p"][sel].T, lam_g=d["lam_g"][sel].T if lam else None,
                              obj_factor=sigma, want=want, **kw)


def _scn(res, b):
    return {k: res[k][:, :, b].T for k in res}


def _equal(a, b, what=""):
    assert set(a) == set(b), (what, set(a), set(b))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what} {k}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_adjoint_products_match_the_checker(name):
    """wbar and pbar of every case (both models, N = 1 / 63, 16 obstacles, obstacle coordinates
    and cost weights from p), na = 3, for (obj_factor, lam_g) = (1, random), (0.37, random),
    (0, random), (1, NULL), each seed alone and all three together: within 1e-10 of the checker's
    relative to the scales of tests/adjoint_ref.py."""
    spec, d, dn = ar.reference(name)
    s = _solver(spec)
    B = er.CASES[name]
    for combo in ar.COMBOS:
        for seeds in (("y",), ("z",), ("Xb",), ar.SEEDS):
            res = _ap(s, d, sigma=combo[0], lam=combo[1], seeds=seeds)
            assert res["wbar"].shape == (spec.nw, ar.NA, B) and res["pbar"].shape == (spec.np, ar.NA, B)
            for b in range(B):
                ref = ar.products_of(dn[combo][b], **{k: d[k][b] for k in seeds})
                ar.check_against(_scn(res, b), ref, f"{name} {combo} seeds {'+'.join(seeds)} scenario {b}")


@pytest.mark.parametrize("name", list(er.CASES))
def test_identities_against_the_forward_entry_points(name):
    """Against the GPU's own products and param_products on their tests' directions:
    <y, jv> + <z, hv> + <Xb, dX> = <wbar, v> and <y, jp> + <z, hp> + <Xb, dXp> = <pbar, dp> within
    TOL times the sum of the absolute terms; wbar with z alone equals products' hv at v = z, and
    pbar with y alone equals param_products' gp at (obj_factor 0, lam_g = y), within the gate."""
    spec, d, dn = ar.reference(name)
    _, dv, _ = pr.reference(name)
    _, dq, _ = qr.reference(name)
    s = _solver(spec)
    B = er.CASES[name]
    x, p, lam = d["w"].T, d["p"].T, d["lam_g"].T
    adj = _ap(s, d, sigma=0.37)
    fv = s.products(x, p, _t(dv["v"]), lam_g=lam, obj_factor=0.37)
    fp = s.param_products(x, p, _t(dq["dp"]), lam_g=lam, obj_factor=0.37)
    worst = 0.0
    for out, fwd, dirs, keys in (("wbar", fv, dv["v"], ("jv", "hv", "dX")), ("pbar", fp, dq["dp"], ("jp", "hp", "dXp"))):
        for b in range(B):
            for a in range(ar.NA):
                for j in range(dirs.shape[1]):
                    terms = [d[sk][b, a] * fwd[fk][:, j, b] for sk, fk in zip(ar.SEEDS, keys)]
                    rt = adj[out][:, a, b] * dirs[b, j]
                    den = sum(float(np.sum(np.abs(t))) for t in terms) + float(np.sum(np.abs(rt)))
                    worst = max(worst, abs(sum(float(np.sum(t)) for t in terms) - float(np.sum(rt))) / (ar.TOL * den))
    print(f"{name}: dot-product identities against the forward entry points, largest defect / bound {worst:.2e}")
    assert worst <= 1.0, (name, worst)
    combo = (0.37, True)
    hv = s.products(x, p, _t(d["z"]), lam_g=lam, obj_factor=0.37)["hv"]
    wz = _ap(s, d, sigma=0.37, seeds=("z",), want=("wbar",))["wbar"]
    py = _ap(s, d, sigma=0.37, seeds=("y",), want=("pbar",))["pbar"]
    for b in range(B):
        sc = ar.products_of(dn[combo][b], z=d["z"][b])["scale"]["wbar"]
        f = float(np.max(np.max(np.abs(wz[:, :, b] - hv[:, :, b]), axis=0) / (ar.TOL * sc)))
        print(f"{name} scenario {b}: wbar(z) against products' hv, error / bound {f:.2e}")
        assert f <= 1.0, (name, b, f)
    for a in range(ar.NA):
        gp = s.param_products(x, p, None, lam_g=d["y"][:, a].T, obj_factor=0.0)["gp"]
        for b in range(B):
            sc = ar.products_of(dn[combo][b], y=d["y"][b])["scale"]["pbar"][a]
            err = np.abs(py[:, a, b] - gp[:, b])
            assert np.all(err[sc == 0] == 0.0), (name, a, b)
            f = float(np.max(err[sc > 0] / (ar.TOL * sc[sc > 0]), initial=0.0))
            print(f"{name} seed {a} scenario {b}: pbar(y) against param_products' gp, error / bound {f:.2e}")
            assert f <= 1.0, (name, a, b, f)


def test_batch_plumbing(monkeypatch):
    """All bitwise: na = 3 equals three na = 1 calls; a per-scenario copy of shared seeds equals
    the broadcast (leading dimension 0); host and device entry points agree for every subset of
    the seeds and of the outputs; the number of wavefronts a scenario's seeds are dealt to does
    not change the results; a NaN entry of one seed leaves the other seeds' outputs unchanged; a
    NaN in an entry of p that nothing reads (the target's third entry; a tail entry no index
    names) changes nothing and that entry's pbar is exactly 0."""
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, na = 66, 3
    d = er.draw_point(spec, B, seed=81)
    d.update(ar.draw_seeds(spec, B, na, seed=82))
    full = _ap(s, d, sigma=0.37)
    assert all(np.all(np.isfinite(full[k])) for k in KEYS)
    for b in (0, 65):
        _equal(_scn(_ap(s, d, slice(b, b + 1), sigma=0.37), 0), _scn(full, b), f"scenario {b}")
    # seeds are independent
    for a in range(na):
        single = _ap(s, d, sigma=0.37, over={k: d[k][:, a:a + 1] for k in ar.SEEDS})
        for k in KEYS:
            np.testing.assert_array_equal(single[k][:, 0], full[k][:, a], err_msg=f"{k} seed {a}")
    # shared seeds: broadcast against a copy per scenario; one seed as a vector
    sh = {k: np.ascontiguousarray(d[k][0].T) for k in ar.SEEDS}  # (n, na)
    shared = _ap(s, d, sigma=0.37, over=sh)
    _equal(shared, _ap(s, d, sigma=0.37, over={k: np.repeat(d[k][:1], B, axis=0) for k in ar.SEEDS}), "ld = 0")
    one = _ap(s, d, sigma=0.37, over={k: v[:, 0] for k, v in sh.items()})
    for k in KEYS:
        np.testing.assert_array_equal(one[k][:, 0], shared[k][:, 0], err_msg=k)
    # a NaN entry poisons its own seed only
    for sk, idx in (("y", 7), ("z", 6), ("Xb", 11)):
        dn_ = d[sk].copy()
        dn_[:, 1, idx] = np.nan
        poisoned = _ap(s, d, sigma=0.37, over={sk: dn_})
        for k in KEYS:
            np.testing.assert_array_equal(poisoned[k][:, [0, 2]], full[k][:, [0, 2]], err_msg=f"{k}, NaN in {sk}")
        assert np.all(np.any(np.isnan(poisoned["wbar"][:, 1]), axis=0) | np.any(np.isnan(poisoned["pbar"][:, 1]), axis=0)), sk
    # the chunk count: this class's workspace holds two slices of the kernel's 7,424 doubles
    assert s.memory_info()["ws_per_scenario"] // (8 * 7424) == 2
    for chunks in ("1", "2", "3"):
        monkeypatch.setenv("NMPC_PRODUCTS_CHUNKS", chunks)
        _equal(_ap(s, d, sigma=0.37), full, f"{chunks} chunks")
    monkeypatch.delenv("NMPC_PRODUCTS_CHUNKS")
    # device entry point: every subset of the seeds and of the outputs, against the host's
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g") + ar.SEEDS}
    shapes = {"wbar": (B, na, spec.nw), "pbar": (B, na, spec.np)}
    for seeds in SUBSETS:
        host = full if seeds == ar.SEEDS else _ap(s, d, sigma=0.37, seeds=seeds)
        for keys in (("wbar",), ("pbar",), KEYS):
            out = {k: torch.full(shapes[k], float("nan"), **f64) for k in keys}
            kw = {("Xbar" if k == "Xb" else k): dev[k] for k in seeds}
            s.adjoint_products_device(dev["w"], dev["p"], out, lam_g=dev["lam_g"], obj_factor=0.37, **kw)
            torch.cuda.synchronize()
            for k in keys:
                np.testing.assert_array_equal(out[k].cpu().numpy(), np.transpose(host[k], (2, 1, 0)),
                                              err_msg=f"{k} of {keys}, seeds {seeds}")
            if keys != KEYS:  # the host entry point with one output
                _equal(_ap(s, d, sigma=0.37, seeds=seeds, want=keys), {k: host[k] for k in keys}, f"host {keys} {seeds}")
    # entries of p that nothing reads: the target's third entry ...
    assert np.all(full["pbar"][10] == 0.0)
    pn = dict(d, p=d["p"].copy())
    pn["p"][:, 10] = np.nan
    _equal(_ap(s, pn, sigma=0.37), full, "NaN in the target's third entry of p")
    # ... and a tail entry that no obstacle or weight index names
    spec2 = dataclasses.replace(er.case_spec("dynamic"), np=18).validate()
    s2 = _solver(spec2)
    d2 = er.draw_point(er.case_spec("dynamic"), 3, seed=83)
    d2["p"] = np.concatenate([d2["p"], np.full((3, 1), 5.0)], axis=1)
    d2.update(ar.draw_seeds(spec2, 3, na, seed=84))
    ref2 = _ap(s2, d2)
    assert np.all(ref2["pbar"][17] == 0.0) and np.all(ref2["pbar"][10] == 0.0) and np.all(ref2["pbar"][11:17] != 0.0)
    d2["p"][:, 17] = np.nan
    d2["p"][:, 10] = np.nan
    _equal(_ap(s2, d2), ref2, "NaN in an unnamed tail entry of p")


def test_stage_zero_of_the_state_seed():
    """Xb alone: stage 0 of X is p[0:nx] itself, so Xb_0 enters pbar's x0 block exactly once --
    pbar(Xb) - pbar(Xb with stage 0 zeroed) is Xb_0 within the gate on both models, and on N = 1
    with Xb at stage 0 only pbar[0:nx] is Xb_0 bitwise, the rest of pbar and all of wbar 0."""
    for name in ("race_track_2", "uav5", "n1"):
        spec, d, dn = ar.reference(name)
        s = _solver(spec)
        nx = spec.nX // (spec.N + 1)
        x0 = d["Xb"].copy()
        x0[:, :, nx:] = 0.0
        rest = d["Xb"] - x0
        got = _ap(s, d, seeds=("Xb",))
        wo = _ap(s, d, seeds=("Xb",), over={"Xb": rest})
        only = _ap(s, d, seeds=("Xb",), over={"Xb": x0})
        np.testing.assert_array_equal(only["pbar"][:nx], _t(d["Xb"])[:nx], err_msg=name)
        assert np.all(only["pbar"][nx:] == 0.0) and np.all(only["wbar"] == 0.0), name
        for b in range(er.CASES[name]):
            sc = ar.products_of(dn[ar.COMBOS[0]][b], Xb=d["Xb"][b])["scale"]["pbar"][:, :nx]
            err = np.abs(got["pbar"][:nx, :, b].T - wo["pbar"][:nx, :, b].T - d["Xb"][b][:, :nx])
            f = float(np.max(err / (ar.TOL * sc)))
            print(f"{name} scenario {b}: Xb_0 enters the x0 block once, error / bound {f:.2e}")
            assert f <= 1.0, (name, b, f)


def test_adjoint_products_device_does_not_synchronise():
    """nmpc_adjoint_products_batch_dev only enqueues (the pattern of tests/test_gpu_param.py::
    test_param_products_device_does_not_synchronise): behind a spinning kernel on a side stream
    the call returns while the stream is still busy, and the results equal an unobstructed
    run's.  After a solve of the same B it allocates nothing."""
    import time
    import torch

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B, na = 64, 3
    d = er.draw_point(spec, B, seed=9)
    d.update(ar.draw_seeds(spec, B, na, seed=10))
    s(x0=np.zeros(spec.nw), lbx=d["lbx"], ubx=d["ubx"], lbg=d["lbg"], ubg=d["ubg"], p=d["p"].T)  # a solve of the same B
    mem = s.memory_info()
    assert mem["ws_bytes"] > 0
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in ("w", "p", "lam_g") + ar.SEEDS}
    st = torch.cuda.Stream()

    def outs():
        return {"wbar": torch.empty(B, na, spec.nw, **f64), "pbar": torch.empty(B, na, spec.np, **f64)}

    def go(o):
        s.adjoint_products_device(dev["w"], dev["p"], o, y=dev["y"], z=dev["z"], Xbar=dev["Xb"], lam_g=dev["lam_g"],
                                  stream=st)

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
    print(f"adjoint_products_device: call {call_ms:.2f} ms, spin {spin_ms:.0f} ms, stream busy after the call: {busy}")
    assert spin_ms > 100.0
    assert busy and call_ms < 0.25 * spin_ms, (call_ms, spin_ms)
    assert s.memory_info() == mem
    for k in o:
        np.testing.assert_array_equal(o[k].cpu().numpy(), ref[k].cpu().numpy(), err_msg=k)


def test_argument_validation_on_a_live_handle():
    """B <= 0, na <= 0, a NULL x or p, every seed NULL, both outputs NULL and a leading dimension
    that is neither 0 nor >= the vector length return NMPC_E_INVALID from both entry points
    before any device call: nothing is written, and the handle still works."""
    from nmpc_amd import _lib

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    L = _lib.lib()
    B, na = 2, 2
    nw, ng, npp, nX = spec.nw, spec.ng, spec.np, spec.nX
    d = er.draw_point(spec, B, seed=5)
    sd = ar.draw_seeds(spec, B, na, seed=6)
    arr = {"x": np.ascontiguousarray(d["w"]), "p": np.ascontiguousarray(d["p"]), "lam": np.ascontiguousarray(d["lam_g"]),
           "y": sd["y"], "z": sd["z"], "Xb": sd["Xb"], "wbar": np.full((B, na, nw), 7.0),
           "pbar": np.full((B, na, npp), 7.0)}
    dp, vp = C.POINTER(C.c_double), C.c_void_p

    def call(B_=B, na_=na, x="x", ld_x=nw, p="p", ld_p=npp, lam="lam", ld_lam=ng, y="y", ld_y=ng * na, z="z",
             ld_z=nw * na, Xb="Xb", ld_Xb=nX * na, wbar="wbar", pbar="pbar", dev=False):
        if dev:  # (host addresses as "device" pointers: a refused call never dereferences them)
            g = lambda k: vp(arr[k].ctypes.data) if k else vp(0)  # noqa: E731
        else:
            g = lambda k: arr[k].ctypes.data_as(dp) if k else None  # noqa: E731
        args = [s._h, B_, na_, g(x), ld_x, g(p), ld_p, g(lam), ld_lam, 1.0, g(y), ld_y, g(z), ld_z, g(Xb), ld_Xb,
                g(wbar), g(pbar)]
        return L.nmpc_adjoint_products_batch_dev(*args, vp(0)) if dev else L.nmpc_adjoint_products_batch(*args)

    # each with the full message of its rule; the last three break two rules at once: the earlier
    # one in the order of the checks answers
    req, ldm = "required pointer is null (x, p)", "leading dimension smaller than the vector length"
    seeds, outs = "every seed pointer is null (y, z, Xb)", "every output pointer is null (wbar, pbar)"
    for dev in (False, True):
        for what, kw, msg in (("B = 0", dict(B_=0), "B <= 0"), ("B < 0", dict(B_=-3), "B <= 0"),
                              ("na = 0", dict(na_=0), "na <= 0"), ("na < 0", dict(na_=-1), "na <= 0"),
                              ("x NULL", dict(x=None), req), ("p NULL", dict(p=None), req),
                              ("every seed NULL", dict(y=None, z=None, Xb=None), seeds),
                              ("both outputs NULL", dict(wbar=None, pbar=None), outs),
                              ("ld_x short", dict(ld_x=nw - 1), ldm), ("ld_p short", dict(ld_p=npp - 1), ldm),
                              ("ld_lam_g short", dict(ld_lam=ng - 1), ldm), ("ld_y short", dict(ld_y=ng * na - 1), ldm),
                              ("ld_y one seed", dict(ld_y=ng), ldm), ("ld_z short", dict(ld_z=nw * na - 1), ldm),
                              ("ld_Xb short", dict(ld_Xb=nX * na - 1), ldm), ("ld_x negative", dict(ld_x=-nw), ldm),
                              ("B = 0 and na = 0", dict(B_=0, na_=0), "B <= 0"),
                              ("na = 0 and x NULL", dict(na_=0, x=None), "na <= 0"),
                              ("no seed and no output", dict(y=None, z=None, Xb=None, wbar=None, pbar=None), seeds),
                              ("no output and ld_x short", dict(wbar=None, pbar=None, ld_x=nw - 1), outs)):
            rc = call(dev=dev, **kw)
            assert rc == -1, (what, dev, rc)  # NMPC_E_INVALID
            assert L.nmpc_last_error(), what
            assert L.nmpc_last_error().decode() == msg, (what, dev)
    call(y=None, z=None, Xb=None)
    assert "seed" in L.nmpc_last_error().decode()
    call(wbar=None, pbar=None)
    assert "output" in L.nmpc_last_error().decode()
    with pytest.raises(_lib.NmpcError):
        _lib.check(call(na_=0))
    assert np.all(arr["wbar"] == 7.0) and np.all(arr["pbar"] == 7.0)  # nothing ran
    # and the handle still works: one seed and one output; leading dimension 0 shares everything
    assert call(y=None, z=None, wbar=None) == 0
    assert np.all(np.isfinite(arr["pbar"])) and np.all(arr["wbar"] == 7.0)
    assert call(ld_x=0, ld_p=0, ld_lam=0, ld_y=0, ld_z=0, ld_Xb=0) == 0
    for k in KEYS:
        assert np.all(np.isfinite(arr[k]))
        np.testing.assert_array_equal(arr[k][0], arr[k][1])
    with pytest.raises(ValueError):
        s.adjoint_products(d["w"].T, d["p"].T)
    with pytest.raises(ValueError):
        s.adjoint_products(d["w"].T, d["p"].T, y=np.zeros((ng, 2)), z=np.zeros((nw, 3)))


def _case_of_the_sensitivity_tests():
    from nmpc_amd import draw_scenarios

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B = 4
    P = draw_scenarios(spec, B, seed=7)
    lbx, ubx, lbg, ubg = spec.bounds()
    sol = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    assert np.all(np.isin(s.stats()["status_code"], (0, 1)))
    return spec, s, B, P, (lbx, ubx, lbg, ubg), sol


def _g(a, K, b):
    """The gate of one GPU product inside <a, K b>: TOL |a|_1 max_i (|K| |b|)_i."""
    return ar.TOL * float(np.sum(np.abs(a))) * float(np.max(np.abs(K) @ np.abs(b), initial=0.0))


def test_reverse_mode_sensitivity_of_a_solution():
    """race_track_2, N = 6, four scenarios, seed 7 (the case of tests/test_gpu_kkt.py and
    tests/test_gpu_param.py), random x_bar, lam_g_bar, X_bar ~ N(0, 1), na = 2.

    (a) q against the dense M at the returned delta: with r = x_bar + Z' X_bar + J' Sigma_s lam_g_bar
        on the free variables, rho(M, q, r) <= kkt_ref.TOL; fixed variables have q = 0 exactly.
    (b) pbar against C' (-q) + Jp' Sigma_s (lam_g_bar - J q) + Xp' X_bar with the checker's dense C, Jp,
        Xp and the GPU's own q and J q, within the pbar gate of tests/adjoint_ref.py: the wiring and
        the signs, without M's conditioning.
    (c) The adjoint identity against sensitivity(tangent="exact") with dp = I[:, :8]:
        D = <x_bar, dx> + <lam_g_bar, dlam_g> + <X_bar, dX*> - <pbar, dp>, dX* = Z dx + Xp dp.
        In exact arithmetic with M q = r and M dx = t (t = -C dp - J' Sigma_s Jp dp) both sides are
        <r, dx> + <Sigma_s lam_g_bar, Jp dp> + <X_bar, Xp dp> = <q, t> + ..., since M is symmetric.
        The computed q and dx have residuals e_q = M q - r, e_x = M dx - t with |e|_inf <= TOL den
        (den = | |M| |.| |_inf + |rhs|_inf, rho's denominator; (a) and tests/test_gpu_param.py bound
        them), so <r, dx> - <q, t> = <M q - e_q, dx> - <q, M dx - e_x> = <q, e_x> - <e_q, dx> and
            |D| <= TOL (|q|_1 den(dx) + |dx|_1 den(q)) + the product gates,
        the product gates being TOL |a|_1 max_i (|K| |b|)_i for each product <a, K b> a kernel formed
        on either side (each appears on both sides, hence the factor 2): <q, C dp>,
        <Sigma_s (|lam_g_bar| + |J| |q|), Jp dp>, <Sigma_s lam_g_bar, J dx>, <X_bar, Z dx>, <X_bar, Xp dp>.
        The measured defect over that bound and cond(M) are printed."""
    from oracle import nmpc_oracle as orc

    spec, s, B, P, (lbx, ubx, lbg, ubg), sol = _case_of_the_sensitivity_tests()
    prob = er.problem_of(spec)
    na, nd = 2, 8
    rng = np.random.default_rng(71)
    xb, lb, Xb = (rng.standard_normal((n, na, B)) for n in (spec.nw, spec.ng, spec.nX))
    got = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=xb, lam_g_bar=lb, X_bar=Xb)
    assert got["pbar"].shape == (spec.np, na, B) and got["info"].shape == (B,) and got["delta"].shape == (B,)
    print(f"reverse-mode sensitivity: info {got['info']}, delta {got['delta']}")
    assert np.all(got["info"] == 0)
    dp = np.eye(spec.np)[:, :nd]
    fwd = s.sensitivity(sol, lbx, ubx, lbg, ubg, P.T, dp, tangent="exact")
    np.testing.assert_array_equal(fwd["delta"], got["delta"])
    dXs = (s.products(sol["x"], P.T, fwd["dx"], lam_g=sol["lam_g"])["dX"]
           + s.param_products(sol["x"], P.T, dp, lam_g=sol["lam_g"])["dXp"])
    for b in range(B):
        x, lam, lx = sol["x"][:, b], sol["lam_g"][:, b], sol["lam_x"][:, b]
        ev = orc.SSEval(prob, x, P[b])
        dn = ar.dense(ev, 1.0, lam)
        J, Z, Cm, Jp, Xp = dn["J"], dn["Z"], dn["C"], dn["Jp"], dn["Xp"]
        sx = kr.barrier_weights(x, lx, lbx, ubx)
        ss = kr.barrier_weights(ev.g, lam, lbg, ubg)
        free = np.isfinite(sx)
        M = kr.dense_M(ev, dn["W"], np.where(free, sx, 0.0), ss, got["delta"][b])
        Mf = M[np.ix_(free, free)]
        aMf = np.abs(Mf)
        cond = float(np.linalg.cond(Mf))
        T = -(Cm @ dp) - J.T @ (ss[:, None] * (Jp @ dp))  # (nw, nd): the forward right-hand sides
        for a in range(na):
            q, jq = got["q"][:, a, b], got["jq"][:, a, b]
            r = xb[:, a, b] + Z.T @ Xb[:, a, b] + J.T @ (ss * lb[:, a, b])
            assert np.all(q[~free] == 0.0)
            rho = kr.rho(Mf, q[free], r[free])
            ref = ar.products_of(dn, y=(ss * (lb[:, a, b] - jq))[None], z=-q[None], Xb=Xb[:, a, b][None])
            fig = ar.check_against({"pbar": got["pbar"][:, a, b][None]}, ref, f"reverse-mode pbar, scenario {b} seed {a}")
            den_q = float(np.max(aMf @ np.abs(q[free]))) + float(np.max(np.abs(r[free])))
            worst = 0.0
            for j in range(nd):
                dx, dl = fwd["dx"][:, j, b], fwd["dlam_g"][:, j, b]
                D = (xb[:, a, b] @ dx + lb[:, a, b] @ dl + Xb[:, a, b] @ dXs[:, j, b]) - got["pbar"][:, a, b] @ dp[:, j]
                den_x = float(np.max(aMf @ np.abs(dx[free]))) + float(np.max(np.abs(T[free, j])))
                bound = kr.TOL * (np.sum(np.abs(q)) * den_x + np.sum(np.abs(dx)) * den_q)
                bound += 2 * (_g(q, Cm, dp[:, j]) + _g(ss * (np.abs(lb[:, a, b]) + np.abs(J) @ np.abs(q)), Jp, dp[:, j])
                              + _g(ss * lb[:, a, b], J, dx) + _g(Xb[:, a, b], Z, dx) + _g(Xb[:, a, b], Xp, dp[:, j]))
                worst = max(worst, abs(D) / bound)
                assert abs(D) <= bound, (b, a, j, D, bound)
            print(f"reverse-mode sensitivity scenario {b} seed {a}: rho(q) {rho:.2e} (bound {kr.TOL:.0e}), "
                  f"pbar error / bound {fig['pbar']:.2e}, adjoint identity defect / bound {worst:.2e}, cond(M) {cond:.1e}")
            assert rho <= kr.TOL, (b, a, rho)
    # one seed kind at a time, shared by the batch as a vector
    only = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=xb[:, 0, 0])
    assert only["pbar"].shape == (spec.np, 1, B) and np.all(np.isfinite(only["pbar"]))
    with pytest.raises(ValueError):
        s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T)
    with pytest.raises(ValueError):  # equality rows, as barrier_weights
        s.sensitivity_adjoint(sol, lbx, ubx, lbg, lbg, P.T, x_bar=xb)


def test_autograd_gradient_is_the_reverse_mode_sensitivity():
    """torch.autograd.grad of a random linear loss on (x, X) through nmpc_amd.autograd.solve
    equals sensitivity_adjoint's pbar for the same seeds bitwise; with max_iter = 1 no scenario
    converges and every row of the gradient is NaN."""
    import torch
    from nmpc_amd import REFERENCE_OPTS, autograd, draw_scenarios

    spec = er.case_spec("race_track_2")
    s = _solver(spec)
    B = 4
    P = draw_scenarios(spec, B, seed=7)
    lbx, ubx, lbg, ubg = spec.bounds()
    f64 = dict(dtype=torch.float64, device="cuda")
    rng = np.random.default_rng(72)
    cx, cX = rng.standard_normal((B, spec.nw)), rng.standard_normal((B, spec.nX))
    p = torch.tensor(P, requires_grad=True, **f64)
    x, X = autograd.solve(s, p, lbx, ubx, lbg, ubg)
    assert tuple(x.shape) == (B, spec.nw) and tuple(X.shape) == (B, spec.nX)
    loss = (torch.tensor(cx, **f64) * x).sum() + (torch.tensor(cX, **f64) * X).sum()
    (g,) = torch.autograd.grad(loss, p)
    assert tuple(g.shape) == (B, spec.np)
    # the same solve, by hand
    out = {"x": torch.empty(B, spec.nw, **f64), "g": torch.empty(B, spec.ng, **f64),
           "lam_x": torch.empty(B, spec.nw, **f64), "lam_g": torch.empty(B, spec.ng, **f64),
           "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    s.solve_device(torch.zeros(B, spec.nw, **f64), *(torch.tensor(v, **f64) for v in (lbx, ubx, lbg, ubg)),
                   torch.tensor(P, **f64), out)
    torch.cuda.synchronize()
    assert np.all(np.isin(out["status"].cpu().numpy(), (0, 1)))
    np.testing.assert_array_equal(x.detach().cpu().numpy(), out["x"].cpu().numpy())
    sol = {k: out[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
    ref = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=cx.T[:, None, :], X_bar=cX.T[:, None, :])
    assert np.all(ref["info"] == 0) and np.all(np.isfinite(ref["pbar"]))
    np.testing.assert_array_equal(g.cpu().numpy(), ref["pbar"][:, 0, :].T)
    # a loss on x alone: X's seed is absent
    x, X = autograd.solve(s, p, lbx, ubx, lbg, ubg)
    (gx,) = torch.autograd.grad((torch.tensor(cx, **f64) * x).sum(), p)
    refx = s.sensitivity_adjoint(sol, lbx, ubx, lbg, ubg, P.T, x_bar=cx.T[:, None, :])
    np.testing.assert_array_equal(gx.cpu().numpy(), refx["pbar"][:, 0, :].T)
    # no scenario converges in one iteration: NaN rows, never zeros
    opts = dict(REFERENCE_OPTS, ipopt=dict(REFERENCE_OPTS["ipopt"], max_iter=1))
    s1 = _solver(spec, opts)
    p1 = torch.tensor(P, requires_grad=True, **f64)
    x1, X1 = autograd.solve(s1, p1, lbx, ubx, lbg, ubg)
    (g1,) = torch.autograd.grad((torch.tensor(cx, **f64) * x1).sum() + (torch.tensor(cX, **f64) * X1).sum(), p1)
    assert np.all(np.isnan(g1.cpu().numpy()))
