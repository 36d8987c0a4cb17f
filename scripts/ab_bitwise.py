"""Dev tool: dump every output of a cold batched solve and a fused closed loop
(config 3, B scenarios, K steps) to an .npz, so two builds of the library
(NMPC_LIB=...) can be compared bit for bit:

    python scripts/ab_bitwise.py out_a.npz        # default library
    NMPC_LIB=exp/other.so python scripts/ab_bitwise.py out_b.npz
    python scripts/ab_bitwise.py --compare out_a.npz out_b.npz

With --fused before the file name the dump is every output of the three entry points at a solve's
point (sensitivity_adjoint_fused, sensitivity_fused, policy_fused) and of kkt_solve instead: on
the solved cases of tests/solve_adjoint_ref.py (na = 3 seeds of all three kinds, nd = 3
directions), and on one batch per exit of the kernels -- fixed controls, info = -11, and info = 1
with the ladder exhausted.  On the solved cases it also dumps evaluate, products, param_products,
adjoint_products and policy_rollout (5 samples), each through the host entry point and through the
device one, so every batched entry point is covered, and the given-point kernels' other branches
through the device entry points: lam_g absent, one output at a time, one seed kind at a time, the
evaluation without the certificate and without any gradient.  The points themselves are dumped too, so equal inputs are shown, and
--compare takes NaNs in the same places as equal whatever their payloads.
"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "mpc-implementation_amd"))


def compare(a, b):
    A, Bz = np.load(a), np.load(b)
    bad = 0
    for k in A.files:
        x, y = A[k], Bz[k]
        same = x.shape == y.shape and np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes()
        if not same and x.shape == y.shape and x.dtype.kind == "f":  # NaN payloads may differ, positions not
            nx = np.isnan(x)
            same = np.array_equal(nx, np.isnan(y)) and (
                np.where(nx, 0.0, x).tobytes() == np.where(nx, 0.0, y).tobytes())
        ndiff = int(np.sum(x != y)) if not same else 0
        print(f"{k:28s} {'bitwise equal' if same else f'DIFFERS in {ndiff} entries'}")
        bad += not same
    return bad


def fused(path):
    sys.path.insert(0, ROOT)
    import torch  # before the library, as main() and the tests have it: the device paths need it
    torch.cuda.init()
    from nmpc_amd import nlpsol, REFERENCE_OPTS
    from tests import solve_adjoint_ref as sr

    def solver(spec, **ipopt):
        return nlpsol("solver", "ipopt", spec, dict(REFERENCE_OPTS, ipopt=dict(REFERENCE_OPTS["ipopt"], **ipopt)))

    out = {}

    def dump(tag, s, sol, bounds, P, B, spec, seed):
        rng = np.random.default_rng(seed)
        sd = {k: rng.standard_normal((n, 3, B)) for k, n in (("x_bar", spec.nw), ("lam_g_bar", spec.ng),
                                                              ("X_bar", spec.nX))}
        dp = rng.standard_normal((spec.np, 3, B))
        for name, r in (("adj", s.sensitivity_adjoint_fused(sol, *bounds, P.T, **sd)),
                        ("tan", s.sensitivity_fused(sol, *bounds, P.T, dp)),
                        ("pol", s.policy_fused(sol, *bounds, P.T, dp))):
            for k, v in r.items():
                out[f"{tag}_{name}_{k}"] = np.asarray(v)
        print(tag, "info", out[f"{tag}_adj_info"], out[f"{tag}_tan_info"], out[f"{tag}_pol_info"], "delta",
              out[f"{tag}_tan_delta"])
        return sd, dp

    def given_points(tag, s, sol, bounds, P, B, spec, sd, dp):
        """evaluate, products, param_products, adjoint_products and policy_rollout at the point, each
        through the host entry point and through the device one."""
        import torch

        def t(a):
            return torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")

        def bm(a):  # (n, k, B) -> the device layout (B, k, n)
            return t(np.transpose(a, (2, 1, 0)))

        def empty(**shapes):
            return {k: torch.empty(shp, dtype=torch.int32 if k == "nsat" else torch.float64, device="cuda")
                    for k, shp in shapes.items()}

        nw, ng, npp, nX, N = spec.nw, spec.ng, spec.np, spec.nX, spec.N
        nu, nx = nw // N, nX // (N + 1)
        x, lg, lx = sol["x"], sol["lam_g"], sol["lam_x"]
        dx, dP, dlg, dlx = t(x.T), t(P), t(lg.T), t(lx.T)
        db = [t(v) for v in bounds]
        pol = s.policy_fused(sol, *bounds, P.T)
        rng = np.random.default_rng(7)
        e0, w = 0.05 * rng.standard_normal((B, 5, nx)), 0.005 * rng.standard_normal((B, 5, N, nx))
        host = {"ev": s.evaluate(x, P.T, lam_g=lg, lam_x=lx, lbx=bounds[0], ubx=bounds[1], lbg=bounds[2], ubg=bounds[3]),
                "prod": s.products(x, P.T, sd["x_bar"], lam_g=lg, obj_factor=0.7),
                "pprod": s.param_products(x, P.T, dp, lam_g=lg, obj_factor=0.7),
                "adjp": s.adjoint_products(x, P.T, y=sd["lam_g_bar"], z=sd["x_bar"], Xbar=sd["X_bar"], lam_g=lg,
                                           obj_factor=0.7),
                "roll": s.policy_rollout(P, x.T, pol["X"], pol["K"], e0, w=w, lbx=bounds[0], ubx=bounds[1],
                                         lbg=bounds[2], ubg=bounds[3])}
        dev = {"ev": empty(f=(B,), g=(B, ng), X=(B, nX), grad_f=(B, nw), grad_l=(B, nw), kkt=(B, 5)),
               "prod": empty(jv=(B, 3, ng), hv=(B, 3, nw), dX=(B, 3, nX)),
               "pprod": empty(jp=(B, 3, ng), hp=(B, 3, nw), dXp=(B, 3, nX), gp=(B, npp)),
               "adjp": empty(wbar=(B, 3, nw), pbar=(B, 3, npp))}
        s.evaluate_device(dx, dP, dev["ev"], lam_g=dlg, lam_x=dlx, lbx=db[0], ubx=db[1], lbg=db[2], ubg=db[3])
        s.products_device(dx, dP, bm(sd["x_bar"]), dev["prod"], lam_g=dlg, obj_factor=0.7)
        s.param_products_device(dx, dP, bm(dp), dev["pprod"], lam_g=dlg, obj_factor=0.7)
        s.adjoint_products_device(dx, dP, dev["adjp"], y=bm(sd["lam_g_bar"]), z=bm(sd["x_bar"]), Xbar=bm(sd["X_bar"]),
                                  lam_g=dlg, obj_factor=0.7)
        Kraw = t(np.swapaxes(pol["K"], -1, -2))  # the kernel's column-major blocks
        dev["roll"] = s.policy_rollout_device(dP, dx, t(pol["X"]), Kraw, t(e0), w=t(w), lbx=db[0], ubx=db[1],
                                              lbg=db[2], ubg=db[3], want=("J", "viol", "nsat", "X", "U"))
        # the kernels' other branches, through the device entry points (an absent output or input is a
        # null pointer there): lam_g absent; one output at a time; one seed kind at a time; the
        # evaluation without the certificate and without any gradient
        v3, dp3 = bm(sd["x_bar"]), bm(dp)
        seeds = {"y": bm(sd["lam_g_bar"]), "z": v3, "Xbar": bm(sd["X_bar"])}
        br = {"ev_noy": empty(f=(B,), g=(B, ng), X=(B, nX), grad_f=(B, nw), grad_l=(B, nw), kkt=(B, 5)),
              "ev_nokkt": empty(f=(B,), g=(B, ng), X=(B, nX), grad_f=(B, nw), grad_l=(B, nw)),
              "ev_nograd": empty(f=(B,), g=(B, ng), X=(B, nX)),
              "prod_noy": empty(jv=(B, 3, ng), hv=(B, 3, nw), dX=(B, 3, nX)),
              "prod_jv": empty(jv=(B, 3, ng)), "prod_hv": empty(hv=(B, 3, nw)),
              "pprod_noy": empty(jp=(B, 3, ng), hp=(B, 3, nw), dXp=(B, 3, nX), gp=(B, npp)),
              "pprod_gp": empty(gp=(B, npp)), "pprod_nohp": empty(jp=(B, 3, ng), dXp=(B, 3, nX), gp=(B, npp)),
              "adjp_noy": empty(wbar=(B, 3, nw), pbar=(B, 3, npp)),
              "adjp_wbar": empty(wbar=(B, 3, nw)), "adjp_pbar": empty(pbar=(B, 3, npp))}
        s.evaluate_device(dx, dP, br["ev_noy"], lam_x=dlx, lbx=db[0], ubx=db[1], lbg=db[2], ubg=db[3])
        s.evaluate_device(dx, dP, br["ev_nokkt"], lam_g=dlg, lam_x=dlx)
        s.evaluate_device(dx, dP, br["ev_nograd"], lam_g=dlg)
        s.products_device(dx, dP, v3, br["prod_noy"], obj_factor=0.7)
        s.products_device(dx, dP, v3, br["prod_jv"], lam_g=dlg, obj_factor=0.7)
        s.products_device(dx, dP, v3, br["prod_hv"], lam_g=dlg, obj_factor=0.7)
        s.param_products_device(dx, dP, dp3, br["pprod_noy"], obj_factor=0.7)
        s.param_products_device(dx, dP, None, br["pprod_gp"], lam_g=dlg, obj_factor=0.7)
        s.param_products_device(dx, dP, dp3, br["pprod_nohp"], lam_g=dlg, obj_factor=0.7)
        s.adjoint_products_device(dx, dP, br["adjp_noy"], obj_factor=0.7, **seeds)
        s.adjoint_products_device(dx, dP, br["adjp_wbar"], lam_g=dlg, obj_factor=0.7, **seeds)
        s.adjoint_products_device(dx, dP, br["adjp_pbar"], lam_g=dlg, obj_factor=0.7, **seeds)
        for kind, seed in seeds.items():
            br[f"adjp_{kind}"] = empty(wbar=(B, 3, nw), pbar=(B, 3, npp))
            s.adjoint_products_device(dx, dP, br[f"adjp_{kind}"], lam_g=dlg, obj_factor=0.7, **{kind: seed})
        torch.cuda.synchronize()
        for name in br:
            for k, v in br[name].items():
                out[f"{tag}_{name}_dev_{k}"] = v.cpu().numpy()
        for name in host:
            for k, v in host[name].items():
                out[f"{tag}_{name}_{k}"] = np.asarray(v)
            for k, v in dev[name].items():
                out[f"{tag}_{name}_dev_{k}"] = v.cpu().numpy()

    for name, (B, _) in sr.SOLVED.items():
        spec, P = sr.scenarios(name)
        s = solver(spec)
        bounds = spec.bounds()
        sol = s(x0=np.zeros(spec.nw), lbx=bounds[0], ubx=bounds[1], lbg=bounds[2], ubg=bounds[3], p=P.T)
        sol = {k: np.array(sol[k], dtype=np.float64).reshape(-1, B) for k in ("x", "g", "lam_x", "lam_g")}
        for k, v in sol.items():
            out[f"{name}_point_{k}"] = v
        sd, dp = dump(name, s, sol, bounds, P, B, spec, 1)
        given_points(name, s, sol, bounds, P, B, spec, sd, dp)
        # the KKT solves at the point's weights, at delta = 0 and at a delta every case factorises with
        sx, ss = s.barrier_weights(sol, *bounds)
        for dl in (0.0, 1e-4):
            r = s.kkt_solve(sol["x"], P.T, r_w=sd["x_bar"], r_g=sd["lam_g_bar"], lam_g=sol["lam_g"], sigma_x=sx,
                            sigma_s=ss, delta=dl)
            for k, v in r.items():
                out[f"{name}_kkt{dl:g}_{k}"] = np.asarray(v)
        # the KKT kernel's other branches: no row right-hand side, no multipliers
        for tag, kw in (("norg", dict(r_w=sd["x_bar"], lam_g=sol["lam_g"])),
                        ("noy", dict(r_w=sd["x_bar"], r_g=sd["lam_g_bar"]))):
            r = s.kkt_solve(sol["x"], P.T, sigma_x=sx, sigma_s=ss, delta=1e-4, **kw)
            for k, v in r.items():
                out[f"{name}_kkt_{tag}_{k}"] = np.asarray(v)
        if name != "race_track_2":
            continue
        lbx, ubx, lbg, ubg = bounds
        nu = spec.nw // spec.N
        # a third of the controls fixed, a whole stage among them
        fx = np.random.default_rng(78).uniform(size=(spec.nw, B)) < 1.0 / 3.0
        fx[:nu, 0] = True
        lb2, ub2 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
        lb2[fx], ub2[fx] = sol["x"][fx], sol["x"][fx]
        dump("fixed", s, sol, (lb2, ub2, lbg, ubg), P, B, spec, 2)
        # info = -11: lbx > ubx in scenario 1, a NaN multiplier in scenario 2
        lb3, ub3 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
        lb3[5, 1] = ub3[5, 1] + 1.0
        sol3 = dict(sol, lam_g=sol["lam_g"].copy())
        sol3["lam_g"][3, 2] = np.nan
        dump("invalid", s, sol3, (lb3, ub3, lbg, ubg), P, B, spec, 3)
        # the ladder: many rungs from 1e-12, then none allowed (info = 1) but for scenario 0, whose last
        # stage is fixed
        dump("rungs", solver(spec, first_hessian_perturbation=1e-12), sol, bounds, P, B, spec, 4)
        lb4, ub4 = (np.repeat(v[:, None], B, axis=1) for v in (lbx, ubx))
        lb4[-nu:, 0] = ub4[-nu:, 0] = sol["x"][-nu:, 0]
        dump("stuck", solver(spec, max_hessian_perturbation=1e-6), sol, (lb4, ub4, lbg, ubg), P, B, spec, 5)
    np.savez(path, **{k: v for k, v in out.items() if v.dtype != object})
    print("saved", path, len(out), "arrays")


def main():
    if sys.argv[1] == "--compare":
        sys.exit(1 if compare(sys.argv[2], sys.argv[3]) else 0)
    if sys.argv[1] == "--fused":
        return fused(sys.argv[2])
    import torch
    from nmpc_amd import nlpsol, config_spec, draw_scenarios, REFERENCE_OPTS
    B = int(os.environ.get("AB_B", "4096")); K = int(os.environ.get("AB_K", "20"))
    cfg = int(os.environ.get("AB_CONFIG", "3"))
    spec = config_spec(cfg)
    P = draw_scenarios(spec, B, seed=1000 + cfg)
    lbx, ubx, lbg, ubg = spec.bounds()
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    sol = s(x0=np.zeros(spec.nw), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, p=P.T)
    st = s.stats()
    out = {"cold_x": sol["x"], "cold_f": sol["f"], "cold_status": np.asarray(st["status_code"]),
           "cold_iters": np.asarray(st["iter_count"])}
    dev = dict(dtype=torch.float64, device="cuda")
    bnd = [torch.tensor(v, **dev) for v in (lbx, ubx, lbg, ubg)]
    p = torch.tensor(P, **dev).contiguous()
    w = torch.zeros(B, spec.nw, **dev)
    hist = {"u": torch.empty(K, B, 6, **dev), "f": torch.empty(K, B, **dev), "fov": torch.zeros(K, B, **dev),
            "status": torch.empty(K, B, dtype=torch.int32, device="cuda"),
            "iters": torch.empty(K, B, dtype=torch.int32, device="cuda")}
    s.closed_loop_device(K, *bnd, p, w, torch.full((B,), 12.0, **dev), torch.full((B,), 0.01, **dev), hist)
    torch.cuda.synchronize()
    for k, v in hist.items():
        out["cl_" + k] = v.cpu().numpy()
    out["cl_p_final"] = p.cpu().numpy()
    out["cl_w_final"] = w.cpu().numpy()
    np.savez(sys.argv[1], **out)
    print("saved", sys.argv[1], "mean cold iters", out["cold_iters"].mean(), "closed-loop iters",
          out["cl_iters"].mean())


if __name__ == "__main__":
    main()
