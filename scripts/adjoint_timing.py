"""Cost of one nmpc_adjoint_products_batch_dev call at the config-3 shape (B = 4,096, N = 20, 10
obstacles, all three seeds, both outputs, multipliers given), per number of seeds (1 and 8),
next to the two routes to a full gradient d loss / d p through a solution:
  reverse: one nmpc_kkt_solve_batch_dev call with na right-hand sides plus one adjoint call with
           na seeds (Solver.sensitivity_adjoint's device sequence; na losses at once);
  forward: one nmpc_param_products_batch_dev call with nd = np directions (jp and hp) plus one
           nmpc_kkt_solve_batch_dev call with nr = np right-hand sides (Solver.sensitivity with
           tangent="exact" and dp = I), whatever the number of losses.

    python scripts/adjoint_timing.py [--points 4096] [--calls 500] [--na 1 8]   # needs an MI355X

delta as scripts/kkt_timing.py picks it.  After 20 warm-up calls every call (or sequence of two)
is bracketed by its own pair of HIP events on the stream (median, min, max reported), and the
whole train by one more pair (mean, back to back).  Prints one JSON line per leg."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]

from scripts.products_timing import timed  # noqa: E402


def main(B, calls, nas):
    import torch
    from nmpc_amd import config_spec, nlpsol, REFERENCE_OPTS
    from tests import adjoint_ref as ar
    from tests import eval_ref as er
    from tests import kkt_ref as kr
    from tests import param_ref as qr

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    prob = er.problem_of(spec)
    d = er.draw_point(spec, B, seed=4096)
    sx, ss = kr.draw_weights(spec, B, "mild", seed=13)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in d}
    dev["sigma_x"], dev["sigma_s"] = torch.tensor(sx, **f64), torch.tensor(ss, **f64)
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "np": spec.np, "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(17)

    def kkt(nr):
        rw = torch.tensor(rng.standard_normal((B, nr, spec.nw)), **f64)
        rg = torch.tensor(rng.standard_normal((B, nr, spec.ng)), **f64)
        out = {"dw": torch.empty(B, nr, spec.nw, **f64), "jdw": torch.empty(B, nr, spec.ng, **f64),
               "info": torch.empty(B, dtype=torch.int32, device="cuda")}
        return out, lambda delta: s.kkt_solve_device(dev["w"], dev["p"], out, r_w=rw, r_g=rg, lam_g=dev["lam_g"],
                                                     obj_factor=1.0, sigma_x=dev["sigma_x"], sigma_s=dev["sigma_s"],
                                                     delta=delta)

    out1, go1 = kkt(1)
    for e in range(0, 13):
        delta = torch.tensor([10.0 ** e], **f64)
        go1(delta)
        torch.cuda.synchronize()
        if bool((out1["info"] == 0).all()):
            break
    # forward route: np directions and np right-hand sides
    nd = spec.np
    dp = torch.tensor(qr.draw_directions(prob, d["p"], nd, seed=12), **f64)
    ro = {"jp": torch.empty(B, nd, spec.ng, **f64), "hp": torch.empty(B, nd, spec.nw, **f64)}
    outn, gon = kkt(nd)

    def forward():
        s.param_products_device(dev["w"], dev["p"], dp, ro, lam_g=dev["lam_g"], obj_factor=1.0)
        gon(delta)

    fw = timed(forward, calls)
    assert bool((outn["info"] == 0).all())
    print(json.dumps({"leg": "forward_route", "nd": nd, "nr": nd, "delta": float(delta[0]), **shape, **fw}), flush=True)
    for na in nas:
        sd = {k: torch.tensor(v, **f64) for k, v in ar.draw_seeds(spec, B, na, seed=21).items()}
        ao = {"wbar": torch.empty(B, na, spec.nw, **f64), "pbar": torch.empty(B, na, spec.np, **f64)}
        r = timed(lambda: s.adjoint_products_device(dev["w"], dev["p"], ao, y=sd["y"], z=sd["z"], Xbar=sd["Xb"],
                                                    lam_g=dev["lam_g"], obj_factor=1.0), calls)
        assert all(bool(torch.isfinite(t).all()) for t in ao.values())
        print(json.dumps({"leg": "adjoint_products", "na": na, **shape, **r}), flush=True)
        outa, goa = kkt(na)
        po = {"pbar": ao["pbar"]}

        def reverse():
            goa(delta)
            # (y and z stand for Sigma_s (lam_bar - J q) and -q: the same work as the real sequence)
            s.adjoint_products_device(dev["w"], dev["p"], po, y=outa["jdw"], z=outa["dw"], Xbar=sd["Xb"],
                                      lam_g=dev["lam_g"], obj_factor=1.0)

        r = timed(reverse, calls)
        assert bool((outa["info"] == 0).all()) and bool(torch.isfinite(po["pbar"]).all())
        print(json.dumps({"leg": "reverse_route", "na": na, "nr": na, "delta": float(delta[0]), **shape, **r,
                          "forward_route_ms_median": fw["per_call_ms_median"],
                          "forward_over_reverse": fw["per_call_ms_median"] / r["per_call_ms_median"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--na", type=int, nargs="+", default=[1, 8])
    a = ap.parse_args()
    main(a.points, a.calls, a.na)
