"""Cost of one nmpc_param_products_batch_dev call at the config-3 shape (B = 4,096, N = 20, 10
obstacles, all four outputs, multipliers given), per number of directions (1, 8 and np), next
to one nmpc_products_batch_dev call with as many directions and one nmpc_eval_batch_dev call at
the same points (scripts/products_timing.py's and scripts/eval_timing.py's figures) -- and so
next to the 2 nd evaluation calls whose central differences one exact sensitivity right-hand
side (Solver.sensitivity(tangent="exact"): one call, nd directions) replaces.

    python scripts/pproducts_timing.py [--points 4096] [--calls 500] [--nd 1 8 11]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream
(median, min, max reported), and the whole train of calls by one more pair (mean per call, back
to back).  Prints one JSON line per leg."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]

from scripts.products_timing import timed  # noqa: E402


def main(B, calls, nds):
    import torch
    from nmpc_amd import config_spec, nlpsol, REFERENCE_OPTS
    from tests import eval_ref as er
    from tests import param_ref as qr
    from tests import products_ref as pr

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    prob = er.problem_of(spec)
    d = er.draw_point(spec, B, seed=4096)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in d}
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "device": torch.cuda.get_device_name(0)}
    eo = {"f": torch.empty(B, **f64), "g": torch.empty(B, spec.ng, **f64), "X": torch.empty(B, spec.nX, **f64),
          "grad_f": torch.empty(B, spec.nw, **f64), "grad_l": torch.empty(B, spec.nw, **f64),
          "kkt": torch.empty(B, 5, **f64)}
    ev = timed(lambda: s.evaluate_device(dev["w"], dev["p"], eo, lam_g=dev["lam_g"], lam_x=dev["lam_x"], lbx=dev["lbx"],
                                         ubx=dev["ubx"], lbg=dev["lbg"], ubg=dev["ubg"]), calls)
    print(json.dumps({"leg": "evaluate", **shape, **ev}), flush=True)
    # what the difference quotients' evaluations ask for: g and grad_l, no certificate
    fo = {"g": eo["g"], "grad_l": eo["grad_l"]}
    fd = timed(lambda: s.evaluate_device(dev["w"], dev["p"], fo, lam_g=dev["lam_g"]), calls)
    print(json.dumps({"leg": "evaluate_g_grad_l", **shape, **fd}), flush=True)
    for nd in nds:
        nd = spec.np if nd <= 0 else nd
        v = torch.tensor(pr.draw_directions(spec, nd, B, seed=11), **f64)
        po = {"jv": torch.empty(B, nd, spec.ng, **f64), "hv": torch.empty(B, nd, spec.nw, **f64),
              "dX": torch.empty(B, nd, spec.nX, **f64)}
        r = timed(lambda: s.products_device(dev["w"], dev["p"], v, po, lam_g=dev["lam_g"], obj_factor=1.0), calls)
        print(json.dumps({"leg": "products", "nv": nd, **shape, **r}), flush=True)
        dp = torch.tensor(qr.draw_directions(prob, d["p"], nd, seed=12), **f64)
        qo = {"jp": torch.empty(B, nd, spec.ng, **f64), "hp": torch.empty(B, nd, spec.nw, **f64),
              "dXp": torch.empty(B, nd, spec.nX, **f64), "gp": torch.empty(B, spec.np, **f64)}
        r = timed(lambda: s.param_products_device(dev["w"], dev["p"], dp, qo, lam_g=dev["lam_g"], obj_factor=1.0), calls)
        assert all(bool(torch.isfinite(t).all()) for t in qo.values())
        print(json.dumps({"leg": "param_products", "nd": nd, **shape, **r,
                          "fd_evaluations_replaced": 2 * nd, "fd_evaluations_ms": 2 * nd * fd["per_call_ms_median"]}),
              flush=True)
        ro = {"jp": qo["jp"], "hp": qo["hp"]}  # one sensitivity right-hand side: these two alone
        r = timed(lambda: s.param_products_device(dev["w"], dev["p"], dp, ro, lam_g=dev["lam_g"], obj_factor=1.0), calls)
        print(json.dumps({"leg": "param_products_jp_hp", "nd": nd, **shape, **r,
                          "fd_evaluations_ms": 2 * nd * fd["per_call_ms_median"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--nd", type=int, nargs="+", default=[1, 8, 0], help="numbers of directions (0 = np)")
    a = ap.parse_args()
    main(a.points, a.calls, a.nd)
