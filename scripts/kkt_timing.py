"""Cost of one nmpc_kkt_solve_batch_dev call at the config-3 shape (B = 4,096, N = 20, 10
obstacles, all three outputs and the verdicts, multipliers and both weights given), per number
of right-hand sides, next to one nmpc_eval_batch_dev and one nmpc_products_batch_dev call at the
same points (scripts/eval_timing.py's and scripts/products_timing.py's figures), and next to
the host-side dense alternative: numpy.linalg.solve on Solver.hessian / Solver.jacobian output.

    python scripts/kkt_timing.py [--points 4096] [--calls 500] [--nr 1 2 8] [--dense-points 256]   # needs an MI355X

delta is the smallest of 1, 10, 100, ... with which every scenario factorises (a scenario with
the wrong inertia stops at its first failing pivot and would flatter the figure).  After 20
warm-up calls every call is bracketed by its own pair of HIP events on the stream (median, min,
max reported), and the whole train of calls by one more pair (mean per call, back to back).
The dense leg runs on the first --dense-points scenarios (the dense Jacobians of 4,096 would
not fit a sensible host buffer) and is reported per scenario.  Prints one JSON line per leg."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]

from scripts.products_timing import timed  # noqa: E402


def main(B, calls, nrs, nd):
    import torch
    from nmpc_amd import config_spec, nlpsol, REFERENCE_OPTS
    from tests import eval_ref as er
    from tests import kkt_ref as kr
    from tests import products_ref as pr

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    d = er.draw_point(spec, B, seed=4096)
    sx, ss = kr.draw_weights(spec, B, "mild", seed=13)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in d}
    dev["sigma_x"], dev["sigma_s"] = torch.tensor(sx, **f64), torch.tensor(ss, **f64)
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "device": torch.cuda.get_device_name(0)}
    eo = {"f": torch.empty(B, **f64), "g": torch.empty(B, spec.ng, **f64), "X": torch.empty(B, spec.nX, **f64),
          "grad_f": torch.empty(B, spec.nw, **f64), "grad_l": torch.empty(B, spec.nw, **f64),
          "kkt": torch.empty(B, 5, **f64)}
    r = timed(lambda: s.evaluate_device(dev["w"], dev["p"], eo, lam_g=dev["lam_g"], lam_x=dev["lam_x"], lbx=dev["lbx"],
                                        ubx=dev["ubx"], lbg=dev["lbg"], ubg=dev["ubg"]), calls)
    print(json.dumps({"leg": "evaluate", **shape, **r}), flush=True)
    rng = np.random.default_rng(17)
    delta = None
    for nr in nrs:
        v = torch.tensor(pr.draw_directions(spec, nr, B, seed=11), **f64)
        po = {"jv": torch.empty(B, nr, spec.ng, **f64), "hv": torch.empty(B, nr, spec.nw, **f64),
              "dX": torch.empty(B, nr, spec.nX, **f64)}
        r = timed(lambda: s.products_device(dev["w"], dev["p"], v, po, lam_g=dev["lam_g"], obj_factor=1.0), calls)
        print(json.dumps({"leg": "products", "nv": nr, **shape, **r}), flush=True)
        rw = torch.tensor(rng.standard_normal((B, nr, spec.nw)), **f64)
        rg = torch.tensor(rng.standard_normal((B, nr, spec.ng)), **f64)
        out = {"dw": torch.empty(B, nr, spec.nw, **f64), "dX": torch.empty(B, nr, spec.nX, **f64),
               "jdw": torch.empty(B, nr, spec.ng, **f64), "info": torch.empty(B, dtype=torch.int32, device="cuda")}

        def go():
            s.kkt_solve_device(dev["w"], dev["p"], out, r_w=rw, r_g=rg, lam_g=dev["lam_g"], obj_factor=1.0,
                               sigma_x=dev["sigma_x"], sigma_s=dev["sigma_s"], delta=delta)

        if delta is None:
            for e in range(0, 13):
                delta = torch.tensor([10.0 ** e], **f64)
                go()
                torch.cuda.synchronize()
                if bool((out["info"] == 0).all()):
                    break
        r = timed(go, calls)
        assert bool((out["info"] == 0).all()) and all(bool(torch.isfinite(out[k]).all()) for k in ("dw", "dX", "jdw"))
        print(json.dumps({"leg": "kkt_solve", "nr": nr, "delta": float(delta[0]), **shape, **r}), flush=True)
    # the host-side dense alternative on the first nd scenarios
    nd = min(nd, B)
    w, p, lg = d["w"][:nd].T, d["p"][:nd].T, d["lam_g"][:nd].T
    dl = float(delta[0])
    rwh = rng.standard_normal((nd, spec.nw))
    t0 = time.perf_counter()
    W, J = s.hessian(w, p, lam_g=lg), s.jacobian(w, p)
    t1 = time.perf_counter()
    for b in range(nd):
        Jb = J[:, :, b]
        M = W[:, :, b] + np.diag(sx[b] + dl) + Jb.T @ ((ss[b] + dl)[:, None] * Jb)
        np.linalg.solve(M, rwh[b])
    t2 = time.perf_counter()
    print(json.dumps({"leg": "host_dense", "points": nd, "nw": spec.nw, "ng": spec.ng,
                      "matrices_ms_per_scenario": (t1 - t0) * 1e3 / nd, "solve_ms_per_scenario": (t2 - t1) * 1e3 / nd,
                      "ms_for_B": (t2 - t0) * 1e3 / nd * B, "B": B}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--nr", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--dense-points", type=int, default=256)
    a = ap.parse_args()
    main(a.points, a.calls, a.nr, a.dense_points)
