"""Cost of the forward-mode sensitivity of a solution at the config-3 shape (B = 4,096, N = 20, 10
obstacles; the batch is solved first, so the points, multipliers and the delta ladder are real),
per number of directions (1, 8, and the feedback gain's nx unit directions).  Legs, all in one
session, `--rounds` times in turn:
  fused:   one nmpc_solve_tangent_batch_dev launch (Solver.sensitivity_device): weights, ladder,
           parameter products and solves, dx, dlam_g and dX out;
  kernels: the parent's two device kernels for the same dx and dlam_g -- param_products_device (jp
           and hp alone), kkt_solve_device at the delta the ladder ends on (weights given, one
           factorisation) -- each alone and as a sequence; what Solver.sensitivity(tangent="exact")
           would cost without its host part;
  gain:    Solver.feedback_gain_device (the fused launch with nx shared unit directions and the
           torch ops that arrange K);
  host:    Solver.sensitivity(tangent="exact") itself, starting from the device-resident solution
           and directions and ending with dx back on the device: wall clock, its copies included.

    python scripts/solve_tangent_timing.py [--points 4096] [--calls 500] [--nd 1 8] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call (or sequence) is bracketed by its own pair of HIP events on the
stream (median, min, max reported), and the whole train by one more pair (mean, back to back).
Prints one JSON line per leg and round, then one summary line per nd with the medians over the
rounds, their span and the ratios."""
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


def main(B, calls, nds, rounds, host_calls):
    import torch
    from nmpc_amd import config_spec, draw_scenarios, nlpsol, REFERENCE_OPTS

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    P = draw_scenarios(spec, B, seed=4096)
    bounds = spec.bounds()
    db = [torch.tensor(np.asarray(v, dtype=np.float64), **f64) for v in bounds]
    dP = torch.tensor(P, **f64)
    sol = {"x": torch.empty(B, spec.nw, **f64), "g": torch.empty(B, spec.ng, **f64),
           "lam_x": torch.empty(B, spec.nw, **f64), "lam_g": torch.empty(B, spec.ng, **f64),
           "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    s.solve_device(torch.zeros(B, spec.nw, **f64), *db, dP, sol)
    torch.cuda.synchronize()
    ok = int(((sol["status"] == 0) | (sol["status"] == 1)).sum())
    nx = spec.nX // (spec.N + 1)
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "np": spec.np, "nx": nx, "converged": ok,
             "device": torch.cuda.get_device_name(0)}
    hsol = {k: sol[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
    sx, ss = s.barrier_weights(hsol, *bounds)
    dsx, dss = torch.tensor(np.ascontiguousarray(sx.T), **f64), torch.tensor(np.ascontiguousarray(ss.T), **f64)
    rng = np.random.default_rng(17)
    for nd in nds:
        dd = torch.tensor(rng.standard_normal((B, nd, spec.np)), **f64)
        fo = {"dx": torch.empty(B, nd, spec.nw, **f64), "dlam_g": torch.empty(B, nd, spec.ng, **f64),
              "dX": torch.empty(B, nd, spec.nX, **f64), "info": torch.empty(B, dtype=torch.int32, device="cuda"),
              "delta": torch.empty(B, **f64)}

        def fused():
            s.sensitivity_device(sol, *db, dP, dd, fo)

        fused()
        torch.cuda.synchronize()
        good = int((fo["info"] == 0).sum())
        delta = fo["delta"].clone()
        rungs = {float(v): int(c) for v, c in zip(*np.unique(delta.cpu().numpy(), return_counts=True))}
        po = {"jp": torch.empty(B, nd, spec.ng, **f64), "hp": torch.empty(B, nd, spec.nw, **f64)}
        ko = {"dw": torch.empty(B, nd, spec.nw, **f64), "jdw": torch.empty(B, nd, spec.ng, **f64),
              "info": torch.empty(B, dtype=torch.int32, device="cuda")}

        def k1():
            s.param_products_device(sol["x"], dP, dd, po, lam_g=sol["lam_g"])

        def k2():  # (hp and jp stand for -hp and -Sigma_s jp: the same work)
            s.kkt_solve_device(sol["x"], dP, ko, r_w=po["hp"], r_g=po["jp"], lam_g=sol["lam_g"], sigma_x=dsx,
                               sigma_s=dss, delta=delta)

        def kernels():
            k1(); k2()

        def gain():
            s.feedback_gain_device(sol, *db, dP)

        def host():
            hs = {k: sol[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
            d = np.ascontiguousarray(dd.cpu().numpy().transpose(2, 1, 0))
            r = s.sensitivity(hs, *bounds, dP.cpu().numpy().T, d, tangent="exact")
            return torch.tensor(np.ascontiguousarray(r["dx"].transpose(2, 1, 0)), **f64)

        med = {"fused": [], "kernels": [], "k1": [], "k2": [], "gain": [], "host": []}
        for rd in range(rounds):
            for leg, go in (("fused", fused), ("k1", k1), ("k2", k2), ("kernels", kernels), ("gain", gain)):
                r = timed(go, calls)
                med[leg].append(r["per_call_ms_median"])
                print(json.dumps({"leg": leg, "nd": nx if leg == "gain" else nd, "round": rd, **shape, **r}), flush=True)
            for _ in range(2):
                host()
            torch.cuda.synchronize()
            ms = []
            for _ in range(host_calls):
                t0 = time.perf_counter()
                host()
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
            med["host"].append(float(np.median(ms)))
            print(json.dumps({"leg": "host", "nd": nd, "round": rd, **shape, "calls": host_calls,
                              "wall_ms_median": float(np.median(ms)), "wall_ms_min": float(np.min(ms)),
                              "wall_ms_max": float(np.max(ms))}), flush=True)
        assert bool((ko["info"] == 0).sum() == good)
        m = {k: float(np.median(v)) for k, v in med.items()}
        print(json.dumps({"leg": "summary", "nd": nd, **shape, "info_0": good, "delta_counts": rungs,
                          "median_ms": m, "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                          "two_kernels_sum_ms": m["k1"] + m["k2"],
                          "fused_over_two_kernels_sum": m["fused"] / (m["k1"] + m["k2"]),
                          "fused_over_sequence": m["fused"] / m["kernels"],
                          "host_over_fused": m["host"] / m["fused"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--nd", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=10)
    a = ap.parse_args()
    main(a.points, a.calls, a.nd, a.rounds, a.host_calls)
