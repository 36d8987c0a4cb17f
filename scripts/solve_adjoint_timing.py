"""Cost of the reverse-mode sensitivity of a solution at the config-3 shape (B = 4,096, N = 20, 10
obstacles; the batch is solved first, so the points, multipliers and the delta ladder are real),
all three seeds, per number of seeds (1 and 8).  Three legs, all in one session, `--rounds` times
in turn:
  fused:   one nmpc_solve_adjoint_batch_dev launch (Solver.sensitivity_adjoint_device): weights,
           ladder, solves and pullback;
  kernels: the parent's three device kernels for the same result -- adjoint_products_device with
           X_bar alone (wbar), kkt_solve_device at the delta the ladder ends on (weights given, one
           factorisation), adjoint_products_device for pbar alone -- each alone and as a sequence;
           what Solver.sensitivity_adjoint would cost without its host part;
  host:    Solver.sensitivity_adjoint itself, starting from the device-resident solution and
           seeds and ending with pbar back on the device: wall clock, its copies included.

    python scripts/solve_adjoint_timing.py [--points 4096] [--calls 500] [--na 1 8] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call (or sequence) is bracketed by its own pair of HIP events on the
stream (median, min, max reported), and the whole train by one more pair (mean, back to back).
Prints one JSON line per leg and round, then one summary line per na with the medians over the
rounds, their span and the two ratios."""
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


def main(B, calls, nas, rounds, host_calls):
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
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "np": spec.np, "converged": ok,
             "device": torch.cuda.get_device_name(0)}
    hsol = {k: sol[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
    sx, ss = s.barrier_weights(hsol, *bounds)
    dsx, dss = torch.tensor(np.ascontiguousarray(sx.T), **f64), torch.tensor(np.ascontiguousarray(ss.T), **f64)
    rng = np.random.default_rng(17)
    for na in nas:
        sd = {k: torch.tensor(rng.standard_normal((B, na, n)), **f64)
              for k, n in (("x_bar", spec.nw), ("lam_g_bar", spec.ng), ("X_bar", spec.nX))}
        fo = {"pbar": torch.empty(B, na, spec.np, **f64), "q": torch.empty(B, na, spec.nw, **f64),
              "jq": torch.empty(B, na, spec.ng, **f64), "info": torch.empty(B, dtype=torch.int32, device="cuda"),
              "delta": torch.empty(B, **f64)}

        def fused():
            s.sensitivity_adjoint_device(sol, *db, dP, fo, **sd)

        fused()
        torch.cuda.synchronize()
        good = int((fo["info"] == 0).sum())
        delta = fo["delta"].clone()
        rungs = {float(v): int(c) for v, c in zip(*np.unique(delta.cpu().numpy(), return_counts=True))}
        wo = {"wbar": torch.empty(B, na, spec.nw, **f64)}
        ko = {"dw": torch.empty(B, na, spec.nw, **f64), "jdw": torch.empty(B, na, spec.ng, **f64),
              "info": torch.empty(B, dtype=torch.int32, device="cuda")}
        po = {"pbar": torch.empty(B, na, spec.np, **f64)}
        rg = dss[:, None, :] * sd["lam_g_bar"]

        def k1():
            s.adjoint_products_device(sol["x"], dP, wo, Xbar=sd["X_bar"], lam_g=sol["lam_g"])

        def k2():  # (wbar stands for x_bar + wbar: the same work)
            s.kkt_solve_device(sol["x"], dP, ko, r_w=wo["wbar"], r_g=rg, lam_g=sol["lam_g"], sigma_x=dsx, sigma_s=dss,
                               delta=delta)

        def k3():  # (jdw and dw stand for Sigma_s (lam_bar - J q) and -q: the same work)
            s.adjoint_products_device(sol["x"], dP, po, y=ko["jdw"], z=ko["dw"], Xbar=sd["X_bar"], lam_g=sol["lam_g"])

        def kernels():
            k1(); k2(); k3()

        def host():
            hs = {k: sol[k].cpu().numpy().T for k in ("x", "g", "lam_x", "lam_g")}
            seeds = {k: np.ascontiguousarray(v.cpu().numpy().transpose(2, 1, 0)) for k, v in sd.items()}
            r = s.sensitivity_adjoint(hs, *bounds, dP.cpu().numpy().T, **seeds)
            return torch.tensor(np.ascontiguousarray(r["pbar"].transpose(2, 1, 0)), **f64)

        med = {"fused": [], "kernels": [], "k1": [], "k2": [], "k3": [], "host": []}
        for rd in range(rounds):
            for leg, go in (("fused", fused), ("k1", k1), ("k2", k2), ("k3", k3), ("kernels", kernels)):
                r = timed(go, calls)
                med[leg].append(r["per_call_ms_median"])
                print(json.dumps({"leg": leg, "na": na, "round": rd, **shape, **r}), flush=True)
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
            print(json.dumps({"leg": "host", "na": na, "round": rd, **shape, "calls": host_calls,
                              "wall_ms_median": float(np.median(ms)), "wall_ms_min": float(np.min(ms)),
                              "wall_ms_max": float(np.max(ms))}), flush=True)
        assert bool((ko["info"] == 0).sum() == good)
        m = {k: float(np.median(v)) for k, v in med.items()}
        print(json.dumps({"leg": "summary", "na": na, **shape, "info_0": good, "delta_counts": rungs,
                          "median_ms": m, "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                          "three_kernels_sum_ms": m["k1"] + m["k2"] + m["k3"],
                          "fused_over_three_kernels_sum": m["fused"] / (m["k1"] + m["k2"] + m["k3"]),
                          "fused_over_sequence": m["fused"] / m["kernels"],
                          "host_over_fused": m["host"] / m["fused"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--na", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=10)
    a = ap.parse_args()
    main(a.points, a.calls, a.na, a.rounds, a.host_calls)
