"""Cost of the feedback policy of a solution at the config-3 shape (B = 4,096, N = 20, 10 obstacles;
the batch is solved first, so the points, multipliers and the delta ladder are real).  Legs, all in
one session, `--rounds` times in turn:
  policy:  one nmpc_solve_policy_batch_dev launch (Solver.policy_device into its own buffers) with
           nd = 0, 1, 3 and 8 directions: K, A, B, X (1,472 + 168 doubles per scenario) and kff out;
  tangent: one nmpc_solve_tangent_batch_dev launch (Solver.sensitivity_device) with nd = 1 and 8,
           for comparison: dx, dlam_g and dX out.

    python scripts/solve_policy_timing.py [--points 4096] [--calls 500] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream (median,
min, max reported), and the whole train by one more pair (mean, back to back).  Prints one JSON
line per leg and round, then one summary line with the medians over the rounds, their span and the
ratios to the tangent launch."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]

from scripts.products_timing import timed  # noqa: E402


def main(B, calls, rounds):
    import torch
    from nmpc_amd import config_spec, draw_scenarios, nlpsol, REFERENCE_OPTS

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    P = draw_scenarios(spec, B, seed=4096)
    db = [torch.tensor(np.asarray(v, dtype=np.float64), **f64) for v in spec.bounds()]
    dP = torch.tensor(P, **f64)
    sol = {"x": torch.empty(B, spec.nw, **f64), "g": torch.empty(B, spec.ng, **f64),
           "lam_x": torch.empty(B, spec.nw, **f64), "lam_g": torch.empty(B, spec.ng, **f64),
           "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    s.solve_device(torch.zeros(B, spec.nw, **f64), *db, dP, sol)
    torch.cuda.synchronize()
    ok = int(((sol["status"] == 0) | (sol["status"] == 1)).sum())
    shape = {"B": B, "N": spec.N, "n_obs": spec.n_obs, "np": spec.np, "converged": ok,
             "device": torch.cuda.get_device_name(0)}
    rng = np.random.default_rng(17)
    legs = []
    for nd in (0, 1, 3, 8):
        dd = torch.tensor(rng.standard_normal((B, nd, spec.np)), **f64) if nd else None
        raw = s.policy_device(sol, *db, dP, dd)["raw"]
        torch.cuda.synchronize()
        good = int((raw["info"] == 0).sum())
        legs.append((f"policy_nd{nd}", good, (lambda dd=dd, raw=raw: s.policy_device(sol, *db, dP, dd, out=raw))))
    for nd in (1, 8):
        dd = torch.tensor(rng.standard_normal((B, nd, spec.np)), **f64)
        fo = {"dx": torch.empty(B, nd, spec.nw, **f64), "dlam_g": torch.empty(B, nd, spec.ng, **f64),
              "dX": torch.empty(B, nd, spec.nX, **f64), "info": torch.empty(B, dtype=torch.int32, device="cuda"),
              "delta": torch.empty(B, **f64)}
        s.sensitivity_device(sol, *db, dP, dd, fo)
        torch.cuda.synchronize()
        good = int((fo["info"] == 0).sum())
        legs.append((f"tangent_nd{nd}", good, (lambda dd=dd, fo=fo: s.sensitivity_device(sol, *db, dP, dd, fo))))
    med = {name: [] for name, _, _ in legs}
    for rd in range(rounds):
        for name, good, go in legs:
            r = timed(go, calls)
            med[name].append(r["per_call_ms_median"])
            print(json.dumps({"leg": name, "round": rd, "info_0": good, **shape, **r}), flush=True)
    m = {k: float(np.median(v)) for k, v in med.items()}
    print(json.dumps({"leg": "summary", **shape, "median_ms": m,
                      "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                      "policy_over_tangent_nd1": m["policy_nd1"] / m["tangent_nd1"],
                      "policy_over_tangent_nd8": m["policy_nd8"] / m["tangent_nd8"]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.points, a.calls, a.rounds)
