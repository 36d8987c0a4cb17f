"""Cost of the policy rollouts' reverse sweep at the config-3 shape (B = 4,096, N = 20, 10 obstacles;
the batch is solved first and its policy formed by Solver.policy_device, so the gains are real).
Legs, all in one session, alternating, `--rounds` times in turn, with M = 1, 64 and 256 samples per
scenario, e0 ~ N(0, diag sigma^2) and w a tenth of that, clamped at the control bounds:
  forward: one nmpc_policy_rollout_batch_dev launch with J, nsat, X_out and U_out (the launch whose
           X the reverse sweep reads; no rows);
  reduced: one nmpc_policy_rollout_adjoint_batch_dev launch, seeds Jb, Xb, Ub, outputs ubar_bar, K_bar,
           Xbar_bar and p_bar (at M > 64 the partial sums' second kernel included);
  all:     e0_bar, w_bar and nsat too.

    python scripts/policy_rollout_adjoint_timing.py [--points 4096] [--calls 500] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream (median,
min, max reported), and the whole train by one more pair (mean, back to back).  Prints one JSON line
per leg and round -- with the bytes the launch must move (X, the seeds and the per-sample outputs; the
scenario's p, plan, gains, bounds and reduced outputs once per scenario) -- then one summary line with
the medians over the rounds, their span, the ratio to the forward launch, bytes per second, and what
central differences through the forward launch would cost for the scalars of (ubar, K, p): two launches
each."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]

from scripts.products_timing import timed  # noqa: E402

SIGMA = (0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02)
REDUCED = ("ubar_bar", "K_bar", "Xbar_bar", "p_bar")


def main(B, calls, rounds, samples):
    import torch
    from nmpc_amd import config_spec, draw_scenarios, nlpsol, REFERENCE_OPTS

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    N, nx, nu = spec.N, spec.nX // (spec.N + 1), spec.nw // spec.N
    f64 = dict(dtype=torch.float64, device="cuda")
    P = draw_scenarios(spec, B, seed=4096)
    db = [torch.tensor(np.asarray(v, dtype=np.float64), **f64) for v in spec.bounds()]
    dP = torch.tensor(P, **f64)
    sol = {"x": torch.empty(B, spec.nw, **f64), "g": torch.empty(B, spec.ng, **f64),
           "lam_x": torch.empty(B, spec.nw, **f64), "lam_g": torch.empty(B, spec.ng, **f64),
           "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    s.solve_device(torch.zeros(B, spec.nw, **f64), *db, dP, sol)
    raw = s.policy_device(sol, *db, dP, None)["raw"]
    torch.cuda.synchronize()
    n_scalars = spec.nw + nu * nx * N + spec.np
    shape = {"B": B, "N": N, "n_obs": spec.n_obs, "np": spec.np, "info_0": int((raw["info"] == 0).sum()),
             "scalars_ubar_K_p": n_scalars, "device": torch.cuda.get_device_name(0)}
    per_scenario = 8 * (spec.np + spec.nw + spec.nX + nu * nx * N + 2 * spec.nw)
    sg = torch.tensor(SIGMA[:nx], **f64)
    gen = torch.Generator(device="cuda").manual_seed(17)
    legs = []
    for M in samples:
        e0 = torch.randn(B, M, nx, generator=gen, **f64) * sg
        w = 0.1 * torch.randn(B, M, N, nx, generator=gen, **f64) * sg
        fwd = s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w, lbx=db[0], ubx=db[1],
                                      want=("J", "nsat", "X", "U"))
        seeds = {"Jb": torch.randn(B, M, generator=gen, **f64), "Xb": torch.randn(B, M, N + 1, nx, generator=gen, **f64),
                 "Ub": torch.randn(B, M, N, nu, generator=gen, **f64)}
        torch.cuda.synchronize()
        moved = B * per_scenario + e0.numel() * 8 + w.numel() * 8 + sum(t.numel() * t.element_size() for t in fwd.values())
        legs.append((f"forward_M{M}", {"M": M, "bytes": moved, "mean_nsat": float(fwd["nsat"].double().mean())},
                     (lambda e0=e0, w=w, fwd=fwd: s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w, lbx=db[0],
                                                                          ubx=db[1], out=fwd, want=()))))
        for name, want in (("reduced", REDUCED), ("all", REDUCED + ("e0_bar", "w_bar", "nsat"))):
            out = s.policy_rollout_adjoint_device(dP, sol["x"], raw["X"], raw["K"], fwd["X"], lbx=db[0], ubx=db[1], want=want,
                                                  **seeds)
            torch.cuda.synchronize()
            moved = (B * per_scenario + fwd["X"].numel() * 8 + sum(t.numel() * 8 for t in seeds.values())
                     + sum(t.numel() * t.element_size() for t in out.values()))
            info = {"M": M, "bytes": moved, "finite": float(torch.isfinite(out["ubar_bar"]).double().mean())}
            legs.append((f"{name}_M{M}", info,
                         (lambda fwd=fwd, seeds=seeds, out=out: s.policy_rollout_adjoint_device(
                             dP, sol["x"], raw["X"], raw["K"], fwd["X"], lbx=db[0], ubx=db[1], out=out, want=(), **seeds))))
    med = {name: [] for name, _, _ in legs}
    for rd in range(rounds):
        for name, info, go in legs:
            r = timed(go, calls)
            med[name].append(r["per_call_ms_median"])
            print(json.dumps({"leg": name, "round": rd, **info, **shape, **r}), flush=True)
    m = {k: float(np.median(v)) for k, v in med.items()}
    info = {name: i for name, i, _ in legs}
    print(json.dumps({"leg": "summary", **shape, "median_ms": m,
                      "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                      "ratio_to_forward": {k: m[k] / m[f"forward_M{info[k]['M']}"] for k in m if not k.startswith("forward")},
                      "bytes": {k: info[k]["bytes"] for k in m},
                      "bytes_per_s": {k: info[k]["bytes"] / (m[k] * 1e-3) for k in m},
                      "central_differences_ms": {k: 2 * n_scalars * m[k] for k in m if k.startswith("forward")}}),
          flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, nargs="+", default=[1, 64, 256])
    a = ap.parse_args()
    main(a.points, a.calls, a.rounds, a.samples)
