"""Cost of the policy's closed-loop covariance at the config-3 shape (B = 4,096, N = 20, 10 obstacles;
the batch is solved first and its policy formed by Solver.policy_device, so the gains are real).
Legs, all in one session, `--rounds` times in turn:
  cov_nc1, cov_nc8: one nmpc_policy_covariance_batch_dev launch (Solver.policy_covariance_device into
                    its own buffers, sigma_g and sigma_u out) with 1 and 8 covariance cases;
  cov_nc1_full:     the same with Sigma_out too;
  torch:            what the launch replaces on the device -- N sequential batched torch products on
                    policy_device's A, B and K, Sigma' = Acl Sigma Acl' + W, with the row gradients, the
                    quadratic forms and the square roots (one case);
  rollout_M256:     the sampling route, one nmpc_policy_rollout_batch_dev launch with M = 256 (J, viol
                    and nsat out; the standard deviations would still have to be formed from X).

    python scripts/policy_covariance_timing.py [--points 4096] [--calls 200] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream (median,
min, max reported), and the whole train by one more pair (mean, back to back).  Prints one JSON
line per leg and round -- with the bytes the covariance launch must move (p, ubar, Xbar, K, S0, W and
the outputs) -- then one summary line with the medians over the rounds, their span and bytes per
second, and how far the sampled standard deviations of M = 256 unclamped rollouts (e0 ~ N(0, S0), w ~
N(0, W)) lie from sigma_g on the scenarios whose policy has info = 0."""
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


def main(B, calls, rounds):
    import torch
    from nmpc_amd import config_spec, draw_scenarios, nlpsol, REFERENCE_OPTS

    assert torch.cuda.is_available(), "this measurement needs a GPU"
    spec = config_spec(3)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    N, nx, nu = spec.N, spec.nX // (spec.N + 1), spec.nw // spec.N
    m, nobs = spec.ng // (N + 1), spec.n_obs
    nb = m - nobs
    f64 = dict(dtype=torch.float64, device="cuda")
    P = draw_scenarios(spec, B, seed=4096)
    db = [torch.tensor(np.asarray(v, dtype=np.float64), **f64) for v in spec.bounds()]
    dP = torch.tensor(P, **f64)
    sol = {"x": torch.empty(B, spec.nw, **f64), "g": torch.empty(B, spec.ng, **f64),
           "lam_x": torch.empty(B, spec.nw, **f64), "lam_g": torch.empty(B, spec.ng, **f64),
           "status": torch.empty(B, dtype=torch.int32, device="cuda")}
    s.solve_device(torch.zeros(B, spec.nw, **f64), *db, dP, sol)
    pol = s.policy_device(sol, *db, dP, None)
    raw = pol["raw"]
    torch.cuda.synchronize()
    ok = raw["info"] == 0
    shape = {"B": B, "N": N, "n_obs": nobs, "np": spec.np, "info_0": int(ok.sum()), "device": torch.cuda.get_device_name(0)}
    sg = torch.tensor(SIGMA[:nx], **f64)
    S1 = torch.diag(sg ** 2).expand(1, nx, nx).contiguous()       # shared by the scenarios (ld = 0)
    W1 = 0.01 * S1
    legs = []
    for name, nc, want in (("cov_nc1", 1, ("sigma_g", "sigma_u")), ("cov_nc8", 8, ("sigma_g", "sigma_u")),
                           ("cov_nc1_full", 1, ("sigma_g", "sigma_u", "Sigma"))):
        S0 = (S1 * torch.linspace(0.5, 2.0, nc, **f64).view(nc, 1, 1)).expand(B, nc, nx, nx).contiguous()
        W = 0.01 * S0
        out = s.policy_covariance_device(dP, sol["x"], raw["X"], raw["K"], S0, W=W, want=want)
        torch.cuda.synchronize()
        moved = 8 * B * (spec.np + spec.nw + spec.nX + nu * nx * N) + 8 * (S0.numel() + W.numel()) \
            + sum(t.numel() * 8 for t in out.values())
        legs.append((name, {"nc": nc, "bytes": moved, "finite": float(torch.isfinite(out["sigma_g"][ok]).double().mean())},
                     (lambda S0=S0, W=W, out=out: s.policy_covariance_device(dP, sol["x"], raw["X"], raw["K"], S0, W=W,
                                                                             out=out, want=()))))

    # route (i): torch on policy_device's A, B, K (views of the column-major blocks: (B, N, n, n) matrices)
    A, Bm, K, X = pol["A"], pol["B"], pol["K"], pol["X"]
    ox = torch.tensor([o.x for o in spec.obstacles], **f64)
    oy = torch.tensor([o.y for o in spec.obstacles], **f64)
    box = [2, 3, 5, 6, 7][:nb]
    S0t, Wt = S1.expand(B, nx, nx), W1.expand(B, nx, nx)

    def torch_route():
        S = S0t
        sig_g, sig_u = [], []
        for k in range(N + 1):
            dx, dy = X[:, k, 0:1] - ox, X[:, k, 1:2] - oy
            d = torch.sqrt(dx * dx + dy * dy)
            g = torch.stack([-dx / d, -dy / d], dim=-1)                      # (B, nobs, 2)
            vo = torch.einsum("boi,bij,boj->bo", g, S[:, :2, :2], g)
            sig_g.append(torch.sqrt(torch.clamp(torch.cat([S[:, box, box], vo], dim=1), min=0.0)))
            if k == N:
                break
            Kk = K[:, k]
            sig_u.append(torch.sqrt(torch.clamp(torch.einsum("bri,bij,brj->br", Kk, S, Kk), min=0.0)))
            Acl = A[:, k] + Bm[:, k] @ Kk
            S = Acl @ S @ Acl.transpose(1, 2) + Wt
        return torch.stack(sig_g, dim=1), torch.stack(sig_u, dim=1)

    tg, tu = torch_route()
    ref = s.policy_covariance_device(dP, sol["x"], raw["X"], raw["K"], S1, W=W1, want=("sigma_g", "sigma_u"))
    torch.cuda.synchronize()
    dg = float((tg[ok] - ref["sigma_g"][ok, 0]).abs().max() / ref["sigma_g"][ok, 0].abs().max())
    du = float((tu[ok] - ref["sigma_u"][ok, 0]).abs().max() / ref["sigma_u"][ok, 0].abs().max())
    legs.append(("torch", {"nc": 1, "against_kernel_sigma_g": dg, "against_kernel_sigma_u": du}, torch_route))

    # route (ii): M = 256 rollouts, e0 ~ N(0, S0) and w ~ N(0, W), unclamped
    M = 256
    gen = torch.Generator(device="cuda").manual_seed(17)
    e0 = torch.randn(B, M, nx, generator=gen, **f64) * sg
    w = 0.1 * torch.randn(B, M, N, nx, generator=gen, **f64) * sg
    out = s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w, lbg=db[2], ubg=db[3], want=("J", "viol", "nsat"))
    legs.append(("rollout_M256", {"M": M}, (lambda out=out: s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w,
                                                                                     lbg=db[2], ubg=db[3], out=out, want=()))))
    # the sampled standard deviations of the rows against sigma_g (in chunks of scenarios: X is large)
    worst, typ = 0.0, []
    for a in range(0, B, 512):
        sl = slice(a, min(a + 512, B))
        Xs = s.policy_rollout_device(dP[sl], sol["x"][sl], raw["X"][sl], raw["K"][sl], e0[sl], w=w[sl], want=("X",))["X"]
        dx, dy = Xs[..., 0:1] - ox, Xs[..., 1:2] - oy
        rows = torch.cat([Xs[..., box], -torch.sqrt(dx * dx + dy * dy)], dim=-1)  # (b, M, N + 1, m), up to the radii
        sd = rows.std(dim=1)
        rg = ref["sigma_g"][sl, 0]
        rel = ((sd - rg).abs() / rg.clamp(min=1e-300))[ok[sl]][:, 1:]
        worst = max(worst, float(rel.max()))
        typ.append(rel.flatten())
    typ = torch.cat(typ)
    sampled = {"M": M, "rel_dev_median": float(typ.median()), "rel_dev_p99": float(typ.quantile(0.99)) if typ.numel() < 1.6e7
               else float(typ[:: max(1, typ.numel() // 1000000)].quantile(0.99)), "rel_dev_max": worst,
               "expected_1_over_sqrt_2M": float(1.0 / np.sqrt(2.0 * M))}
    torch.cuda.synchronize()

    med = {name: [] for name, _, _ in legs}
    for rd in range(rounds):
        for name, info, go in legs:
            r = timed(go, calls)
            med[name].append(r["per_call_ms_median"])
            print(json.dumps({"leg": name, "round": rd, **info, **shape, **r}), flush=True)
    mm = {k: float(np.median(v)) for k, v in med.items()}
    info = {name: i for name, i, _ in legs}
    print(json.dumps({"leg": "summary", **shape, "median_ms": mm,
                      "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                      "bytes": {k: info[k]["bytes"] for k in mm if "bytes" in info[k]},
                      "bytes_per_s": {k: info[k]["bytes"] / (mm[k] * 1e-3) for k in mm if "bytes" in info[k]},
                      "torch_against_kernel": {"sigma_g": dg, "sigma_u": du},
                      "sampled_against_sigma_g": sampled}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.points, a.calls, a.rounds)
