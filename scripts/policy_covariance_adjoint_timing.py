"""Cost of the reverse sweep of the policy's covariance at the config-3 shape (B = 4,096, N = 20, 10
obstacles; the batch is solved first and its policy formed by Solver.policy_device, so the gains are
real).  Legs, all in one session, `--rounds` times in turn:
  fwd_nc1, fwd_nc8:   one nmpc_policy_covariance_batch_dev launch with Sigma, sigma_u and sigma_g out
                      (what the reverse sweep needs), 1 and 8 covariance cases;
  adj_nc1, adj_nc8:   one nmpc_policy_covariance_adjoint_batch_dev launch with every output;
  adj_nc1_S0K, adj_nc8_S0K: the same with S0_bar_out and K_bar_out alone;
  torch_fwd_bwd:      torch.autograd through the N sequential batched torch products on policy_device's
                      A, B and K (one case): forward and backward of the sum of the deviations.  It
                      reaches K, S0 and W only -- A and B are constants there, so it gives no gradient
                      with respect to the plan or p.

    python scripts/policy_covariance_adjoint_timing.py [--points 4096] [--calls 200] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream (median,
min, max reported), and the whole train by one more pair (mean, back to back).  Prints one JSON line
per leg and round, then one summary line with the medians over the rounds and their span, and how far
the kernel's K_bar and S0_bar lie from torch.autograd's on the scenarios whose policy has info = 0."""
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
    from nmpc_amd import config_spec, draw_scenarios, nlpsol, policy, REFERENCE_OPTS

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
    S1 = torch.diag(sg ** 2).expand(1, nx, nx).contiguous()
    legs, kept = [], {}
    for nc in (1, 8):
        S0 = (S1 * torch.linspace(0.5, 2.0, nc, **f64).view(nc, 1, 1)).expand(B, nc, nx, nx).contiguous()
        W = 0.01 * S0
        fwd = s.policy_covariance_device(dP, sol["x"], raw["X"], raw["K"], S0, W=W, want=("Sigma", "sigma_u", "sigma_g"))
        torch.cuda.synchronize()
        # the seeds of the loss sum(sigma_u) + sum(sigma_g), on the variances
        vu = policy.var_seed(fwd["sigma_u"], torch.ones_like(fwd["sigma_u"])).contiguous()
        vg = policy.var_seed(fwd["sigma_g"], torch.ones_like(fwd["sigma_g"])).contiguous()
        legs.append((f"fwd_nc{nc}", {"nc": nc}, (lambda S0=S0, W=W, fwd=fwd: s.policy_covariance_device(
            dP, sol["x"], raw["X"], raw["K"], S0, W=W, out=fwd, want=()))))
        for tag, want in (("", s.COVARIANCE_ADJ_OUT), ("_S0K", ("S0_bar", "K_bar"))):
            out = s.policy_covariance_adjoint_device(dP, sol["x"], raw["X"], raw["K"], fwd["Sigma"], var_u_bar=vu, var_g_bar=vg,
                                                     want=want)
            torch.cuda.synchronize()
            kept[f"adj_nc{nc}{tag}"] = out
            legs.append((f"adj_nc{nc}{tag}", {"nc": nc, "finite": float(torch.isfinite(out["S0_bar"][ok]).double().mean())},
                         (lambda fwd=fwd, vu=vu, vg=vg, out=out: s.policy_covariance_adjoint_device(
                             dP, sol["x"], raw["X"], raw["K"], fwd["Sigma"], var_u_bar=vu, var_g_bar=vg, out=out, want=()))))

    # torch.autograd through the sequential products on policy_device's A, B, K (one case)
    A, Bm, X = pol["A"], pol["B"], pol["X"]
    ox = torch.tensor([o.x for o in spec.obstacles], **f64)
    oy = torch.tensor([o.y for o in spec.obstacles], **f64)
    box = [2, 3, 5, 6, 7][:nb]
    S0c = (S1 * 0.5).expand(B, nx, nx).contiguous()  # case 0 of the legs above

    def root(v):  # sqrt(max(v, 0)) whose gradient is 0, not inf or NaN, where v <= 0 (policy.var_seed's rule)
        pos = v > 0
        return torch.where(pos, torch.sqrt(torch.where(pos, v, torch.ones_like(v))), torch.zeros_like(v))

    def torch_loss(K, S0t, Wt):
        S, tot = S0t, 0.0
        for k in range(N + 1):
            dx, dy = X[:, k, 0:1] - ox, X[:, k, 1:2] - oy
            d = torch.sqrt(dx * dx + dy * dy)
            g = torch.stack([-dx / d, -dy / d], dim=-1)
            vo = torch.einsum("boi,bij,boj->bo", g, S[:, :2, :2], g)
            tot = tot + root(torch.cat([S[:, box, box], vo], dim=1)).sum()
            if k == N:
                break
            Kk = K[:, k]
            tot = tot + root(torch.einsum("bri,bij,brj->br", Kk, S, Kk)).sum()
            Acl = A[:, k] + Bm[:, k] @ Kk
            S = Acl @ S @ Acl.transpose(1, 2) + Wt
        return tot

    def torch_route():
        K = pol["K"].detach().clone().requires_grad_(True)
        S0t = S0c.clone().requires_grad_(True)
        Wt = (0.01 * S0c).clone().requires_grad_(True)
        return torch.autograd.grad(torch_loss(K, S0t, Wt), [K, S0t, Wt])

    gK, gS, _ = torch_route()
    torch.cuda.synchronize()
    mine = kept["adj_nc1_S0K"]
    kb = mine["K_bar"][:, 0].transpose(-1, -2)  # to (B, N, nu, nx)
    dK = float((gK[ok] - kb[ok]).abs().max() / kb[ok].abs().max())
    sb = mine["S0_bar"][:, 0]
    dS = float((0.5 * (gS + gS.transpose(1, 2))[ok] - sb[ok]).abs().max() / sb[ok].abs().max())
    legs.append(("torch_fwd_bwd", {"nc": 1, "against_kernel_K_bar": dK, "against_kernel_S0_bar": dS}, torch_route))

    med = {name: [] for name, _, _ in legs}
    for rd in range(rounds):
        for name, info, go in legs:
            r = timed(go, calls)
            med[name].append(r["per_call_ms_median"])
            print(json.dumps({"leg": name, "round": rd, **info, **shape, **r}), flush=True)
    mm = {k: float(np.median(v)) for k, v in med.items()}
    print(json.dumps({"leg": "summary", **shape, "median_ms": mm,
                      "span_ms": {k: [float(min(v)), float(max(v))] for k, v in med.items()},
                      "torch_against_kernel": {"K_bar": dK, "S0_bar": dS}}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.points, a.calls, a.rounds)
