"""Cost of the policy's cost-to-go expansion at the config-3 shape (B = 4,096, N = 20, 10 obstacles; the
batch is solved first and its policy formed by Solver.policy_device, so the gains are real).
Legs, all in one session, `--rounds` times in turn:
  value_nc1, value_nc8: one nmpc_policy_value_batch_dev launch (Solver.policy_value_device into its own
                        buffers, J, dJ and varJ out) with 1 and 8 covariance cases;
  value_nc1_P:          the same with P_out too;
  torch:                the recursion's products on the device -- N sequential batched torch products on
                        policy_device's A, B and K, Acl = A + B K, lam = g + Acl' lam, P = M + Acl' P Acl,
                        then the two inner products (one case).  g_k and M_k are GIVEN to this leg
                        (recovered from the launch's lam and P): torch has no stage-cost Hessian and no
                        dynamics curvature, so the leg is a lower bound of the route it stands for;
  rollout_M256:         the sampling route, one nmpc_policy_rollout_batch_dev launch with M = 256 whose
                        sample mean of J estimates J + dJ.

    python scripts/policy_value_timing.py [--points 4096] [--calls 200] [--rounds 3]   # needs an MI355X

After 20 warm-up calls every call is bracketed by its own pair of HIP events on the stream (median,
min, max reported), and the whole train by one more pair (mean, back to back).  Prints one JSON line
per leg and round -- with the bytes the launch must move (p, ubar, Xbar, K, S0, W and the outputs) --
then one summary line with the medians over the rounds, their span and bytes per second, and how far
the mean of J over M = 256 unclamped rollouts (e0 ~ N(0, S0), w ~ N(0, W)) lies from J + dJ in units of
J's sampled standard error, on the scenarios whose policy has info = 0."""
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
    shape = {"B": B, "N": N, "n_obs": spec.n_obs, "np": spec.np, "info_0": int(ok.sum()), "device": torch.cuda.get_device_name(0)}
    sg = torch.tensor(SIGMA[:nx], **f64)
    S1 = torch.diag(sg ** 2).expand(1, nx, nx).contiguous()       # shared by the scenarios (ld = 0)
    W1 = 0.01 * S1
    legs = []
    for name, nc, want in (("value_nc1", 1, ("J", "dJ", "varJ")), ("value_nc8", 8, ("J", "dJ", "varJ")),
                           ("value_nc1_P", 1, ("J", "dJ", "varJ", "P"))):
        S0 = (S1 * torch.linspace(0.5, 2.0, nc, **f64).view(nc, 1, 1)).expand(B, nc, nx, nx).contiguous()
        W = 0.01 * S0
        out = s.policy_value_device(dP, sol["x"], raw["X"], raw["K"], S0=S0, W=W, want=want)
        torch.cuda.synchronize()
        moved = 8 * B * (spec.np + spec.nw + spec.nX + nu * nx * N) + 8 * (S0.numel() + W.numel()) \
            + sum(t.numel() * 8 for t in out.values())
        legs.append((name, {"nc": nc, "bytes": moved, "finite": float(torch.isfinite(out["dJ"][ok]).double().mean())},
                     (lambda S0=S0, W=W, out=out: s.policy_value_device(dP, sol["x"], raw["X"], raw["K"], S0=S0, W=W, out=out,
                                                                        want=()))))

    # the torch route on policy_device's A, B, K (views of the column-major blocks: (B, N, n, n) matrices)
    ref = s.policy_value_device(dP, sol["x"], raw["X"], raw["K"], S0=S1, W=W1, want=("J", "lam", "P", "dJ", "varJ"))
    torch.cuda.synchronize()
    A, Bm, K = pol["A"], pol["B"], pol["K"]
    Acl0 = A + Bm @ K
    Mk = ref["P"][:, :-1] - Acl0.transpose(2, 3) @ ref["P"][:, 1:] @ Acl0          # given to the leg
    gk = ref["lam"][:, :-1] - (Acl0.transpose(2, 3) @ ref["lam"][:, 1:, :, None])[..., 0]
    S0t, Wt = S1[0].expand(B, nx, nx), W1[0].expand(B, nx, nx)

    def torch_route():
        lam = torch.zeros(B, nx, **f64)
        Pk = torch.zeros(B, nx, nx, **f64)
        Ps, Ls = torch.zeros(B, nx, nx, **f64), torch.zeros(B, nx, nx, **f64)
        for k in range(N - 1, -1, -1):
            Ps, Ls = Ps + Pk, Ls + lam[:, :, None] * lam[:, None, :]
            Acl = A[:, k] + Bm[:, k] @ K[:, k]
            At = Acl.transpose(1, 2)
            lam = gk[:, k] + (At @ lam[:, :, None])[..., 0]
            Pk = Mk[:, k] + At @ Pk @ Acl
        dJ = 0.5 * ((Pk * S0t).sum(dim=(1, 2)) + (Ps * Wt).sum(dim=(1, 2)))
        var = torch.einsum("bi,bij,bj->b", lam, S0t, lam) + (Ls * Wt).sum(dim=(1, 2))
        return dJ, var

    tdJ, tvar = torch_route()
    torch.cuda.synchronize()
    dd = float((tdJ[ok] - ref["dJ"][ok, 0]).abs().max() / ref["dJ"][ok, 0].abs().max())
    dv = float((tvar[ok] - ref["varJ"][ok, 0]).abs().max() / ref["varJ"][ok, 0].abs().max())
    legs.append(("torch", {"nc": 1, "against_kernel_dJ": dd, "against_kernel_varJ": dv}, torch_route))

    # the sampling route: M = 256 rollouts, e0 ~ N(0, S0) and w ~ N(0, W), unclamped, no rows
    M = 256
    gen = torch.Generator(device="cuda").manual_seed(17)
    e0 = torch.randn(B, M, nx, generator=gen, **f64) * sg
    w = 0.1 * torch.randn(B, M, N, nx, generator=gen, **f64) * sg
    out = s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w, want=("J",))
    torch.cuda.synchronize()
    legs.append(("rollout_M256", {"M": M}, (lambda out=out: s.policy_rollout_device(dP, sol["x"], raw["X"], raw["K"], e0, w=w,
                                                                                     out=out, want=()))))
    Js = out["J"][ok]
    EJ = (ref["J"] + ref["dJ"][:, 0])[ok]
    se = Js.std(dim=1) / np.sqrt(M)
    z = (Js.mean(dim=1) - EJ) / se
    z0 = (Js.mean(dim=1) - ref["J"][ok]) / se                     # the same against the plan's cost alone
    sampled = {"M": M, "z_mean": float(z.mean()), "z_rms": float((z * z).mean().sqrt()), "z_abs_median": float(z.abs().median()),
               "z_abs_max": float(z.abs().max()), "z_against_J_alone_mean": float(z0.mean()),
               "z_against_J_alone_rms": float((z0 * z0).mean().sqrt()),
               "z_abs_p99": float(z.abs().quantile(0.99)), "share_abs_z_above_3": float((z.abs() > 3.0).double().mean()),
               "share_abs_z_above_3_against_J_alone": float((z0.abs() > 3.0).double().mean()),
               "worst": {k: float(v[z.abs().argmax()]) for k, v in (("J", ref["J"][ok]), ("dJ", ref["dJ"][ok, 0]),
                                                                    ("sampled_mean", Js.mean(dim=1)), ("standard_error", se))},
               "dJ_over_standard_error_median": float((ref["dJ"][ok, 0] / se).median()),
               "sqrt_varJ_over_sampled_std_median": float((ref["varJ"][ok, 0].sqrt() / Js.std(dim=1)).median())}

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
                      "torch_against_kernel": {"dJ": dd, "varJ": dv},
                      "sampled_mean_against_J_plus_dJ": sampled}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    main(a.points, a.calls, a.rounds)
