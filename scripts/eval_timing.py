"""Cost of one nmpc_eval_batch_dev call at the config-3 shape (B = 4,096, N = 20, 10 obstacles,
all six outputs, multipliers and bounds given), and of the numpy certificate loop
(oracle.SSEval + the five KKT numbers, tests/eval_ref.py) over the same points.

    python scripts/eval_timing.py --gpu [--calls 200]    # needs an MI355X
    python scripts/eval_timing.py --cpu [--points 4096]  # numpy loop, no GPU needed

GPU: after 20 warm-up calls every call is bracketed by its own pair of HIP events on the
stream (median, min, max reported), and the whole train of calls by one more pair (mean per
call, back to back).  Prints one JSON line per leg."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mpc-implementation_amd")]


def points(B):
    from nmpc_amd import config_spec
    from tests import eval_ref as er

    spec = config_spec(3)
    return spec, er.draw_point(spec, B, seed=4096)


def gpu_leg(B, calls):
    import torch
    from nmpc_amd import nlpsol, REFERENCE_OPTS

    assert torch.cuda.is_available(), "the GPU leg needs a GPU"
    spec, d = points(B)
    s = nlpsol("solver", "ipopt", spec, REFERENCE_OPTS)
    f64 = dict(dtype=torch.float64, device="cuda")
    dev = {k: torch.tensor(np.ascontiguousarray(d[k]), **f64) for k in d}
    out = {"f": torch.empty(B, **f64), "g": torch.empty(B, spec.ng, **f64), "X": torch.empty(B, spec.nX, **f64),
           "grad_f": torch.empty(B, spec.nw, **f64), "grad_l": torch.empty(B, spec.nw, **f64),
           "kkt": torch.empty(B, 5, **f64)}

    def go():
        s.evaluate_device(dev["w"], dev["p"], out, lam_g=dev["lam_g"], lam_x=dev["lam_x"], lbx=dev["lbx"],
                          ubx=dev["ubx"], lbg=dev["lbg"], ubg=dev["ubg"])

    for _ in range(20):
        go()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        go()
        b.record()
    torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        go()
    t1.record()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(v).all()) for v in out.values())
    print(json.dumps({"leg": "gpu", "B": B, "N": spec.N, "n_obs": spec.n_obs, "calls": calls,
                      "per_call_ms_median": float(np.median(ms)), "per_call_ms_min": float(ms.min()),
                      "per_call_ms_max": float(ms.max()), "train_ms_per_call": t0.elapsed_time(t1) / calls,
                      "device": torch.cuda.get_device_name(0)}))


def cpu_leg(B):
    from tests import eval_ref as er

    spec, d = points(B)
    prob = er.problem_of(spec)
    t0 = time.perf_counter()
    for b in range(B):
        er.cpu_eval(prob, d["w"][b], d["p"][b], d["lam_g"][b], d["lam_x"][b], d["lbx"], d["ubx"], d["lbg"], d["ubg"])
    dt = time.perf_counter() - t0
    print(json.dumps({"leg": "cpu_numpy", "points": B, "N": spec.N, "n_obs": spec.n_obs, "seconds": dt,
                      "ms_per_point": 1e3 * dt / B}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=200)
    a = ap.parse_args()
    if a.gpu:
        gpu_leg(a.points, a.calls)
    if a.cpu:
        cpu_leg(a.points)
