"""Rounding spread of the oracle's first iterations (test infrastructure only; oracle-only,
nothing here comes from the kernel).

For every case of tests/trace_cases.py (one problem shape per fp64 kernel class / model, two
scenarios, cold start at zero) the oracle runs with max_iter = 8 and trace=True.  Stored in
tests/golden/trace_spread.npz, per case and scenario (the deviations per case: the larger of
its two scenarios'):

  rows, chk   the plain oracle's trace rows (iter, mu, f, theta, delta_w, alpha_pr, alpha_du,
              ls_trials: the kernel's column order) and convergence-check quantities
              (err, dinf / s_d, cviol, cmp / s_c at iteration counts 0..8, IpoptDense.chk);
  dev_abs,    per field, the largest absolute / relative deviation of the rounding variants
  dev_rel     (trace_cases.VARIANTS: la_variant 1..3, the same Newton step from permuted
              Cholesky factorisations, and the objective from the literal stage-cost form
              summed in reverse order: rounding alone) from the plain oracle -- absolute
              over the values below 1e-6 of theta and the check fields, relative over all
              others;
  lead        the number of leading iterations on which every variant takes the plain
              oracle's line-search trial counts (all in the main phase).

tests/test_gpu_trace.py holds the kernel's trace to 30 x these deviations (mu, delta_w and f
to fixed relative figures, trace_cases.FIXED_REL);
tests/test_oracle.py checks that a 1e-7 error in the oracle's gradient, one obstacle row or
Newton step fails that comparison by 10 x and more.

A second fixture, tests/golden/trace_spread_fp32.npz, holds the same layout's lead, dev_abs and
dev_rel for the fp32 leg on trace_cases.GATED: the deviation of the refined float32 variants
(trace_cases.FP32_VARIANTS: a float32 Cholesky factor with one fp64 refinement step under the
identity and the three permutations, also with the literal objective) from the plain fp64
oracle, and the leading iterations on which all of them take its iteration and trial counts.

    python tests/golden/gen_trace_spread.py [--check] [--jobs 8] [--only fp64|fp32]
        (--check: regenerate both and compare with the committed files instead of writing them)
"""
import argparse
import multiprocessing as mp
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "mpc-implementation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import trace_cases as tc  # noqa: E402


def job(args):
    name, b = args
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except ImportError:
        pass
    case = tc.build_case(name)
    plain = tc.oracle_trace(case, b)
    variants = [tc.oracle_trace(case, b, v)[:2] for v in tc.VARIANTS]
    lead, dev_abs, dev_rel = tc.spread(plain[:2], variants)
    return name, b, dict(rows=plain[0], chk=plain[1], status=np.int32(plain[2]), lead=np.int32(lead),
                         dev_abs=dev_abs, dev_rel=dev_rel)


def job32(args):
    """The fp32 fixture's part of one (case, scenario): the refined float32 variants against the
    plain fp64 oracle."""
    name, b = args
    try:
        from threadpoolctl import threadpool_limits
        threadpool_limits(1)
    except ImportError:
        pass
    case = tc.build_case(name)
    plain = tc.oracle_trace(case, b)
    variants = [tc.oracle_trace(case, b, v)[:2] for v in tc.FP32_VARIANTS]
    lead, dev_abs, dev_rel = tc.spread(plain[:2], variants)
    return name, b, dict(lead=np.int32(lead), dev_abs=dev_abs, dev_rel=dev_rel)


def generate(jobs, fp32=False):
    todo = [(n, b) for n in (tc.GATED if fp32 else tc.CASES) for b in (0, 1)]
    out = {"fields": np.array(tc.FIELDS)}
    with mp.get_context("fork").Pool(jobs) as pool:
        for name, b, r in pool.imap_unordered(job32 if fp32 else job, todo):
            for k, v in r.items():
                if k.startswith("dev_"):  # per case: the larger of the two scenarios'
                    out[f"{name}__{k}"] = np.maximum(out.get(f"{name}__{k}", 0.0), v)
                else:
                    out[f"{name}__{b}__{k}"] = v
            print(f"{name}/{b}{' fp32' if fp32 else ''}: lead {int(r['lead'])}, largest relative deviation "
                  + ", ".join(f"{f} {r['dev_rel'][i]:.1e}" for i, f in enumerate(tc.FIELDS)), flush=True)
    return dict(sorted(out.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--only", choices=("fp64", "fp32"), help="one of the two fixtures (default: both)")
    a = ap.parse_args()
    rc = 0
    for path, fp32 in ((tc.FIXTURE, False), (tc.FIXTURE_FP32, True)):
        if a.only and a.only != ("fp32" if fp32 else "fp64"):
            continue
        out = generate(a.jobs, fp32)
        if a.check:
            old = np.load(path)
            assert sorted(old.files) == sorted(out), "key sets differ"
            bad = [k for k in out if not np.array_equal(old[k], out[k], equal_nan=k.endswith(("rows", "chk")))]
            print(f"{os.path.basename(path)}: " + ("fixture reproduced bit for bit" if not bad else f"DIFFERENT: {bad}"))
            rc |= 1 if bad else 0
        else:
            np.savez_compressed(path, **out)
            print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    sys.exit(rc)


if __name__ == "__main__":
    main()
