"""The policy-rollout adjoint entry points without a GPU: exported, declared, a NULL handle refused
before any device call, the kernel part of the evaluation unit with its source under the build hash --
and the checker of tests/test_gpu_policy_rollout_adjoint.py (tests/rollout_adjoint_ref.py) shown to
pass its own gate on the oracle alone, with every mutant missing it on every scenario where it can act.

The gate: on the 13 solved scenarios, with the dense-oracle policy of tests/policy_ref.py, the clamp
box of rollout_ref.widen and four samples (sample 0 undisturbed, samples 1 and 2 scaled by 20, sample 3
at its ordinary size), random seeds Jb, Xb, Ub and a random joint direction d over (p[x0, target,
weight entries], ubar, Xbar, K, e0, w), the K part scaled by max |K|: per sample the central
difference of Jb J + <Xb, X> + <Ub, U> through rollout_ref.rollout_one at step H must agree with
<gradient, d> to within BOUND x sum_i |g_i| |d_i|.

The bound: the difference's rounding error is about eps |L| / H = 2e-7 relative at H = 5e-7 with
|L| ~ 1e3 and a derivative of the same order, truncation (H^2) far below it; BOUND = 1e-5 leaves a
factor of 20 to 50 over that.  A condition, not a tolerance: the clamp's derivative is a step, so both
difference points must have the base point's set of clamped entries, asserted from the checker's U and
the box before comparing (at H = 1e-6 some samples flip a clamp decision and the difference is off by
up to 590 %).  Each scenario must show a sample with nsat > 0 and one with nsat = 0.

The measured figures are printed wherever the suite runs."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import policy_ref as pf
from tests import rollout_adjoint_ref as ra
from tests import rollout_ref as rr
from tests import solve_adjoint_ref as sr

NAMES = ("nmpc_policy_rollout_adjoint_batch", "nmpc_policy_rollout_adjoint_batch_dev")
SIGMA = (0.5, 0.5, 0.5, 0.02, 0.02, 0.02, 0.02, 0.02)
SCALE = 20.0
M = 4
# disturbance seed, chosen on the oracle alone: the first of 500, 400, 12, 700, 800 ... 2700 (steps of 100) at
# which all 52 samples keep their clamp sets under the difference step and the difference can be trusted (the
# central differences at H and H / 2 agree to 1e-6 of the scale).  The K part of d is scaled by max |K|, up to
# ~1e4 at the last stages, so a saturating sample's u_raw moves by up to ~1e-2 under the step: most seeds flip a
# clamp on one of the 52 samples.  Seed 1100 keeps every set and still misses the bound on one sample (dynamic,
# scenario 0, sample 1: 3.09e-5 of the scale); that is the step's truncation, not the checker: at H, H / 2,
# H / 4, H / 8 the figure is 3.09e-5, 7.73e-6, 1.93e-6, 4.83e-7, a factor of 4.00 per halving, with the clamp
# sets unchanged at each (measured with this file's _figures(c, h=...)); the H against H / 2 condition below
# is what excludes such a sample without looking at the gradient
SEED = 2700
H = 5e-7
BOUND = 1e-5


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 30 + (name.endswith("_dev"))
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_policy_rollout_adjoint_batch(" in text and "int nmpc_policy_rollout_adjoint_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever
    else is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_policy_rollout_adjoint.py::test_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp, ip = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int32)
    buf = (C.c_double * 8)()
    q, qi = C.cast(buf, dp), C.cast(buf, ip)
    outs = (q,) * 6 + (qi,)
    for B, Ms, ins, o in ((1, 1, [q, 0] * 10, outs), (0, 1, [q, 0] * 10, outs), (1, 0, [q, 0] * 10, outs),
                          (1, 1, [q, -1] * 10, outs), (1, 1, [None, 0] * 10, (None,) * 7)):
        rc = L.nmpc_policy_rollout_adjoint_batch(None, B, Ms, *ins, *o)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, Ms)
    a = vp(C.addressof(buf))
    rc = L.nmpc_policy_rollout_adjoint_batch_dev(None, 1, 1, *([a, 0] * 10), *([a] * 7), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_adjoint_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by nmpc_eval.hip after
    nmpc_policy_rollout.hip, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        text = fh.read()
    assert '#include "nmpc_policy_rollout_adjoint.hip"' in text
    assert text.index('#include "nmpc_policy_rollout.hip"') < text.index('#include "nmpc_policy_rollout_adjoint.hip"')
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_policy_rollout_adjoint.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


@functools.lru_cache(maxsize=None)
def _cases():
    """Per solved scenario: its data, the four samples' base rollouts, the seeds and the direction."""
    out = []
    i = 0
    for name in pf.SOLVED:
        spec, prob, P, bounds, sols = sr.solved(name)
        assert all(s["status"] in (0, 1) for s in sols), [s["status"] for s in sols]
        dp = pf.directions(spec, len(sols), 95)[:, :1]
        for b in range(len(sols)):
            pol = pf.policy_of(name, b, dp)
            N, nu, nx = prob.N, prob.nu, prob.nx
            lo, hi = rr.widen(bounds[0], bounds[1])
            lo, hi = lo.reshape(N, nu), hi.reshape(N, nu)
            e0, w = rr.draw_disturbances(prob, 1, M, SIGMA, SEED + i, big=(1, 2), scale=SCALE)
            rng = np.random.default_rng(600 + i)
            seeds = [(float(rng.standard_normal()), rng.standard_normal((N + 1, nx)), rng.standard_normal((N, nu)))
                     for _ in range(M)]
            ti = prob.target_index
            d = {"p": np.zeros(len(P[b])), "ubar": rng.standard_normal((N, nu)), "Xbar": rng.standard_normal((N + 1, nx)),
                 "K": rng.standard_normal((N, nu, nx)) * np.max(np.abs(pol["K"])),
                 "e0": rng.standard_normal((M, nx)), "w": rng.standard_normal((M, N, nx))}
            d["p"][ra.read_entries(prob)] = rng.standard_normal(len(ra.read_entries(prob)))
            assert ti + 1 < len(P[b])
            c = {"name": name, "b": b, "prob": prob, "p": P[b], "ubar": sols[b]["x"].reshape(N, nu), "Xbar": pol["X"],
                 "K": pol["K"], "lo": lo, "hi": hi, "e0": e0[0], "w": w[0], "seeds": seeds, "d": d}
            c["base"] = [rr.rollout_one(prob, c["p"], c["ubar"], c["Xbar"], c["K"], c["e0"][s], c["w"][s], lo, hi)
                         for s in range(M)]
            out.append(c)
            i += 1
    return out


def _moved(c, s, t):
    """rollout_one of sample s at the inputs moved by t along the direction."""
    d = c["d"]
    return rr.rollout_one(c["prob"], c["p"] + t * d["p"], c["ubar"] + t * d["ubar"], c["Xbar"] + t * d["Xbar"],
                          c["K"] + t * d["K"], c["e0"][s] + t * d["e0"][s], c["w"][s] + t * d["w"][s], c["lo"], c["hi"])


def _figures(c, mutant=None, h=H):
    """Per sample: (|difference - <g, d>| / sum |g_i| |d_i|, the same relative to |<g, d>|, nsat, the
    clamp sets of both difference points equal the base point's, |difference at h - difference at h / 2| over the
    same sum: the difference's own error, whatever the gradient)."""
    prob, d, figs = c["prob"], c["d"], []
    for s in range(M):
        Jb, Xb, Ub = c["seeds"][s]
        g = ra.adjoint_one(prob, c["p"], c["ubar"], c["Xbar"], c["K"], c["base"][s]["X"], Jb, Xb, Ub, c["lo"], c["hi"],
                           mutant=mutant)
        assert g["nsat"] == c["base"][s]["nsat"]
        pairs = ((g["p_bar"], d["p"]), (g["ubar_bar"], d["ubar"]), (g["Xbar_bar"], d["Xbar"]), (g["K_bar"], d["K"]),
                 (g["e0_bar"], d["e0"][s]), (g["w_bar"], d["w"][s]))
        gd = sum(float(np.sum(a * b)) for a, b in pairs)
        scale = sum(float(np.sum(np.abs(a) * np.abs(b))) for a, b in pairs)
        rp, rm = _moved(c, s, h), _moved(c, s, -h)
        base_set = ra.clamp_set(c["base"][s]["U"], c["lo"], c["hi"])
        same = bool(np.array_equal(ra.clamp_set(rp["U"], c["lo"], c["hi"]), base_set)
                    and np.array_equal(ra.clamp_set(rm["U"], c["lo"], c["hi"]), base_set))
        fd = (ra.loss_one(rp, Jb, Xb, Ub) - ra.loss_one(rm, Jb, Xb, Ub)) / (2 * h)
        h2 = (ra.loss_one(_moved(c, s, h / 2), Jb, Xb, Ub) - ra.loss_one(_moved(c, s, -h / 2), Jb, Xb, Ub)) / h
        figs.append((abs(fd - gd) / scale, abs(fd - gd) / abs(gd), g["nsat"], same, abs(fd - h2) / scale))
    return figs


def test_the_checker_passes_its_own_gate():
    """The directional derivative against central differences of rollout_one on the 13 solved
    scenarios x 4 samples, the clamp sets unchanged by the difference step, both kinds of sample
    present."""
    worst = 0.0
    for c in _cases():
        figs = _figures(c)
        print(f"{c['name']} scenario {c['b']}: |fd - <g, d>| / sum |g||d| = " + ", ".join(f"{f[0]:.1e}" for f in figs)
              + "; relative to |<g, d>| " + ", ".join(f"{f[1]:.1e}" for f in figs) + f"; nsat {[f[2] for f in figs]}")
        assert all(f[3] for f in figs), (c["name"], c["b"], "a difference point flipped a clamp decision")
        assert any(f[2] > 0 for f in figs) and any(f[2] == 0 for f in figs), (c["name"], c["b"], [f[2] for f in figs])
        assert all(f[4] <= 1e-6 for f in figs), (c["name"], c["b"], "the difference itself is off", [f[4] for f in figs])
        assert all(f[0] <= BOUND for f in figs), (c["name"], c["b"], figs)
        worst = max(worst, max(f[1] for f in figs))
    print(f"largest |fd - <g, d>| / |<g, d>| over the {len(_cases()) * M} samples: {worst:.2e} (bound {BOUND:.0e} of the "
          f"absolute-term sum)")


@pytest.mark.parametrize("which", ra.MUTANTS)
def test_every_mutant_misses_the_gate(which):
    """Each mutant misses the gate on every scenario where it can act: `nomask` on a sample with
    nsat > 0, `noKt` and `transpose` wherever K is not 0, `shiftlam` everywhere."""
    for c in _cases():
        assert np.max(np.abs(c["K"])) > 0
        figs = _figures(c, mutant=which)
        acts = [f for f in figs if f[2] > 0] if which == "nomask" else figs
        assert acts, (which, c["name"], c["b"])
        print(f"{c['name']} scenario {c['b']}, mutant {which}: |fd - <g, d>| / sum |g||d| = "
              + ", ".join(f"{f[0]:.1e}" for f in acts) + f" (bound {BOUND:.0e})")
        assert max(f[0] for f in acts) > BOUND, (which, c["name"], c["b"], figs)
