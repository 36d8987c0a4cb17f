"""The policy-covariance adjoint entry points without a GPU: exported, declared, a NULL handle refused
before any device call, the kernel's file part of the evaluation unit and under the build hash -- and the
checker of tests/test_gpu_policy_covariance_adjoint.py (tests/covariance_adjoint_ref.py) held against
central differences of tests/covariance_ref.covariance_one on the oracle alone.

Cases: those of tests/test_covariance_capi.py::_cases (the 13 solved scenarios with the dense-oracle
policy, n1, and two scenarios of n63_16obs), each with obs_var drawn in [0.25, 1.25) where it has
obstacles and with seeds Sb (asymmetric), ub and gb drawn N(0, 1), fixed by seed.  With
L = sum_k <Sb_k, Sigma_k> + <ub, var_u> + <gb, var_g>, the checker's <gradient, direction> is held
against (L(+eps d) - L(-eps d)) / 2 eps along one random direction per input group; the figure is
|difference| / max(|central difference|, |<gradient, direction>|) (0 where both are 0).

  linear   (S0, W, obs_var; symmetric directions for S0 and W): L is linear in them, so the identity
           holds to rounding at eps = 1e-3.  Measured: worst 2.7e-14; gate 10 x that.
  K, ubar, Xbar, p: eps in {1e-4, 1e-5, 1e-6}, every figure printed; gated at 10 x the worst figure over
           the cases at the group's best eps (the margin is for the platform's libm).  Measured, worst
           over the cases at eps = 1e-4 / 1e-5 / 1e-6:
             K     7.7e-7 / 8.2e-9 / 7.6e-9    gate 7.6e-8 at 1e-6
             ubar  1.3e-7 / 1.9e-6 / 1.3e-5    gate 1.3e-6 at 1e-4  (n1 scenario 0 sets all three; the
                                               other cases stay below 9.4e-8 / 3.1e-7 / 5.1e-6)
             Xbar  3.4e-7 / 5.7e-9 / 5.8e-8    gate 5.7e-8 at 1e-5
             p     3.3e-8 / 3.3e-7 / 5.9e-6    gate 3.3e-7 at 1e-4  (non-zero on `dynamic` alone)
           On benign plans (random plans and gains of size 0.3) the same recursion reaches 1e-9 and
           better; the solved cases' deadbeat gains and n1's single stage cost up to two digits.
  mutants  each mutant's figure in its own groups (transpose, half: K, ubar, Xbar; shift: K; noW: linear;
           rows: Xbar) misses the gate by at least 100 x on every case.  Left out where the mutant is
           structurally the original: `shift` on n1 (N = 1: no K_1 to take K_0's place) and `rows` on the
           cases without obstacles (none among these cases).
The measured figures are printed wherever the suite runs."""
import ctypes as C
import functools
import os
import shutil

import numpy as np
import pytest

import __graft_entry__ as ge
from nmpc_amd import _lib
from tests import covariance_adjoint_ref as ar
from tests import covariance_ref as cr
from tests.test_covariance_capi import _cases

NAMES = ("nmpc_policy_covariance_adjoint_batch", "nmpc_policy_covariance_adjoint_batch_dev")
EPS_LIN = 1e-3
EPS = (1e-4, 1e-5, 1e-6)
GROUPS = ("K", "ubar", "Xbar", "p")
# 10 x the worst measured figure (module docstring) at the group's best eps
GATE = {"linear": (EPS_LIN, 2.7e-13), "K": (1e-6, 7.6e-8), "ubar": (1e-4, 1.3e-6), "Xbar": (1e-5, 5.7e-8),
        "p": (1e-4, 3.3e-7)}
MUTANT_GROUPS = {"transpose": ("K", "ubar", "Xbar"), "shift": ("K",), "noW": ("linear",), "half": ("K", "ubar", "Xbar"),
                 "rows": ("Xbar",)}
TEETH = 100.0


def test_both_symbols_are_exported_and_declared():
    L = _lib.lib()
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == 27 + (name.endswith("_dev"))
    with open(os.path.join(ge.ROOT, "include", "nmpc_amd.h")) as fh:
        text = fh.read()
    assert "int nmpc_policy_covariance_adjoint_batch(" in text and "int nmpc_policy_covariance_adjoint_batch_dev(" in text


def test_invalid_arguments_are_refused_before_any_device_call():
    """NMPC_E_INVALID before anything is read or written: a NULL handle is refused first, whatever else
    is wrong with the call.  The other checks need a live handle:
    tests/test_gpu_policy_covariance_adjoint.py::test_gate_f_argument_validation_on_a_live_handle runs them."""
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    for B, nc, ins, outs in ((1, 1, [q, 0] * 8, (q,) * 8), (0, 1, [q, 0] * 8, (q,) * 8), (1, 0, [q, 0] * 8, (q,) * 8),
                             (1, 1, [q, -1] * 8, (q,) * 8), (1, 1, [None, 0] * 8, (None,) * 8)):
        rc = L.nmpc_policy_covariance_adjoint_batch(None, B, nc, *ins, *outs)
        assert rc == -1 and b"handle" in L.nmpc_last_error(), (B, nc)
    a = vp(C.addressof(buf))
    rc = L.nmpc_policy_covariance_adjoint_batch_dev(None, 1, 1, *([a, 0] * 8), *([a] * 8), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_adjoint_kernel_lives_in_the_evaluation_unit(tmp_path, monkeypatch):
    """Still nine translation units: the kernel's file is included by the forward kernel's, after its
    last line of code, and the library's build id covers it."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    with open(os.path.join(ge.CSRC, "nmpc_policy_covariance.hip")) as fh:
        text = fh.read()
    inc = '#include "nmpc_policy_covariance_adjoint.hip"'
    assert text.count("#include") == 1 and text.rstrip().endswith(inc)
    with open(os.path.join(ge.CSRC, "nmpc_eval.hip")) as fh:
        assert "covariance_adjoint" not in fh.read()
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    with open(copy / "nmpc_policy_covariance_adjoint.hip", "ab") as fh:
        fh.write(b"\n// x\n")
    assert ge.source_hash() != before


@functools.lru_cache(maxsize=None)
def _setup(i):
    """Case i with its obs_var, seeds, directions, forward result and the checker's gradient."""
    name, b, prob, p, ubar, Xbar, K, S0, W = _cases()[i]
    N, nx, nu, m = prob.N, prob.nx, prob.nu, prob.m
    rng = np.random.default_rng(700 + i)
    ov = 0.25 + rng.random(prob.n_obs) if prob.n_obs else None
    seeds = (rng.standard_normal((N + 1, nx, nx)), rng.standard_normal((N, nu)), rng.standard_normal((N + 1, m)))
    d = {"S0": ar.sym(rng.standard_normal((nx, nx))) * np.max(np.abs(S0)), "W": ar.sym(rng.standard_normal((nx, nx))) * np.max(np.abs(W)),
         "obs_var": rng.standard_normal(prob.n_obs), "K": rng.standard_normal(K.shape),
         "ubar": rng.standard_normal(ubar.shape), "Xbar": rng.standard_normal(Xbar.shape), "p": rng.standard_normal(p.shape)}
    fwd = cr.covariance_one(prob, p, ubar, Xbar, K, S0, W, ov)
    return dict(name=name, b=b, prob=prob, ins=dict(p=p, ubar=ubar, Xbar=Xbar, K=K, S0=S0, W=W, obs_var=ov), seeds=seeds, d=d,
                Sigma=fwd["Sigma"])


@functools.lru_cache(maxsize=None)
def _central(i, group, eps):
    """(L(+eps d) - L(-eps d)) / 2 eps along the direction of `group` ("linear": S0, W and obs_var at once)."""
    c = _setup(i)
    keys = ("S0", "W", "obs_var") if group == "linear" else (group,)
    val = []
    for sgn in (1.0, -1.0):
        ins = dict(c["ins"])
        for k in keys:
            if ins[k] is not None:
                ins[k] = ins[k] + sgn * eps * c["d"][k]
        val.append(ar.loss_one(c["prob"], ins["p"], ins["ubar"], ins["Xbar"], ins["K"], ins["S0"], ins["W"], ins["obs_var"],
                               *c["seeds"]))
    return (val[0] - val[1]) / (2.0 * eps)


@functools.lru_cache(maxsize=None)
def _analytic(i, mutant=None):
    """<gradient, direction> per group from the checker (under `mutant`)."""
    c = _setup(i)
    ins, d = c["ins"], c["d"]
    g = ar.adjoint_one(c["prob"], ins["p"], ins["ubar"], ins["Xbar"], ins["K"], c["Sigma"], *c["seeds"], mutant=mutant)
    lin = float(np.sum(g["S0_bar"] * d["S0"]) + np.sum(g["W_bar"] * d["W"]) + np.sum(g["obs_var_bar"] * d["obs_var"]))
    return {"linear": lin, "K": float(np.sum(g["K_bar"] * d["K"])), "ubar": float(np.sum(g["ubar_bar"] * d["ubar"])),
            "Xbar": float(np.sum(g["Xbar_bar"] * d["Xbar"])), "p": float(np.sum(g["p_bar"] * d["p"])), "p_bar": g["p_bar"]}


def _figure(i, group, eps, mutant=None):
    fd, an = _central(i, group, eps), _analytic(i, mutant)[group]
    top = max(abs(fd), abs(an))
    return 0.0 if top == 0.0 else abs(fd - an) / top


def test_the_checker_agrees_with_central_differences():
    """Every group of every case at its gate; every figure printed first."""
    worst = {g: {e: 0.0 for e in ((EPS_LIN,) if g == "linear" else EPS)} for g in ("linear",) + GROUPS}
    bad = []
    for i in range(len(_cases())):
        c = _setup(i)
        prob = c["prob"]
        f = _figure(i, "linear", EPS_LIN)
        worst["linear"][EPS_LIN] = max(worst["linear"][EPS_LIN], f)
        line = [f"linear {f:.1e}"]
        if f > GATE["linear"][1]:
            bad.append((c["name"], c["b"], "linear", f))
        for g in GROUPS:
            figs = {e: _figure(i, g, e) for e in EPS}
            for e, v in figs.items():
                worst[g][e] = max(worst[g][e], v)
            line.append(f"{g} " + " / ".join(f"{figs[e]:.1e}" for e in EPS))
            if figs[GATE[g][0]] > GATE[g][1]:
                bad.append((c["name"], c["b"], g, figs[GATE[g][0]]))
        print(f"{c['name']} scenario {c['b']} (N = {prob.N}): " + ", ".join(line))
        # p_bar is non-zero only at the obstacle centres taken from p
        pb = _analytic(i)["p_bar"]
        centres = {int(q) for q in list(prob.obs_x_pidx) + list(prob.obs_y_pidx) if q >= 0}
        assert all(pb[q] == 0.0 for q in range(len(pb)) if q not in centres), (c["name"], c["b"])
    for g, w in worst.items():
        print(f"worst over the cases, {g}: " + ", ".join(f"eps {e:.0e}: {v:.2e}" for e, v in w.items())
              + f"   (gate {GATE[g][1]:.1e} at eps {GATE[g][0]:.0e})")
    assert not bad, bad


@pytest.mark.parametrize("which", ar.MUTANTS)
def test_every_mutant_misses_the_gate(which):
    """Each mutant misses the gate of one of its groups by at least 100 x on every case (module
    docstring: the cases where it is structurally the original are left out)."""
    smallest = np.inf
    for i in range(len(_cases())):
        c = _setup(i)
        prob = c["prob"]
        if (which == "shift" and prob.N == 1) or (which == "rows" and prob.n_obs == 0):
            print(f"{c['name']} scenario {c['b']}: mutant {which} is the original here, left out")
            continue
        miss = max(_figure(i, g, GATE[g][0], mutant=which) / GATE[g][1] for g in MUTANT_GROUPS[which])
        print(f"{c['name']} scenario {c['b']}, mutant {which}: figure / gate = {miss:.2e}")
        assert miss >= TEETH, (which, c["name"], c["b"], miss)
        smallest = min(smallest, miss)
    print(f"mutant {which}: smallest miss {smallest:.2e} x the gate")
