"""The basis of the bounds of tests/test_gpu_fp32_step.py, measured wherever the suite runs, on
the float32 restatement of tests/fp32_ref.py and the dense matrices of tests/kkt_ref.py alone:
the table of rho after no, one and two fp64 refinements of a float32 factorisation, the
separation between 'refined' and 'not refined', the barrier regime's record, and mutants of the
refinement's residual."""
import numpy as np
import pytest

from tests import eval_ref as er
from tests import fp32_ref as fr
from tests import kkt_ref as kr


def test_the_float64_restatement_is_kkt_refs():
    """dtype = float64: operation for operation kkt_ref.riccati_np (bitwise), fixed variables
    included; kkt_ref's own callers are untouched."""
    for name in ("race_track_2", "uav5", "n1"):
        spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
        fx = fr.draw_fixed(spec, er.CASES[name])
        for b, ev in enumerate(evs):
            for fixed in (None, fx[b]):
                a = (ev, inp["obj_factor"], inp["lam_g"][b], inp["sigma_x"][b], inp["sigma_s"][b], inp["delta"][b])
                dw, ok = kr.riccati_np(*a, inp["r_w"][b], inp["r_g"][b], fixed=fixed)
                F = fr.Factor(*a, np.float64, fixed)
                assert ok and F.ok
                np.testing.assert_array_equal(F.solve(inp["r_w"][b], inp["r_g"][b]), dw)


@pytest.mark.parametrize("regime", fr.GATED)
@pytest.mark.parametrize("name", list(er.CASES))
def test_the_table_and_the_separation(name, regime):
    """Per case and combo: rho of the float32 step, after one and after two fp64 refinements
    (max over scenarios and columns), and rho0_ref >= 100 x bound1: an unrefined step cannot
    meet the refined step's bound.  One refinement buys four to six orders of magnitude."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, regime, combo)
        ref, bd = fr.bounds(name, regime, combo)
        cond = max(o["cond"] for o in per)
        print(f"{name} {regime} obj {combo[0]}: cond {cond:.1e}, rho float32 {ref[0]:.1e}, one refinement {ref[1]:.1e}, "
              f"two {ref[2]:.1e}; bound1 {bd[1]:.1e}, rho0_ref / bound1 {ref[0] / bd[1]:.0f}")
        assert ref[0] >= fr.SEPARATION * bd[1], (name, regime, combo, ref, bd)
        assert ref[0] <= 1e-6  # the float32 step is a float32 step (unit roundoff 6e-8)
        assert ref[1] <= ref[0] and ref[2] <= max(ref[1], spec.nw * fr.EPS)  # (at the fp64 floor both are rounding)


@pytest.mark.parametrize("name", list(er.CASES))
def test_the_barrier_regime_is_recorded(name):
    """cond(M) up to 1e15: the float32 Cholesky fails on some scenario of most cases, and where
    it succeeds a refinement gains little.  Printed, nothing gated but that the record exists."""
    for combo in kr.COMBOS:
        spec, inp, per, evs = kr.reference(name, "barrier", combo)
        r, ok = fr.case_figures(name, "barrier", combo)
        for b in range(er.CASES[name]):
            what = f"{name} barrier obj {combo[0]} scenario {b}: cond {per[b]['cond']:.1e}, "
            print(what + (f"rho {r[b, 0]:.1e} / {r[b, 1]:.1e} / {r[b, 2]:.1e}" if ok[b] else "float32 Cholesky fails"))
        assert r.shape == (er.CASES[name], 3) and np.all(np.isfinite(r[ok]))


def test_the_restatement_with_fixed_variables():
    """uav8g and uav5 with a third of the controls fixed (a whole stage among them): the refined
    float32 step is exactly 0 there and meets the case's bounds on the reduced system."""
    for name in ("race_track_2", "uav5"):
        spec, inp, per, evs = kr.reference(name, "mild", kr.COMBOS[1])
        ref, bd = fr.bounds(name, "mild", kr.COMBOS[1])
        fx = fr.draw_fixed(spec, er.CASES[name])
        for b, ev in enumerate(evs):
            dws = fr.steps(ev, per[b], inp, b, fixed=fx[b])
            r = np.max(fr.rhos(dws, per[b], ~fx[b]), axis=1)
            print(f"{name} fixed scenario {b}: {int(fx[b].sum())} of {spec.nw} fixed, rho {r[0]:.1e} / {r[1]:.1e} / {r[2]:.1e}")
            assert all(np.all(d[:, fx[b]] == 0.0) for d in dws)
            assert np.all(r <= bd), (name, b, r, bd)


# what each mutant needs to be visible: delta > 0 on some scenario (n1: delta = 0 everywhere;
# uav5 at obj_factor 1: delta = 0 everywhere), S_k != 0 (n1, N = 1: no S_k)
def _applies(mutant, name, inp):
    if mutant == "no_delta":
        return bool(np.any(inp["delta"] > 0))
    if mutant == "no_Hxu":
        return name != "n1"
    return True


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_a_wrong_refinement_residual_misses_the_bound(mutant):
    """The refinement's residual formed without delta on the control diagonal, without the two
    S_k entries, without sigma_x, or in float32: after one such refinement the step misses
    bound1 by >= 10x on some scenario of every mild case the mutant applies to (measured: at
    least 4.6e2x -- the float32 residual on race_track_2 -- and 3e5x to 5e9x for the dropped
    terms).  Every mutant reaches 10x on every applicable case: none is left unasserted."""
    for combo in kr.COMBOS:
        for name in er.CASES:
            spec, inp, per, evs = kr.reference(name, "mild", combo)
            if not _applies(mutant, name, inp):
                continue
            ref, bd = fr.bounds(name, "mild", combo)
            worst = 0.0
            for b, ev in enumerate(evs):
                dws = fr.steps(ev, per[b], inp, b, mutant=mutant, nref=1)
                worst = max(worst, float(np.max(fr.rhos(dws, per[b])[1])) / bd[1])
            print(f"{mutant} {name} obj {combo[0]}: rho(dw1) / bound1 = {worst:.1e}")
            assert worst >= fr.MARGIN, (mutant, name, combo, worst)
