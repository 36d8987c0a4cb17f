"""The test-side probe library (tests/probe): it cross-compiles for gfx950 without a GPU,
exports its launchers, is built from the product's own kernel source, and stays out of the
product (its library, and the hash nmpc_build_id reports)."""
import ctypes
import os
import shutil
import subprocess

import __graft_entry__ as ge
from tests.probe import build as pb


def test_probe_cross_compiles_and_exports_its_launchers():
    path = pb.build()
    assert os.path.exists(path)
    with open(pb.STAMP) as fh:
        assert fh.read().strip() == pb.probe_hash()
    L = ctypes.CDLL(path)
    for n in pb.EXPORTS:
        assert hasattr(L, n), n
    with open(path, "rb") as fh:
        blob = fh.read()
    assert b"gfx950" in blob                       # a device code object for the target
    assert b"nmpc_solve_batch" not in blob         # NMPC_TU_CLASS == 0: no C-ABI in the probe
    # argument validation happens before any device call
    assert pb.lib().nmpc_probe_qd(0, None, None, None) != 0


def test_probe_exports_the_step_launcher_for_every_precision_class(tmp_path, monkeypatch):
    """nmpc_probe_lq_step: exported, its kernel instantiated for CapC (fp64), CapC32 and CapA32
    (fp32 factors; the mangled Cap<N, m, lds_rows, type> of each is in the device code), its
    arguments checked before any device call, and the probe's hash covers every product file its
    translation unit reads."""
    path = pb.build()
    assert "nmpc_probe_lq_step" in pb.EXPORTS and hasattr(ctypes.CDLL(path), "nmpc_probe_lq_step")
    with open(path, "rb") as fh:
        blob = fh.read()
    for cap in (b"3CapILi63ELi21ELb0EdLb0EE", b"3CapILi63ELi21ELb0EfLb0EE", b"3CapILi20ELi15ELb1EfLb0EE"):
        assert b"probe_lq_kernelIN9nmpc_impl" + cap in blob, cap
    assert set(pb.LQ_CLASSES) == set(pb.LQ_CAPACITY) == {"C", "C32", "A32"}
    L = pb.lib()
    z = (ctypes.c_double * 8)()
    q = ctypes.cast(z, ctypes.POINTER(ctypes.c_double))
    i = ctypes.cast((ctypes.c_int32 * 2)(), ctypes.POINTER(ctypes.c_int32))
    assert L.nmpc_probe_lq_step(0, None, 1, 1, q, q, q, 1.0, q, q, q, q, q, q, q, q, i) == 1    # no description
    from nmpc_amd import _lib
    d = _lib.Desc()                                                                           # N = 0: refused
    assert L.nmpc_probe_lq_step(0, ctypes.byref(d), 1, 1, q, q, q, 1.0, q, q, q, q, q, q, q, q, i) == 1
    d.N, d.np, d.T = 21, 11, 0.2
    assert L.nmpc_probe_lq_step(7, ctypes.byref(d), 1, 1, q, q, q, 1.0, q, q, q, q, q, q, q, q, i) == 1  # no such class
    assert L.nmpc_probe_lq_step(2, ctypes.byref(d), 1, 1, q, q, q, 1.0, q, q, q, q, q, q, q, q, i) == 1  # N > 20 in CapA32
    assert L.nmpc_probe_lq_step(0, ctypes.byref(d), 0, 1, q, q, q, 1.0, q, q, q, q, q, q, q, q, i) == 1  # B = 0
    assert list(z) == [0.0] * 8
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = pb.probe_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert pb.probe_hash() == before
    for f in ("nmpc_solve.hip", "nmpc_eval.h"):
        with open(copy / f, "ab") as fh:
            fh.write(b"\n// x\n")
        changed = pb.probe_hash()
        assert changed != before, f
        before = changed


def test_probe_includes_the_product_source_and_the_product_ignores_the_probe():
    with open(pb.SRC) as fh:
        text = fh.read()
    assert '#include "../../mpc-implementation_amd/csrc/nmpc_solve.hip"' in text
    assert "#define NMPC_TU_CLASS 0" in text
    before = ge.source_hash()
    assert pb.probe_hash() != before
    for root, _, files in os.walk(ge.PKG_DIR):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                with open(os.path.join(root, f), errors="replace") as fh:
                    assert "nmpc_probe" not in fh.read(), f
    if os.path.exists(ge.LIB):
        with open(ge.LIB, "rb") as fh:
            assert b"nmpc_probe" not in fh.read()


def test_an_unknown_translation_unit_class_is_a_compile_error():
    src = os.path.join(ge.CSRC, "nmpc_solve.hip")
    r = subprocess.run([ge.HIPCC, *ge._flags(), "--cuda-host-only", "-DNMPC_TU_CLASS=8", "-E", src, "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "NMPC_TU_CLASS must be" in r.stderr
    r = subprocess.run([ge.HIPCC, *ge._flags(), "--cuda-host-only", "-DNMPC_TU_CLASS=0", "-E", src, "-o", os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
