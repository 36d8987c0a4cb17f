"""The test-side probe library (tests/probe): it cross-compiles for gfx950 without a GPU,
exports its launchers, is built from the product's own kernel source, and stays out of the
product (its library, and the hash nmpc_build_id reports)."""
import ctypes
import os
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
