"""Builds and loads tests/probe/nmpc_probe.hip: probe kernels around the device primitives
of the product's kernel source (which the probe #includes), compiled with the product's own
flags (__graft_entry__._flags) into tests/probe/_build/ (git-ignored).  Rebuilt when the
hash of the probe, the kernel source, the header and the flags changes.  Test-side only: the
product library never loads it, and it is no part of nmpc_build_id's hash."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = os.path.join(HERE, "nmpc_probe.hip")
OUT_DIR = os.path.join(HERE, "_build")
LIB = os.path.join(OUT_DIR, "libnmpc_probe.so")
STAMP = LIB + ".hash"

EXPORTS = ("nmpc_probe_wreduce", "nmpc_probe_readlane_f64", "nmpc_probe_readlane_f32", "nmpc_probe_logacc",
           "nmpc_probe_unary", "nmpc_probe_rsqf", "nmpc_probe_qd", "nmpc_probe_lq_step")
# nmpc_probe_lq_step's cls argument: the kernel class whose factorisation, solves and refinement run
LQ_CLASSES = {"C": 0, "C32": 1, "A32": 2}
LQ_CAPACITY = {"C": (63, 21), "C32": (63, 21), "A32": (20, 15)}  # N, rows per stage


def _entry():
    import sys
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge


def probe_hash() -> str:
    ge = _entry()
    h = hashlib.sha256()
    # every file the probe's translation unit reads: nmpc_solve.hip includes nmpc_eval.h
    for f in (SRC, os.path.join(ge.CSRC, "nmpc_solve.hip"), os.path.join(ge.CSRC, "nmpc_eval.h"),
              os.path.join(ROOT, "include", "nmpc_amd.h")):
        with open(f, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(ge._flags()).replace(ROOT, "").encode())
    return h.hexdigest()[:32]


def build(force: bool = False) -> str:
    """Compile the probe for gfx950 (no GPU needed) unless an up-to-date one is there."""
    tag = probe_hash()
    if not force and os.path.exists(LIB) and os.path.exists(STAMP):
        with open(STAMP) as fh:
            if fh.read().strip() == tag:
                return LIB
    ge = _entry()
    os.makedirs(OUT_DIR, exist_ok=True)
    tmp = f"{LIB}.{os.getpid()}.tmp"
    subprocess.run([ge.HIPCC, *ge._flags(), "-shared", SRC, "-o", tmp], check=True)
    os.replace(tmp, LIB)
    with open(STAMP, "w") as fh:
        fh.write(tag + "\n")
    return LIB


_lib = None


def lib():
    """The probe library through ctypes (built on demand)."""
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(build())
    dp, fp, ip, i32, i64 = (C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32, C.c_int64)
    L.nmpc_probe_wreduce.argtypes = [i32, i32, dp, dp]
    L.nmpc_probe_readlane_f64.argtypes = [i32, dp, ip, dp]
    L.nmpc_probe_readlane_f32.argtypes = [i32, fp, ip, fp]
    L.nmpc_probe_logacc.argtypes = [i32, i32, i32, dp, ip, dp]
    L.nmpc_probe_unary.argtypes = [i32, i64, dp, dp]
    L.nmpc_probe_rsqf.argtypes = [i64, fp, fp]
    L.nmpc_probe_qd.argtypes = [i64, dp, dp, dp]
    L.nmpc_probe_lq_step.argtypes = ([i32, C.c_void_p, i32, i32, dp, dp, dp, C.c_double] + [dp] * 5 + [dp, dp, dp, ip])
    for n in EXPORTS:
        getattr(L, n).restype = C.c_int
    _lib = L
    return L
