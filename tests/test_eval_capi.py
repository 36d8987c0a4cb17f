"""The evaluation entry points without a GPU: exported, argument checks before any device
call, and built as a translation unit of their own whose source the build hash covers."""
import ctypes as C
import os

import __graft_entry__ as ge
from nmpc_amd import _lib


def test_null_handle_is_invalid_for_both_entry_points():
    L = _lib.lib()
    dp, vp = C.POINTER(C.c_double), C.c_void_p
    buf = (C.c_double * 8)()
    q = C.cast(buf, dp)
    rc = L.nmpc_eval_batch(None, 1, q, 0, q, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None, 0,
                           q, None, None, None, None, None)
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    a = vp(C.addressof(buf))
    rc = L.nmpc_eval_batch_dev(None, 1, a, 0, a, 0, *([vp(0), 0] * 6), a, *([vp(0)] * 5), vp(0))
    assert rc == -1 and b"handle" in L.nmpc_last_error()
    assert list(buf) == [0.0] * 8


def test_evaluation_kernel_is_its_own_translation_unit(tmp_path, monkeypatch):
    """Nine translation units; the ninth is nmpc_eval.hip, which reaches the solver's device
    functions by including its source with no class selected, and the library's build id
    covers both new files."""
    assert len(ge._TUS) == 9 and ge._TUS[-1] == ("eval", "nmpc_eval.hip")
    assert [d for _, d in ge._TUS[:8]] == ["-DNMPC_TU_HOST"] + [f"-DNMPC_TU_CLASS={i}" for i in range(1, 8)]
    src = os.path.join(ge.CSRC, "nmpc_eval.hip")
    with open(src) as fh:
        text = fh.read()
    assert "#define NMPC_TU_CLASS 0" in text and '#include "nmpc_solve.hip"' in text
    # the hash over a copy of csrc/ moves when either new file does
    import shutil
    copy = tmp_path / "csrc"
    shutil.copytree(ge.CSRC, copy)
    before = ge.source_hash()
    monkeypatch.setattr(ge, "CSRC", str(copy))
    assert ge.source_hash() == before
    for name in ("nmpc_eval.hip", "nmpc_eval.h"):
        with open(copy / name, "ab") as fh:
            fh.write(b"\n// x\n")
        after = ge.source_hash()
        assert after != before, name
        before = after
