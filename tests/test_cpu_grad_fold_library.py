"""CPU tests (no GPU) of libt2v_gradfold.so's boundary, what tests/test_cpu_flow_refine_library.py asks of libt2v_flow.so: a
compiler confirms the prototypes and constants the reader read from include/t2v_grad_fold.h, the library exports exactly the
header's symbols, its kernels are the fold kernel's three modes and nothing else, and every refusal comes back as
ERR_INVALID with a message before anything is launched."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm(*args):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("`nm` (binutils) is needed to list the symbols of the libraries and is not on PATH")
    return subprocess.run([nm] + list(args), check=True, capture_output=True, text=True).stdout


def test_a_compiler_confirms_the_header(tmp_path):
    from text2video_amd import _cabi, _gradfoldlib
    h = _cabi.read_header("t2v_grad_fold.h")
    assert list(h.functions) == ["t2v_grad_fold_abi_version", "t2v_grad_fold"]
    assert h.functions["t2v_grad_fold"] == ("int", ["t2v_ctx*", "void*", "float*", "float*", "long", "int", "float"])
    assert h.signatures == _gradfoldlib.SIGNATURES and h.opaque == {"t2v_ctx"} and not h.structs
    assert h.constants == {"T2V_GRAD_FOLD_ABI_VERSION": 1, "T2V_GRAD_FOLD_OPEN": 0, "T2V_GRAD_FOLD_ADD": 1,
                           "T2V_GRAD_FOLD_CLOSE": 2}
    assert (_gradfoldlib.ABI_VERSION, _gradfoldlib.OPEN, _gradfoldlib.ADD, _gradfoldlib.CLOSE) == (1, 0, 1, 2)
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: it is the check that the header reader read the header right"
    # the header stands beside t2v.h in one translation unit (both declare the opaque t2v_ctx)
    tu = ['#include <type_traits>', '#include "t2v.h"', '#include "t2v_grad_fold.h"']
    for name, (ret, params) in h.functions.items():
        tu.append('static_assert(std::is_same<decltype(&%s), %s (*)(%s)>::value, "%s");' % (name, ret, ", ".join(params), name))
    for name, value in h.constants.items():
        tu.append('static_assert(%s == %d, "%s");' % (name, value, name))
    text = "\n".join(tu)
    assert "float*, float*, long, int, float" in text
    for text, ok in ((text, True), (text.replace("float*, float*, long, int, float", "float*, float*, int, int, float", 1), False)):
        src = tmp_path / ("fold_%s.cpp" % ok)
        src.write_text(text + "\n")
        r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) is ok, r.stderr[-3000:]


def test_the_library_exports_the_header_and_its_kernels_are_the_fold_kernel(lib_built):
    from text2video_amd import _gradfoldlib
    lib = _gradfoldlib.load()
    assert lib.t2v_grad_fold_abi_version() == _gradfoldlib.ABI_VERSION
    out = _nm("-D", "--defined-only", _gradfoldlib.LIB_PATH)
    exported = {s for s in (ln.split()[-1] for ln in out.splitlines() if ln.strip()) if s.startswith("t2v_")}
    assert exported == set(_gradfoldlib.SIGNATURES), sorted(exported ^ set(_gradfoldlib.SIGNATURES))
    text = _nm("-C", _gradfoldlib.LIB_PATH)
    assert set(re.findall(r"__device_stub__(\w+?)(?:\(|<)", text)) == {"grad_fold_kernel"}
    assert {int(k) for k in re.findall(r"__device_stub__grad_fold_kernel<(\d+)>", text)} == \
        {_gradfoldlib.OPEN, _gradfoldlib.ADD, _gradfoldlib.CLOSE}


def test_refusals_need_no_gpu(lib_built):
    """nothing is launched and nothing read: the pointers below are never dereferenced, and the message is where
    t2v_last_error reads it"""
    from text2video_amd import _gradfoldlib, _lib
    lib = _gradfoldlib.load()
    ctx, g, a = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)
    O, A, C = _gradfoldlib.OPEN, _gradfoldlib.ADD, _gradfoldlib.CLOSE

    def refused(word, *args):
        rc = lib.t2v_grad_fold(*args)
        msg = lib_built.t2v_last_error()
        assert rc == _lib.ERR_INVALID and word in msg, (rc, msg, args)

    refused(b"null", None, None, g, a, 8, O, 1.0)
    refused(b"null", ctx, None, None, a, 8, O, 1.0)
    refused(b"null", ctx, None, g, None, 8, C, 1.0)
    refused(b"n must be", ctx, None, g, a, 0, A, 1.0)
    refused(b"n must be", ctx, None, g, a, -5, A, 1.0)
    refused(b"mode", ctx, None, g, a, 8, 3, 1.0)
    refused(b"mode", ctx, None, g, a, 8, -1, 1.0)
    for bad in (0.0, -0.5, float("inf"), float("nan")):
        for mode in (O, A, C):
            refused(b"scale", ctx, None, g, a, 8, mode, bad)
    refused(b"aligned", ctx, None, ctypes.c_void_p((1 << 20) + 2), a, 8, O, 1.0)
    # overlapping ranges: the same buffer, acc beginning inside grad, grad beginning inside acc; touching ranges do not overlap
    refused(b"overlap", ctx, None, g, g, 8, A, 1.0)
    refused(b"overlap", ctx, None, g, ctypes.c_void_p((1 << 20) + 28), 8, A, 1.0)
    refused(b"overlap", ctx, None, ctypes.c_void_p((1 << 20) + 4), g, 8, C, 0.5)
