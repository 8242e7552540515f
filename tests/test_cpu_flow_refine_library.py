"""CPU tests (no GPU) of libt2v_flow.so's boundary, what tests/test_cpu_cabi.py asks of the other libraries: a compiler
confirms the prototypes and constants the reader read from include/t2v_flow_refine.h, the library exports exactly the header's
symbols, and its kernels are the Lucas-Kanade kernels plus the refinement's and nothing else."""
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
    from text2video_amd import _cabi, _flowlib
    h = _cabi.read_header("t2v_flow_refine.h")
    assert list(h.functions) == ["t2v_flow_refine_abi_version", "t2v_optical_flow_refined_workspace_floats",
                                 "t2v_optical_flow_refined", "t2v_optical_flow_refined_u8"]
    assert h.signatures == _flowlib.SIGNATURES and h.opaque == {"t2v_ctx"} and not h.structs
    assert h.constants == {"T2V_FLOW_REFINE_ABI_VERSION": 1, "T2V_FLOW_REFINE_MAX_FUSED": 8}
    assert (_flowlib.ABI_VERSION, _flowlib.MAX_FUSED) == (1, 8)
    # the entries take what the LK entries of t2v.h take, plus (float alpha, int refine_iters, int iters_per_launch)
    lk = _cabi.read_header("t2v.h").functions
    for name in ("t2v_optical_flow", "t2v_optical_flow_u8"):
        ret, params = lk[name]
        assert h.functions[name.replace("flow", "flow_refined")] == (ret, params[:-2] + ["float", "int", "int"] + params[-2:])
    assert h.functions["t2v_optical_flow_refined_workspace_floats"] == lk["t2v_optical_flow_workspace_floats"]
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: it is the check that the header reader read the header right"
    # the header stands beside t2v.h in one translation unit (both declare the opaque t2v_ctx)
    tu = ['#include <type_traits>', '#include "t2v.h"', '#include "t2v_flow_refine.h"']
    for name, (ret, params) in h.functions.items():
        tu.append('static_assert(std::is_same<decltype(&%s), %s (*)(%s)>::value, "%s");' % (name, ret, ", ".join(params), name))
    for name, value in h.constants.items():
        tu.append('static_assert(%s == %d, "%s");' % (name, value, name))
    for text, ok in (("\n".join(tu), True), ("\n".join(tu).replace("float, int, int, float*, float*", "float, int, long, float*, float*", 1), False)):
        src = tmp_path / ("flow_%s.cpp" % ok)
        src.write_text(text + "\n")
        r = subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                           capture_output=True, text=True)
        assert (r.returncode == 0) is ok, r.stderr[-3000:]


def test_the_library_exports_the_header_and_its_kernels_are_the_flow_kernels(lib_built):
    from text2video_amd import _flowlib
    lib = _flowlib.load()
    assert lib.t2v_flow_refine_abi_version() == _flowlib.ABI_VERSION
    out = _nm("-D", "--defined-only", _flowlib.LIB_PATH)
    exported = {s for s in (ln.split()[-1] for ln in out.splitlines() if ln.strip()) if s.startswith("t2v_")}
    assert exported == set(_flowlib.SIGNATURES), sorted(exported ^ set(_flowlib.SIGNATURES))
    # kernel stubs of the library: the LK kernels (MODE 0, 1 and 3: never the smoothing hand-down of the LK entry), the
    # preparation, one Jacobi kernel per fused step count, the plain output pass
    stubs = set(re.findall(r"__device_stub__(\w+?)(?:\(|<)", _nm("-C", _flowlib.LIB_PATH)))
    assert stubs == {"flow_grey_kernel", "flow_grey_u8_kernel", "flow_pool_kernel", "flow_lk_kernel", "flow_hs_prep_kernel",
                     "flow_hs_kernel", "flow_out_plain_kernel"}, sorted(stubs)
    text = _nm("-C", _flowlib.LIB_PATH)
    assert {int(k) for k in re.findall(r"__device_stub__flow_hs_kernel<(\d+)>", text)} == set(range(1, _flowlib.MAX_FUSED + 1))
    assert {int(k) for k in re.findall(r"__device_stub__flow_lk_kernel<(\d+)>", text)} == {0, 1, 3}
    # refusals need no GPU: nothing is launched, and the message is where t2v_last_error reads it
    import ctypes
    from text2video_amd import _lib
    assert lib.t2v_optical_flow_refined_workspace_floats(64, 96, 0) == 2 * lib_built.t2v_optical_flow_workspace_floats(64, 96, 0)
    assert lib.t2v_optical_flow_refined_workspace_floats(7, 96, 0) == 0
    p = ctypes.c_void_p(16)      # never read
    rc = lib.t2v_optical_flow_refined(p, None, p, 4, 0, p, 4, 0, 64, 96, 0, 3, 3, 1e-3, 0.2, 64, 9, p, p)
    assert rc == _lib.ERR_INVALID and b"iters_per_launch" in lib_built.t2v_last_error()
    rc = lib.t2v_optical_flow_refined_u8(p, None, p, 3, p, 3, 64, 96, 0, 3, 3, 1e-3, 0.0, 64, 0, p, p)
    assert rc == _lib.ERR_INVALID and b"alpha" in lib_built.t2v_last_error()
