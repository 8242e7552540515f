"""The guards of libt2v_hip.so and include/t2v.h, restated for what T2V_ALGO_DIRECT_BF16X2 adds beside them (no GPU):

* libt2v_split.so: every kernel instantiation in it has exactly one entry in split_direct_reference.SPLIT_LIBRARY_TABLE and
  every entry names an instantiation that exists and tests that exist (what tests/test_cpu_kernel_variants.py asks of
  libt2v_hip.so); it exports its four launch-side functions and nothing else, and its interface word is libt2v_hip.so's.
* include/t2v_bf16x2.h: a compiler confirms the prototypes the reader read (what tests/test_cpu_cabi.py asks of t2v.h), every
  declared symbol is exported by libt2v_hip.so, and libt2v_hip.so exports no t2v_ symbol that neither header declares."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

import kernel_variants as kv
import split_direct_reference as sdr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nm(*args):
    nm = shutil.which("nm")
    if nm is None:
        pytest.fail("`nm` (binutils) is needed to list the symbols of the libraries and is not on PATH")
    return subprocess.run([nm] + list(args), check=True, capture_output=True, text=True).stdout


def _split_path():
    from text2video_amd import _lib
    return os.path.join(os.path.dirname(_lib.LIB_PATH), "libt2v_split.so")


def test_table_claims_exactly_the_kernels_of_the_split_library(lib_built):
    names, stubs, strange = [], 0, []
    for line in _nm("-C", _split_path()).splitlines():
        if "__device_stub__" not in line:
            continue
        stubs += 1
        sym = line.split(None, 2)[-1]
        sym = sym[5:] if sym.startswith("void ") else sym
        if sym.startswith(("t2v::__device_stub__", "t2v::(anonymous namespace)::__device_stub__")):
            names.append(kv.normalise(sym))
        else:
            strange.append(line)
    assert len(names) == stubs and not strange, strange
    assert len(set(names)) == len(names) == 4, names
    table = set(sdr.SPLIT_LIBRARY_TABLE)
    assert set(names) == table, (sorted(set(names) - table), sorted(table - set(names)))
    # one census per library: no name is claimed twice, and libt2v_hip.so holds none of these kernels
    assert not table & set(kv.TABLE)
    from text2video_amd import _lib
    hip_stubs = _nm("-C", _lib.LIB_PATH)
    for name in table:
        assert name.split("::")[1].split("<")[0] not in hip_stubs, name
    for name, entry in sdr.SPLIT_LIBRARY_TABLE.items():
        assert isinstance(entry, kv.Existing) and entry.nodeids, name
        for nodeid in entry.nodeids:
            path, _, test = nodeid.partition("::")
            with open(os.path.join(ROOT, path)) as f:
                assert re.search(r"^def %s\(" % re.escape(test), f.read(), re.M), "%s: no test %s in %s" % (name, test, path)


def test_split_library_exports_and_interface(lib_built):
    out = _nm("-D", "--defined-only", _split_path())
    exported = sorted(s for s in (ln.split()[-1] for ln in out.splitlines() if ln.strip()) if not s.startswith("_"))
    assert exported == ["t2v_split_interface", "t2v_split_launch_conv", "t2v_split_launch_norm_apply", "t2v_split_launch_pairs"]
    from text2video_amd import _lib
    needed = subprocess.run(["readelf", "-d", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "libt2v_split.so" in needed and "$ORIGIN" in needed
    split = ctypes.CDLL(_split_path())
    split.t2v_split_interface.restype = ctypes.c_int
    word = split.t2v_split_interface()
    assert word >> 16 == 1 and 0 < (word & 0xffff) < 4096, hex(word)      # revision 1, sizeof(ConvKParams)
    # libt2v_hip.so compares the word before every launch: a supported query loads and runs without a device
    d = _lib.ConvDesc(64, 64, 128, 256, 3, 3, 2, 1, _lib.PAD_ZERO, 0, _lib.ACT_NONE, 1.0, 0, _lib.ALGO_DIRECT_BF16X2)
    assert lib_built.t2v_conv_direct_bf16x2_supported(ctypes.byref(d), 128) == 1


def _translation_unit(h):
    tu = ["#include <cstddef>", "#include <type_traits>", '#include "%s"' % h.name]
    for name, (ret, params) in h.functions.items():
        tu.append('static_assert(std::is_same<decltype(&%s), %s (*)(%s)>::value, "%s");' % (name, ret, ", ".join(params), name))
        for t, c in zip([ret] + params, [h.signatures[name][0]] + h.signatures[name][1]):
            if c is not None:
                tu.append('static_assert(sizeof(%s) == %d, "%s: %s");' % (t, ctypes.sizeof(c), name, t))
    return "\n".join(tu) + "\n"


def _compile(text, tmp_path, name):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: it is the check that the header reader read the header right"
    src = tmp_path / name
    src.write_text(text)
    return subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)


def test_a_compiler_confirms_the_companion_header(tmp_path):
    from text2video_amd import _cabi, _lib
    base = _lib._binding.header
    h = _cabi.read_header("t2v_bf16x2.h", base)
    assert list(h.functions) == ["t2v_conv_direct_bf16x2_supported", "t2v_instance_norm_apply_bf16x2"]
    assert not h.structs and not h.opaque and not h.constants          # types and constants are t2v.h's
    assert h.signatures == _lib.BF16X2_SIGNATURES
    assert h.signatures["t2v_conv_direct_bf16x2_supported"] == (ctypes.c_int, [ctypes.POINTER(_lib.ConvDesc), ctypes.c_int])
    assert h.functions["t2v_instance_norm_apply_bf16x2"][1][-3:] == ["long", "int", "int"]
    tu = _translation_unit(h)
    assert tu.count("is_same") == 2
    r = _compile(tu, tmp_path, "bf16x2.cpp")
    assert r.returncode == 0, r.stderr[-4000:]
    wrong = tu.replace("float*, long, int, int)", "float*, int, int, int)", 1)      # one `long` read as `int`
    assert wrong != tu
    r = _compile(wrong, tmp_path, "bf16x2_wrong.cpp")
    assert r.returncode != 0 and "t2v_instance_norm_apply_bf16x2" in r.stderr, r.stderr[-2000:]
    # the reader takes `#include "t2v.h"` only from a companion that is given that header
    with open(os.path.join(ROOT, "include", "t2v_bf16x2.h")) as f:
        text = f.read()
    with pytest.raises(_cabi.HeaderError, match="preprocessor line outside the vocabulary"):
        _cabi.Header(text, "t2v_bf16x2.h")


def test_every_symbol_of_both_headers_is_exported_and_nothing_else(lib_built):
    from text2video_amd import _lib
    with open(os.path.join(ROOT, "include", "t2v_bf16x2.h")) as f:
        declared = set(re.findall(r"\b(t2v_[a-z0-9_]+)\s*\(", f.read()))
    assert declared == set(_lib.BF16X2_SIGNATURES) and len(declared) == 2
    assert not declared & set(_lib.SIGNATURES)
    for name in declared:
        fn = getattr(lib_built, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib.BF16X2_SIGNATURES[name][0], _lib.BF16X2_SIGNATURES[name][1])
    out = _nm("-D", "--defined-only", _lib.LIB_PATH)
    exported = {s for s in (ln.split()[-1] for ln in out.splitlines() if ln.strip()) if s.startswith("t2v_")}
    assert exported == set(_lib.SIGNATURES) | declared, sorted(exported ^ (set(_lib.SIGNATURES) | declared))
