"""CPU tests (no GPU) of text2video_amd/_cabi.py, the reader the ctypes bindings take the C ABI from: a compiler confirms
what it read from the three headers (types of every entry point, layout of every struct, value of every constant), and the
reader refuses what is outside its vocabulary instead of guessing."""
import ctypes
import os
import shutil
import subprocess
import sys

import pytest

from text2video_amd import _cabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"t2v.h": (116, 4), "t2v_jpeg.h": (7, 0), "t2v_jpeg_decode.h": (6, 0)}      # entry points, structs


def _translation_unit(headers):
    """C++ that compiles only if every parsed prototype, struct layout, constant and ctypes size is the header's"""
    tu = ["#include <cstddef>", "#include <type_traits>"] + ['#include "%s"' % h.name for h in headers]
    for h in headers:
        for name, (ret, params) in h.functions.items():
            tu.append('static_assert(std::is_same<decltype(&%s), %s (*)(%s)>::value, "%s");' % (name, ret, ", ".join(params), name))
            for t, c in zip([ret] + params, [h.signatures[name][0]] + h.signatures[name][1]):
                if c is not None:     # the ctypes object passes as many bytes as the C type takes
                    tu.append('static_assert(sizeof(%s) == %d, "%s: %s");' % (t, ctypes.sizeof(c), name, t))
        for name, cls in h.structs.items():
            tu.append('static_assert(sizeof(%s) == %d, "sizeof %s");' % (name, ctypes.sizeof(cls), name))
            for field, _ in cls._fields_:
                f = getattr(cls, field)
                tu.append('static_assert(offsetof(%s, %s) == %d && sizeof(%s::%s) == %d, "%s.%s");'
                          % (name, field, f.offset, name, field, f.size, name, field))
        for name, value in h.constants.items():
            tu.append('static_assert(%s == %d, "%s");' % (name, value, name))
    return "\n".join(tu) + "\n"


def _compile(text, tmp_path, name):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed: it is the check that the header reader read the headers right"
    src = tmp_path / name
    src.write_text(text)
    return subprocess.run([gxx, "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                          capture_output=True, text=True)


def test_a_compiler_confirms_what_the_reader_read(tmp_path):
    headers = [_cabi.read_header(n) for n in HEADERS]
    for h in headers:
        assert (len(h.functions), len(h.structs)) == HEADERS[h.name] and list(h.signatures) == list(h.functions)
        assert h.constants[h.name[:-2].replace("_decode", "dec").upper() + "_ABI_VERSION"] >= 1
    tu = _translation_unit(headers)
    assert tu.count("is_same") == 129 and tu.count("offsetof") == 14 + 14 + 4 + 10
    r = _compile(tu, tmp_path, "abi.cpp")
    assert r.returncode == 0, r.stderr[-4000:]
    # the check has teeth: one `long` read as `int`, one field moved, one constant off by one -- each is a compile error
    h = headers[0]
    ret, params = h.functions["t2v_conv2d_forward_winograd_batch_stages"]
    assert params[6] == "long"
    for wrong, word in ((tu.replace("int, long, const float*, const float*, float*", "int, int, const float*, const float*, float*", 1),
                         "t2v_conv2d_forward_winograd_batch_stages"),
                        (tu.replace("offsetof(t2v_gen_io, out) == 40", "offsetof(t2v_gen_io, out) == 36"), "t2v_gen_io.out"),
                        (tu.replace("static_assert(T2V_ERR_HANDOVER == -4", "static_assert(T2V_ERR_HANDOVER == -3"), "T2V_ERR_HANDOVER")):
        assert wrong != tu
        r = _compile(wrong, tmp_path, "abi_wrong.cpp")
        assert r.returncode != 0 and word in r.stderr, (word, r.stderr[-2000:])


def test_the_modules_bind_what_the_reader_read():
    from text2video_amd import _jpegdeclib, _jpeglib, _lib, ops
    h = _lib._binding.header
    assert _lib.SIGNATURES is h.signatures and _lib.ConvDesc is h.structs["t2v_conv_desc"] and _lib.GenIO is h.structs["t2v_gen_io"]
    assert _lib.SIGNATURES["t2v_conv_out_dims"] == (ctypes.c_int, [ctypes.POINTER(_lib.ConvDesc), ctypes.POINTER(ctypes.c_int),
                                                                     ctypes.POINTER(ctypes.c_int)])
    assert _lib.SIGNATURES["t2v_last_error"] == (ctypes.c_char_p, []) and _lib.SIGNATURES["t2v_reload_env"] == (None, [])
    assert _lib.SIGNATURES["t2v_device_malloc"][1] == [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
    assert _lib.SIGNATURES["t2v_train_visuals_u8"][1][2] is ctypes.c_void_p      # `const float* const*`: an array passed in
    assert (_lib.ABI_VERSION, _lib.T2V_OK, _lib.MAX_BATCH, _lib.ALGO_POLYPHASE_BF16X2, _lib.COPY_D2D) == (h.constants["T2V_ABI_VERSION"], 0, 8, 5, 3)
    assert (ops.RESAMPLE_MAX_TAPS, ops.METRICS_MAX_BOXES, ops.METRICS_MAX_SIDE) == (33, 3, 8192)
    assert (_jpeglib.MIN_DIM, _jpeglib.MAX_DIM, _jpeglib.MAX_IMAGES, _jpeglib.T2V_JPEG_OK) == (8, 2048, 1024, 0)
    assert (_jpegdeclib.NOT_CONVERGED, _jpegdeclib.CORRUPT, _jpegdeclib.T2V_JPEGDEC_OK) == (1, 2, 0)
    assert _jpeglib.check is not _jpegdeclib.check and _jpeglib.load is not _lib.load
    # the lean frame loop loads the binding without torch or numpy
    r = subprocess.run([sys.executable, "-c", "import sys; from text2video_amd import _lib, _jpeglib, _jpegdeclib; "
                        "assert not {'torch', 'numpy'} & set(sys.modules), sorted(sys.modules)"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_a_missing_header_or_library_says_where(tmp_path, monkeypatch):
    monkeypatch.setattr(_cabi, "INCLUDE_DIR", str(tmp_path))
    with pytest.raises(RuntimeError, match=r"header .*t2v\.h not found"):
        _cabi.read_header("t2v.h")
    (tmp_path / "x.h").write_text("#define X_ABI_VERSION 3\nint x_abi_version(void);\nconst char* x_last_error(void);\n")
    b = _cabi.bind(str(tmp_path / "libx.so"), "x.h", "x_abi_version", "X_ABI_VERSION", "it is required (no fallback)")
    assert b.abi_version == 3 and b.prefix == "x" and list(b.signatures) == ["x_abi_version", "x_last_error"]
    with pytest.raises(RuntimeError, match=r"libx\.so not found at .*no fallback.*Build it with"):
        b.load()


REFUSED = {
    "unsigned parameter": ("int f(unsigned n);", "unsigned"),
    "unsigned int parameter": ("int f(unsigned int n);", "unsigned int"),
    "function-pointer parameter": ("int f(void* ctx, void (*done)(int status));", "int f(void* ctx, void (*done)(int status))"),
    "variadic": ("int f(const char* fmt, ...);", "..."),
    "parameter without a name": ("int f(int a, float);", "float"),
    "pointer parameter without a name": ("int f(const float*);", "const float*"),
    "empty parameter list": ("int f();", "int f()"),
    "struct by value": ("typedef struct { int a; } s_t;\nint f(s_t s);", "`s_t` by value"),
    "unknown struct pointer": ("int f(const other_t* s);", "other_t"),
    "array field": ("typedef struct { int a; float b[4]; } s_t;", "float b[4]"),
    "bit field": ("typedef struct { int a : 3; } s_t;", "int a : 3"),
    "two pointer declarators": ("typedef struct { float *a, *b; } s_t;", "float *a, *b"),
    "non-integer define": ("#define X 1.5\nint f(void);", "#define X 1.5"),
    "function-like define": ("#define F(x) 1\nint f(void);", "#define F(x) 1"),
    "conditional code": ("#if 0\nint f(void);\n#endif", "#if 0"),
    "enumerator expression": ("enum { A = 1 << 3 };", "1 << 3"),
    "missing semicolon": ("int f(int a)\nint g(int b);", "int f(int a) int g(int b)"),
    "missing last semicolon": ("int f(int a);\nint g(int b)", "int g(int b)"),
    "unknown return type": ("bool f(void);", "bool"),
}


@pytest.mark.parametrize("case", list(REFUSED), ids=lambda c: c.replace(" ", "_"))
def test_the_reader_refuses_what_it_does_not_know(case):
    text, named = REFUSED[case]
    with pytest.raises(_cabi.HeaderError) as e:
        _cabi.Header(text, "case.h")
    assert str(e.value).startswith("case.h: ") and named in str(e.value), str(e.value)


def test_the_reader_accepts_its_vocabulary():
    h = _cabi.Header("""
        /* a header
         * like the tree's */
        #ifndef CASE_H_
        #define CASE_H_
        #include <stddef.h>
        #ifdef __cplusplus
        extern "C" {
        #endif
        #define CASE_ABI_VERSION 7
        #define CASE_MASK 0x1F
        typedef enum { CASE_OK = 0, CASE_ERR_A = -1, CASE_ERR_B = -7, CASE_NEXT, CASE_AFTER /* -5 */ } case_status;
        enum { CASE_FIRST, CASE_SECOND, CASE_TEN = 10, CASE_ELEVEN, };
        typedef struct case_ctx case_ctx;
        typedef struct {
            int H, W;        /* two declarators; a comment with a ; and a } in it */
            float scale;
            const float* w;  // and a line comment
            size_t n;
            double d; long l;
        } case_desc;
        int case_create(case_ctx** out, int device);
        int
        case_run(case_ctx* ctx,          /* the context, ( or NULL ) */
                 const case_desc* d, /* a comment , with ( a comma ) and parentheses */ int* Hout,
                 const float* const* panels, long stride, double lr, size_t n, const uint8_t* src, void** out,
                 float x);
        const char* case_last_error(void);
        void case_reset(void);
        size_t case_bytes(const case_desc *d , int n);
        #ifdef __cplusplus
        }
        #endif
        #endif /* CASE_H_ */
        """, "case.h")
    assert h.constants == {"CASE_ABI_VERSION": 7, "CASE_MASK": 31, "CASE_OK": 0, "CASE_ERR_A": -1, "CASE_ERR_B": -7, "CASE_NEXT": -6,
                           "CASE_AFTER": -5, "CASE_FIRST": 0, "CASE_SECOND": 1, "CASE_TEN": 10, "CASE_ELEVEN": 11}
    assert h.fields == {"case_desc": [("int", "H"), ("int", "W"), ("float", "scale"), ("const float*", "w"), ("size_t", "n"),
                                      ("double", "d"), ("long", "l")]}
    desc = h.structs["case_desc"]
    assert desc._fields_ == [("H", ctypes.c_int), ("W", ctypes.c_int), ("scale", ctypes.c_float), ("w", ctypes.c_void_p),
                             ("n", ctypes.c_size_t), ("d", ctypes.c_double), ("l", ctypes.c_long)]
    assert h.opaque == {"case_ctx"}
    assert h.functions == {
        "case_create": ("int", ["case_ctx**", "int"]),
        "case_run": ("int", ["case_ctx*", "const case_desc*", "int*", "const float* const*", "long", "double", "size_t",
                             "const uint8_t*", "void**", "float"]),
        "case_last_error": ("const char*", []), "case_reset": ("void", []), "case_bytes": ("size_t", ["const case_desc*", "int"])}
    assert list(h.functions) == ["case_create", "case_run", "case_last_error", "case_reset", "case_bytes"]
    P, vp = ctypes.POINTER, ctypes.c_void_p
    assert h.signatures == {
        "case_create": (ctypes.c_int, [P(vp), ctypes.c_int]),
        "case_run": (ctypes.c_int, [vp, P(desc), P(ctypes.c_int), vp, ctypes.c_long, ctypes.c_double, ctypes.c_size_t, vp, P(vp),
                                    ctypes.c_float]),
        "case_last_error": (ctypes.c_char_p, []), "case_reset": (None, []), "case_bytes": (ctypes.c_size_t, [P(desc), ctypes.c_int])}
