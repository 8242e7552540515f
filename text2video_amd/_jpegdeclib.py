"""ctypes binding of libt2v_jpegdec.so (C ABI declared in include/t2v_jpeg_decode.h): the GPU JPEG decoder.

A library of its own beside libt2v_hip.so and libt2v_jpeg.so: raw device pointers and a stream in, no context.  No
fallback: if the shared library is missing or does not export the declared symbols, load() raises.  Build it with
`python __graft_entry__.py` or `make -C text2video_amd/csrc`.
"""
import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libt2v_jpegdec.so")

T2V_JPEGDEC_OK = 0
ABI_VERSION = 1
MIN_DIM, MAX_DIM, MAX_IMAGES = 8, 2048, 1024     # T2V_JPEGDEC_MIN_DIM, T2V_JPEGDEC_MAX_DIM, T2V_JPEGDEC_MAX_IMAGES
NOT_CONVERGED, CORRUPT = 1, 2                    # bits of the per-image status word

# name -> (restype, argtypes); every symbol include/t2v_jpeg_decode.h declares
SIGNATURES = {
    "t2v_jpegdec_abi_version": (c_int, []),
    "t2v_jpegdec_last_error": (c_char_p, []),
    "t2v_jpegdec_supported": (c_int, [c_int, c_int, c_int]),
    "t2v_jpegdec_table_bytes": (c_size_t, []),
    "t2v_jpegdec_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_size_t]),
    "t2v_jpegdec_decode_u8": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p,
                                      c_void_p, c_int, c_void_p]),
}

_lib = None
_load_lock = threading.RLock()


def load():
    """Load libt2v_jpegdec.so and bind every declared symbol.  Raises if anything is missing.  libt2v_hip.so is loaded first
    (text2video_amd._lib.load): that settles which HIP runtime the process uses, the one all the libraries then share."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libt2v_jpegdec.so not found at %s: the GPU JPEG decoder is required for --gpu_decode / ops.jpeg_decode_u8 "
                "(no fallback).  Build it with `python __graft_entry__.py` or `make -C text2video_amd/csrc`." % LIB_PATH)
        from . import _lib as _hiplib
        _hiplib.load()
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.t2v_jpegdec_abi_version() != ABI_VERSION:
            raise RuntimeError("libt2v_jpegdec.so ABI %d != binding ABI %d" % (lib.t2v_jpegdec_abi_version(), ABI_VERSION))
        _lib = lib
        return lib


def check(status, what=""):
    if status != T2V_JPEGDEC_OK:
        msg = load().t2v_jpegdec_last_error()
        raise RuntimeError("t2v_jpegdec %s failed (status %d): %s" % (what, status, msg.decode() if msg else "?"))
