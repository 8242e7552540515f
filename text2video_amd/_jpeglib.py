"""ctypes binding of libt2v_jpeg.so (C ABI declared in include/t2v_jpeg.h): the GPU JPEG encoder.

A library of its own beside libt2v_hip.so: raw device pointers and a stream in, no context.  No fallback: if the shared
library is missing or does not export the declared symbols, load() raises.  Build it with `python __graft_entry__.py` or
`make -C text2video_amd/csrc`.
"""
import ctypes
import os
import threading
from ctypes import c_char_p, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libt2v_jpeg.so")

T2V_JPEG_OK = 0
ABI_VERSION = 1
MIN_DIM, MAX_DIM, MAX_IMAGES = 8, 2048, 1024     # T2V_JPEG_MIN_DIM, T2V_JPEG_MAX_DIM, T2V_JPEG_MAX_IMAGES

# name -> (restype, argtypes); every symbol include/t2v_jpeg.h declares
SIGNATURES = {
    "t2v_jpeg_abi_version": (c_int, []),
    "t2v_jpeg_last_error": (c_char_p, []),
    "t2v_jpeg_supported": (c_int, [c_int, c_int]),
    "t2v_jpeg_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "t2v_jpeg_scan_capacity": (c_size_t, [c_int, c_int]),
    "t2v_jpeg_stage_u8": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_int, c_long, c_void_p]),
    "t2v_jpeg_encode_u8": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_size_t,
                                   c_void_p]),
}

_lib = None
_load_lock = threading.RLock()


def load():
    """Load libt2v_jpeg.so and bind every declared symbol.  Raises if anything is missing.  libt2v_hip.so is loaded first
    (text2video_amd._lib.load): that settles which HIP runtime the process uses, the one both libraries then share."""
    global _lib
    if _lib is not None:
        return _lib
    with _load_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "libt2v_jpeg.so not found at %s: the GPU JPEG encoder is required for --gpu_jpeg / ops.jpeg_encode_u8 "
                "(no fallback).  Build it with `python __graft_entry__.py` or `make -C text2video_amd/csrc`." % LIB_PATH)
        from . import _lib as _hiplib
        _hiplib.load()
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        if lib.t2v_jpeg_abi_version() != ABI_VERSION:
            raise RuntimeError("libt2v_jpeg.so ABI %d != binding ABI %d" % (lib.t2v_jpeg_abi_version(), ABI_VERSION))
        _lib = lib
        return lib


def check(status, what=""):
    if status != T2V_JPEG_OK:
        msg = load().t2v_jpeg_last_error()
        raise RuntimeError("t2v_jpeg %s failed (status %d): %s" % (what, status, msg.decode() if msg else "?"))
