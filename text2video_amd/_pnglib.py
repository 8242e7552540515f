"""ctypes binding of libt2v_png.so, the GPU PNG writer; its C ABI is read from include/t2v_png.h (_cabi.py).

A library of its own beside libt2v_hip.so: raw device pointers and a stream in, no context.  No fallback: if the shared
library is missing or does not export the declared symbols, load() raises.  Build it with `python __graft_entry__.py` or
`make -C text2video_amd/csrc`.
"""
import os

from . import _cabi, _lib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libt2v_png.so")
# libt2v_hip.so is loaded first (_lib.load): that settles which HIP runtime the process uses, the one both libraries share
_binding = _cabi.bind(LIB_PATH, "t2v_png.h", "t2v_png_abi_version", "T2V_PNG_ABI_VERSION",
                      "the GPU PNG writer is required for --frame_format png / ops.png_encode_u8 (no fallback)", first=_lib.load)
SIGNATURES = _binding.signatures      # name -> (restype, argtypes); every symbol the header declares, in its order
load, check = _binding.load, _binding.check
globals().update(_binding.constants("T2V_PNG_"))      # ABI_VERSION, MIN_DIM, MAX_DIM, MAX_IMAGES, BAND_ROWS, OK, ERR_*
