"""ctypes binding of libt2v_gradfold.so, the fold of a flat gradient bucket into the accumulator of an optimiser step that
walks several clips per rank (t2v_grad_fold); its C ABI is read from include/t2v_grad_fold.h (_cabi.py).

A library of its own beside libt2v_hip.so, which it links: it takes that library's context, and a refusal leaves its message
where t2v_last_error reads it, so statuses go through _lib.check.  No fallback: if the shared library is missing or does not
export the declared symbols, load() raises.  Build it with `python __graft_entry__.py` or `make -C text2video_amd/csrc`.
"""
import os

from . import _cabi, _lib

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libt2v_gradfold.so")
# libt2v_hip.so is loaded first (_lib.load): that settles which HIP runtime the process uses, the one both libraries share
_binding = _cabi.bind(LIB_PATH, "t2v_grad_fold.h", "t2v_grad_fold_abi_version", "T2V_GRAD_FOLD_ABI_VERSION",
                      "the gradient fold is required for a train step of several clips per rank (no fallback)",
                      first=_lib.load)
SIGNATURES = _binding.signatures      # name -> (restype, argtypes); every symbol the header declares, in its order
load = _binding.load
check = _lib.check                    # (the message is libt2v_hip.so's t2v_last_error)
ABI_VERSION = _binding.header.constants["T2V_GRAD_FOLD_ABI_VERSION"]
OPEN, ADD, CLOSE = (_binding.header.constants["T2V_GRAD_FOLD_" + k] for k in ("OPEN", "ADD", "CLOSE"))
