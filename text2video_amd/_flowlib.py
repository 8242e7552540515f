"""ctypes binding of libt2v_flow.so, the refined dense optical flow (t2v_optical_flow_refined); its C ABI is read from
include/t2v_flow_refine.h (_cabi.py).

A library of its own beside libt2v_hip.so, which it links: it takes that library's context, and a refusal leaves its message
where t2v_last_error reads it, so statuses go through _lib.check.  No fallback: if the shared library is missing or does not
export the declared symbols, load() raises.  Build it with `python __graft_entry__.py` or `make -C text2video_amd/csrc`.
"""
import os

from . import _cabi, _lib

# (T2V_FLOW_LIBRARY: another build of the same ABI -- same-box A/B runs of a kernel change, scripts/ only)
LIB_PATH = os.environ.get("T2V_FLOW_LIBRARY") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libt2v_flow.so")
# libt2v_hip.so is loaded first (_lib.load): that settles which HIP runtime the process uses, the one both libraries share
_binding = _cabi.bind(LIB_PATH, "t2v_flow_refine.h", "t2v_flow_refine_abi_version", "T2V_FLOW_REFINE_ABI_VERSION",
                      "the refined optical flow is required for ops.optical_flow(..., refine_iters=N) (no fallback)",
                      first=_lib.load)
SIGNATURES = _binding.signatures      # name -> (restype, argtypes); every symbol the header declares, in its order
load = _binding.load
check = _lib.check                    # (the message is libt2v_hip.so's t2v_last_error)
ABI_VERSION = _binding.header.constants["T2V_FLOW_REFINE_ABI_VERSION"]
MAX_FUSED = _binding.header.constants["T2V_FLOW_REFINE_MAX_FUSED"]      # the largest iters_per_launch
