"""ctypes binding of libt2v_hip.so.  include/t2v.h is the one description of the C ABI: signatures, structs and constants
are read from it (text2video_amd/_cabi.py), nothing is repeated here.

The product path has NO fallback: if the shared library is missing or does not export the
expected symbols, importing/using it raises.  Build it with `python __graft_entry__.py` or
`make -C text2video_amd/csrc`.
"""
import ctypes
import os
from ctypes import c_void_p

from . import _cabi

_HERE = os.path.dirname(os.path.abspath(__file__))
# (T2V_LIBRARY: another build of the same ABI -- same-box A/B runs of a kernel change, scripts/ only)
LIB_PATH = os.environ.get("T2V_LIBRARY") or os.path.join(_HERE, "lib", "libt2v_hip.so")


def _hip_runtime_first():
    # torch must initialise first: it bundles its own libamdhip64.so (same soname as /opt/rocm's).
    # Loaded in this order the one HIP runtime of the process is torch's and device pointers /
    # streams are shared; the other order would put two HIP runtimes in one process.
    # (The torch-free frame loop of vid2vid/test.py -- _xp.LEAN -- never imports torch: the library then brings the
    # ROCm installation's runtime in through its own RUNPATH.)
    from ._xp import LEAN
    if not LEAN:
        import torch  # noqa: F401
        hip_rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if os.path.exists(hip_rt):
            ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)
    elif os.environ.get("T2V_HIP_RUNTIME", "torch") != "system":
        # torch-free process, same HIP runtime: the copy PyTorch bundles (located without importing torch) -- the one every
        # measurement and test of this tree ran on; T2V_HIP_RUNTIME=system takes the ROCm installation's instead
        import importlib.util
        spec = importlib.util.find_spec("torch")
        hip_rt = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so") if spec and spec.origin else ""
        if os.path.exists(hip_rt):
            ctypes.CDLL(hip_rt, mode=ctypes.RTLD_GLOBAL)


_binding = _cabi.bind(LIB_PATH, "t2v.h", "t2v_abi_version", "T2V_ABI_VERSION",
                      "the HIP extension is required (no CPU fallback)", first=_hip_runtime_first)
SIGNATURES = _binding.signatures      # name -> (restype, argtypes); every symbol include/t2v.h declares, in its order
# include/t2v_bf16x2.h: the entry points of the split-bf16 direct convolution (T2V_ALGO_DIRECT_BF16X2), same library
BF16X2_SIGNATURES = _binding.companion("t2v_bf16x2.h").signatures
load, check = _binding.load, _binding.check
ConvDesc, GenDesc, Layer, GenIO = (_binding.header.structs[s] for s in ("t2v_conv_desc", "t2v_gen_desc", "t2v_layer", "t2v_gen_io"))
# every T2V_* constant of the header without the prefix: ABI_VERSION, PAD_*, ACT_*, ALGO_*, MAX_BATCH, COPY_*, VISUALS_*,
# RESAMPLE_MAX_TAPS, METRICS_MAX_BOXES, METRICS_MAX_SIDE, ERR_*, GEMM_*, ...
globals().update(_binding.constants("T2V_"))
T2V_OK = _binding.header.constants["T2V_OK"]
# values of t2v_gen_desc.conv_algo, which the header describes in a comment and does not name
CONV_ALGO_BF16X2 = 3            # the selection of 0 with its F(4x4,3x3) trunk in split-bf16 arithmetic
CONV_ALGO_BF16X2_STRIDE2 = 4    # 3, and the polyphase stride-2 / transposed layers in split-bf16 as well
CONV_ALGO_BF16X2_OUTER = 5      # 4, and the stride-2 / transposed layers that stay direct (128 <-> 256) in split-bf16 as well


class Context:
    """Owns a t2v_ctx bound to one device."""

    def __init__(self, device=0):
        self.lib = load()
        self._h = c_void_p()
        check(self.lib.t2v_create(ctypes.byref(self._h), int(device)), "t2v_create")
        self.device = int(device)

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self.lib.t2v_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
