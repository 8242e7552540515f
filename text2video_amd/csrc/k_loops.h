// k_loops.h -- what the wave-specialised GEMM kernels share (conv_igemm.hip, conv_wgrad.hip, winograd_split.hip,
// conv_igemm_split.hip): 4 MFMA waves + 4 loader waves per block, an LDS ring of RING stages, one s_barrier per stage -- the
// loader waves' K loop, and for the fixed-grid ("stream-K") kernels the accumulator hand-over between two blocks.  Also the
// small pieces every kernel with an LDS-DMA loader or more than 64 KiB of dynamic LDS needs (conv_stem.hip and conv_head.hip
// as well): dma16, the XCD-banded tile order, the dynamic-LDS opt-in.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>

#include "t2v_internal.h"

namespace t2v {

typedef unsigned int v4u __attribute__((__vector_size__(16)));   // 16 raw bytes of a b128 buffer load / store

// XCD-banded tile order: block b of nb runs on XCD b % 8 (relied on for speed only), and every XCD gets one contiguous band
// of the nb tiles -- the first nb % 8 bands one tile longer -- so that neighbouring tiles share operands in that XCD's L2.
__host__ __device__ constexpr int xcd_band(int b, int nb) {
    const int xcd = b & 7, idx = b >> 3;
    const int q = nb >> 3, r = nb & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}
constexpr bool xcd_band_permutes(int nb) {   // b -> xcd_band(b, nb) hits every tile 0 .. nb - 1 exactly once
    bool seen[64] = {};
    for (int b = 0; b < nb; ++b) {
        const int t = xcd_band(b, nb);
        if (t < 0 || t >= nb || seen[t]) return false;
        seen[t] = true;
    }
    return true;
}
constexpr bool xcd_band_permutes_up_to(int n) {
    for (int nb = 1; nb <= n; ++nb)
        if (!xcd_band_permutes(nb)) return false;
    return true;
}
static_assert(xcd_band_permutes_up_to(64), "xcd_band: not a permutation of the tiles");

// The opt-in to more than 64 KiB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize) for one kernel, before its
// launch.  The attribute is per device: one flag per (kernel, device), atomic -- two host threads that race set it twice --
// and a device index outside the table sets it every time.  `bytes` is the same at every call for one kernel.  (static: the
// flags stay out of the libraries' exports.)
template <auto Kernel>
static hipError_t optin_dynamic_lds(int bytes) {
    constexpr int kMaxDevices = 64;
    static std::atomic<bool> done[kMaxDevices];
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const bool tabled = dev >= 0 && dev < kMaxDevices;
    if (tabled && done[dev].load(std::memory_order_acquire)) return hipSuccess;
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && tabled) done[dev].store(true, std::memory_order_release);
    return e;
}

// One LDS-DMA instruction through buffer addressing: 64 lanes x 16 B -> 1 KiB at the wave-uniform LDS
// address `lds_dst`; source = base + voff (per lane, bytes) + soff (scalar, bytes).  Lanes with
// voff >= nbytes are out of range and write zeros.  (Device-only builtins: the host pass of hipcc
// must not see them, or it silently drops the kernel stubs.)
__device__ __forceinline__ void dma16(const void* base, unsigned nbytes, char* lds_dst, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, nbytes, 0x00020000);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(srd, (__attribute__((address_space(3))) void*)lds_dst, 16, voff, soff, 0, 0);
#endif
}

// Stage kt+AHEAD is issued into the slot that barrier(kt-1) released; before barrier(kt) the loader only waits (counted
// vmcnt) for stage kt+1, so every DMA has AHEAD stage times to land and is never on the critical path.  Raw s_barrier +
// asm waits: __syncthreads() would drain vmcnt to 0.  Stages past the end re-fetch the last stage (no branches; an empty
// range [kb, kb) fetches stage kb once and meets the MFMA waves at B0 only).  issue_stage(stage, slot) must issue exactly
// LD_PER_WAVE DMA instructions per wave and is called with non-decreasing stages.
template <int RING, int LD_PER_WAVE, class Issue>
__device__ __forceinline__ void loader_k_loop(int kb, int ke, Issue&& issue_stage) {
    constexpr int AHEAD = RING - 1;  // stages in flight beyond the one being computed
#pragma unroll
    for (int st = 0; st < AHEAD; ++st) issue_stage(max(kb, min(kb + st, ke - 1)), st);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AHEAD - 1) * LD_PER_WAVE) : "memory");
    __builtin_amdgcn_s_barrier();  // B0: the first stage has landed
    int slot = AHEAD;              // slot of stage kt+AHEAD (== slot released by barrier(kt-1))
    for (int kt = kb; kt < ke; ++kt) {
        issue_stage(max(kb, min(kt + AHEAD, ke - 1)), slot);
        // stage kt+1 landed; the younger stages (RING >= 3) stay in flight across the barrier
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((AHEAD - 1) * LD_PER_WAVE) : "memory");
        __builtin_amdgcn_s_barrier();  // barrier(kt)
        slot = slot >= RING - 1 ? 0 : slot + 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// ---- the accumulator hand-over of the fixed-grid kernels ---------------------------------------------------------------------
// (conv_igemm.hip: wino_gemm_sk_kernel, wino_gemm_skr_kernel, wino_gemm_skt_kernel; conv_wgrad.hip: wino_wgrad_sk_kernel --
// the only kernels of the library in which one block waits for another.)
//
// A tile cut between two blocks is begun by one and finished by the other.  The PRODUCER runs the tile's first K stages as
// the FIRST piece of its run, writes its accumulators to its own slot of `partial` (handover_publish) and raises its per-wave
// tag (handover_raise) once those stores have left; the CONSUMER gets to the tile as the LAST piece of its run and starts
// its K loop from those accumulators instead of zeros (handover_fetch).  Wave `wid` of the producer wrote what wave `wid` of
// the consumer reads: both run the same tile configuration, so the element -> (wave, register, lane) mapping is the tile's
// own.  The producer is a block of the same XCD with a lower index (blockIdx - 8, or half the XCD's blocks lower): it was
// dispatched before the consumer and published before anything it waits for itself, so nobody waits for a block that
// started after it and the wait is normally over before it starts.
//   * The wait is bounded by TIME -- one second of the 100 MHz constant clock -- not by a poll count.  If the tag is still
//     missing then, something is broken: the consumer poisons its tile with NaNs and raises the sticky error word `err`
//     (pinned host memory, t2v_internal.h: async_error_word); the host reports T2V_ERR_HANDOVER from its next entry point
//     and falls back to one block per tile.  No hung queue, no silently wrong frame.
//   * The tag is unique per launch (sk_handover), so flags left by earlier launches never match.  A captured graph re-issues
//     the SAME tag on every replay: the consumer therefore clears the flag it has taken, and the replay starts clean.
//   * The slot crosses the XCDs' L2s in general.  Write-through (sc1) 16-byte buffer stores on the producer's side and sc1
//     loads on the consumer's are the pair that is coherent between them inside one launch; the tag is raised only after
//     s_waitcnt vmcnt(0) says those stores have left for memory.
//   * A slot holds PW floats per wave, TM x TN fragments of 1024 at scalar offsets off one SRD.  The scratch buffer's layout
//     is sk_handover()'s (conv_igemm.hip).
constexpr unsigned long long kHandoverTimeoutTicks = 100000000ull;

// Poll the producer wave's tag with agent-scope loads until it shows this launch's value.  Returns true on a time-out.
__device__ __forceinline__ bool handover_wait(const unsigned long long* flag, unsigned long long tag, unsigned* err, int lane) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag) return false;
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        __builtin_amdgcn_s_sleep(4);
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == tag) return false;
        if (wall_clock64() - t0 > kHandoverTimeoutTicks) break;
    }
    if (err && lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return true;
}

// Consumer: take over the accumulators that wave `wid` of block `src` published (NaNs after a time-out) and clear its flag.
template <int PW, int TM, int TN, class Acc>
__device__ __forceinline__ void handover_fetch(const SkHandover& h, int src, int wid, int lane, Acc (&acc)[TM][TN]) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PW >= TM * TN * 1024, "hand-over slot too small for this tile");
    const unsigned long long* fl = h.flags + src * 4 + wid;
    const bool timed_out = handover_wait(fl, h.tag, h.err, lane);
    if (lane == 0) __hip_atomic_store(const_cast<unsigned long long*>(fl), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const __amdgpu_buffer_rsrc_t srd = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float*>(h.partial) + (size_t)(src * 4 + wid) * PW, 0, PW * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                auto raw = __builtin_amdgcn_raw_buffer_load_b128(srd, lane * 16, ((i * TN + j) * 4 + q) * 1024, /*sc1*/ 16);
                float v[4];
                __builtin_memcpy(v, &raw, 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[i][j][q * 4 + e] = timed_out ? __builtin_nanf("") : v[e];
            }
#endif
}

// Producer: write this wave's accumulators to its slot.  The tag follows at the wave's next wait point (handover_raise), so
// that the stores drain while the loaders fetch the next tile's first stage.
template <int PW, int TM, int TN, class Acc>
__device__ __forceinline__ void handover_publish(const SkHandover& h, int wid, int lane, const Acc (&acc)[TM][TN]) {
#if defined(__HIP_DEVICE_COMPILE__)
    static_assert(PW >= TM * TN * 1024, "hand-over slot too small for this tile");
    const __amdgpu_buffer_rsrc_t srd =
        __builtin_amdgcn_make_buffer_rsrc(h.partial + (size_t)(blockIdx.x * 4 + wid) * PW, 0, PW * 4, 0x00020000);
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[i][j][q * 4 + e];
                v4u raw;
                __builtin_memcpy(&raw, v, 16);
                __builtin_amdgcn_raw_buffer_store_b128(raw, srd, lane * 16, ((i * TN + j) * 4 + q) * 1024, /*sc1*/ 16);
            }
#endif
}

// Producer: the published stores have left for memory -- raise this wave's tag.
__device__ __forceinline__ void handover_raise(const SkHandover& h, int wid, int lane) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(h.flags + blockIdx.x * 4 + wid, h.tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace t2v
