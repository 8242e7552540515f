// libt2v_jpegdec.so (include/t2v_jpeg_decode.h): baseline JPEG decoding on the GPU, byte for byte the RGB array
// libjpeg-turbo / Pillow gives.  DESIGN.md section 4.11 has the rules and the synchronisation scheme.
//
// One call = one memset (the coefficients) and eight launches, the same for every content:
//   1. jpegdec_blind_kernel    one thread per 128-byte subsequence of a scan, 256 per workgroup, the workgroup's bytes and
//                              the image's tables in LDS.  Subsequence 0 is decoded from the true start state, every other
//                              one from the blind state (its first data bit, block 0, DC); the end state and the number of
//                              blocks completed go to state buffer A as one 64-bit word.  Also resets the image's status.
//   2. jpegdec_sync_kernel     A -> B: up to kRounds rounds inside the workgroup.  In a round every thread decodes its
//                              subsequence again from the end state its predecessor holds (the workgroup's first thread: the
//                              one the previous launch left for the subsequence before it); the rounds end early once no
//                              thread of the workgroup changed its state.
//   3. jpegdec_sync_kernel     B -> A: the same again, now that every workgroup's input is its predecessor's settled state.
//   4. jpegdec_scan_kernel     one workgroup per image: exclusive prefix sum of the block counts = every subsequence's first
//                              block ordinal; a total other than the image's block count, or a chain that ends inside a
//                              block, sets T2V_JPEGDEC_CORRUPT.
//   5. jpegdec_write_kernel    the same walk from the stored predecessor state, now writing int16 coefficients in natural
//                              order (DC as differences) at the block ordinals.  Its end state is compared with the stored
//                              one: a difference means the chain is no fixed point and sets T2V_JPEGDEC_NOT_CONVERGED.
//   6. jpegdec_dc_kernel       one workgroup per image and component: prefix sum of the DC differences in coding order.
//   7. jpegdec_idct_kernel     eight threads per block: dequantise, "islow" columns then rows through LDS, + 128, clamp, into
//                              the component's plane (block-grid size).
//   8. jpegdec_colour_kernel   one thread per pixel: fancy up-sampling of Cb and Cr from the planes, clamped to their real
//                              extent, and the fixed-point YCbCr -> RGB conversion.
// All four decoding kernels share one symbol walk (run_subsequence) with two sinks, so a state compared is a state written.
// Integer arithmetic only, no float, no inline assembly; every store is a vector store.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/t2v_jpeg_decode.h"

namespace {

thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define JPEGDEC_HIP_CHECK(expr)                                                                       \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));           \
            return T2V_JPEGDEC_ERR_HIP;                                                               \
        }                                                                                             \
    } while (0)
#define JPEGDEC_REQUIRE(cond, ...)           \
    do {                                     \
        if (!(cond)) {                       \
            set_error(__VA_ARGS__);          \
            return T2V_JPEGDEC_ERR_INVALID;  \
        }                                    \
    } while (0)

constexpr int kSubseqBytes = 128;      // one thread's share of a scan: 1024 bits (tests/jpeg_decode_reference.py: SUBSEQ_BYTES)
constexpr int kRounds = 22;            // correction rounds per synchronisation launch: twice the most a 512 x 512 frame needed
constexpr int kThreads = 256;          // subsequences per workgroup of the decoding kernels
constexpr int kRowStride = 132;        // bytes between subsequences in LDS: 33 dwords, so equal offsets fall on 32 different banks
constexpr int kRows = kThreads + 1;    // a symbol that starts in the last subsequence may end in the next one
constexpr int kSpanBytes = kRows * kSubseqBytes;
constexpr int kTableBytes = 3968;      // t2v_jpegdec_table_bytes()
constexpr int kQuantBytes = 384;
constexpr int kHuffBytes = 896;
constexpr size_t kMaxScanCapacity = (size_t)1 << 28;      // bit positions fit 32 bits

__device__ const uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ---------------------------------------------------------------------------------------------------------------------
// geometry and workspace
// ---------------------------------------------------------------------------------------------------------------------
struct Geom {
    int H, W;
    int hs, vs;            // Y's sampling factors
    int ny, bpm;           // Y blocks and all blocks per MCU
    int mw, mh, nmcu;      // MCU grid
    int nblocks;           // per image, in coding order
    int yw, yh;            // Y plane at block-grid size
    int cwp, chp;          // a chroma plane at block-grid size
    int cw, ch;            // the chroma planes' real extent: ceil(W / hs) x ceil(H / vs)
    size_t plane_bytes;    // Y + Cb + Cr per image
    int nsub, nwg;         // subsequences per image, workgroups of kThreads of them
};

bool supported(int H, int W, int sampling) {
    return H >= T2V_JPEGDEC_MIN_DIM && H <= T2V_JPEGDEC_MAX_DIM && W >= T2V_JPEGDEC_MIN_DIM && W <= T2V_JPEGDEC_MAX_DIM &&
           sampling >= 0 && sampling <= 2;
}

bool capacity_ok(size_t cap) { return cap >= 16 && cap <= kMaxScanCapacity && cap % 16 == 0; }

Geom geometry(int H, int W, int sampling, size_t scan_capacity) {
    Geom g;
    g.H = H;
    g.W = W;
    g.hs = sampling == 0 ? 1 : 2;
    g.vs = sampling == 2 ? 2 : 1;
    g.ny = g.hs * g.vs;
    g.bpm = g.ny + 2;
    g.mw = (W + 8 * g.hs - 1) / (8 * g.hs);
    g.mh = (H + 8 * g.vs - 1) / (8 * g.vs);
    g.nmcu = g.mw * g.mh;
    g.nblocks = g.nmcu * g.bpm;
    g.yw = g.mw * 8 * g.hs;
    g.yh = g.mh * 8 * g.vs;
    g.cwp = g.mw * 8;
    g.chp = g.mh * 8;
    g.cw = (W + g.hs - 1) / g.hs;
    g.ch = (H + g.vs - 1) / g.vs;
    g.plane_bytes = (size_t)g.yw * g.yh + 2 * (size_t)g.cwp * g.chp;
    g.nsub = (int)((scan_capacity + kSubseqBytes - 1) / kSubseqBytes);
    g.nwg = (g.nsub + kThreads - 1) / kThreads;
    return g;
}

struct Workspace {
    uint64_t* state_a;     // [nimg][nsub]
    uint64_t* state_b;
    uint32_t* first;       // [nimg][nsub]
    int16_t* coef;         // [nimg][nblocks][64]
    uint8_t* planes;       // [nimg][plane_bytes]
    size_t coef_bytes;
    size_t bytes;
};

Workspace carve(const Geom& g, int nimg, void* base) {
    auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    Workspace w;
    size_t at = 0;
    uint8_t* p = (uint8_t*)base;
    const size_t states = up((size_t)nimg * g.nsub * sizeof(uint64_t));
    w.state_a = (uint64_t*)(p + at);
    at += states;
    w.state_b = (uint64_t*)(p + at);
    at += states;
    w.first = (uint32_t*)(p + at);
    at += up((size_t)nimg * g.nsub * sizeof(uint32_t));
    w.coef = (int16_t*)(p + at);
    w.coef_bytes = (size_t)nimg * g.nblocks * 64 * sizeof(int16_t);
    at += up(w.coef_bytes);
    w.planes = p + at;
    at += up((size_t)nimg * g.plane_bytes);
    w.bytes = at;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// the symbol walk
// ---------------------------------------------------------------------------------------------------------------------
// A state: the raw bit position p = 8 B + o of the next bit (B never the stuffed 00 behind an FF), the block index within the
// MCU b and the zigzag index of the next coefficient k.  Packed with the blocks completed n into one word, so that a state
// is read and written whole.
__device__ __forceinline__ uint64_t pack_state(uint32_t p, uint32_t b, uint32_t k, uint32_t n) {
    return (uint64_t)p | ((uint64_t)(k & 63u) << 32) | ((uint64_t)(b & 7u) << 38) | ((uint64_t)(n & 4095u) << 41);
}
__device__ __forceinline__ uint32_t state_p(uint64_t s) { return (uint32_t)s; }
__device__ __forceinline__ uint32_t state_k(uint64_t s) { return (uint32_t)(s >> 32) & 63u; }
__device__ __forceinline__ uint32_t state_b(uint64_t s) { return (uint32_t)(s >> 38) & 7u; }
__device__ __forceinline__ uint32_t state_n(uint64_t s) { return (uint32_t)(s >> 41) & 4095u; }
__device__ __forceinline__ uint64_t state_only(uint64_t s) { return s & (((uint64_t)1 << 41) - 1); }

struct DecodeArgs {
    const uint8_t* scans;
    const uint32_t* lengths;
    const uint8_t* tables;
    const uint64_t* state_in;
    uint64_t* state_out;
    const uint32_t* first;
    int16_t* coef;
    uint32_t* status;
    uint32_t capacity;
    int nsub, ny, bpm, nblocks;
};

struct NullSink {
    __device__ __forceinline__ void coefficient(uint32_t, uint32_t, int) {}
    __device__ __forceinline__ void invalid(uint32_t) {}
};

struct CoefSink {
    int16_t* coef;         // the image's [nblocks][64]
    uint32_t first, nblocks;
    bool bad;
    __device__ __forceinline__ void coefficient(uint32_t n, uint32_t k, int value) {
        const uint32_t ordinal = first + n;
        if (ordinal < nblocks) coef[(size_t)ordinal * 64 + kNatural[k & 63u]] = (int16_t)value;
    }
    __device__ __forceinline__ void invalid(uint32_t n) { bad = bad || first + n < nblocks; }
};

// The workgroup's window of the scan in LDS: kRows subsequences from byte `base` on, bytes from `len` on as 0xFF.
struct Window {
    const uint8_t* bytes;
    uint32_t base, span;       // span: bytes of the window below len
    __device__ __forceinline__ uint32_t at(uint32_t q) const {
        const uint32_t x = q - base;
        return x < span ? bytes[(x >> 7) * kRowStride + (x & 127u)] : 0xFFu;
    }
};

__device__ __forceinline__ void load_window(uint8_t* lds, const uint8_t* scan, uint32_t base, uint32_t len, uint32_t capacity) {
    for (int i = threadIdx.x; i < kSpanBytes / 16; i += kThreads) {
        const uint32_t x = (uint32_t)i * 16;
        const uint32_t q = base + x;
        uint32_t v[4] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
        if (q < len && q + 16 <= capacity) {      // (capacity is a multiple of 16, so a started 16 bytes lie inside it)
            const uint4 g = *(const uint4*)(scan + q);
            v[0] = g.x;
            v[1] = g.y;
            v[2] = g.z;
            v[3] = g.w;
        }
        uint32_t* d = (uint32_t*)(lds + (x >> 7) * kRowStride + (x & 127u));
#pragma unroll
        for (int j = 0; j < 4; ++j) d[j] = v[j];
    }
}

// Decode the symbols that start before byte `end` from state (p, b, k) -> the packed end state with the blocks completed.
template <class Sink>
__device__ __forceinline__ uint64_t run_subsequence(const Window& win, const uint8_t* tb, int ny, int bpm, uint64_t start,
                                                    uint32_t end, Sink& sink) {
    uint32_t B = state_p(start) >> 3, o = state_p(start) & 7u, b = state_b(start), k = state_k(start), n = 0;
    while (B < end) {
        uint64_t w = 0;      // five data bytes from B on, stuffed 00s left out
        uint32_t q = B;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint32_t v = win.at(q);
            w = (w << 8) | v;
            q += v == 0xFFu ? 2u : 1u;
        }
        const uint32_t bits = (uint32_t)(w >> (8u - o));      // the next 32 bits
        const uint8_t* t = tb + kQuantBytes + ((b < (uint32_t)ny ? 0 : 2) + (k ? 1 : 0)) * kHuffBytes;
        const uint32_t e = ((const uint16_t*)t)[bits >> 24];
        uint32_t length = e >> 8;
        int sym = (int)(e & 255u);
        if (e == 0) {
            sym = -1;
            length = 16;
            const int32_t* maxcode = (const int32_t*)(t + 512);
            const int32_t* valoff = (const int32_t*)(t + 576);
            for (uint32_t l = 9; l <= 16; ++l) {
                const int32_t code = (int32_t)(bits >> (32u - l));
                if (code <= maxcode[l - 1]) {
                    sym = t[640 + ((uint32_t)(code + valoff[l - 1]) & 255u)];
                    length = l;
                    break;
                }
            }
        }
        length = length < 1 ? 1 : (length > 16 ? 16 : length);      // whatever the blob holds, a symbol consumes 1..31 bits
        uint32_t used = 16;
        if (sym < 0) {      // no such code: 16 bits are dropped, the block state stays
            sink.invalid(n);
        } else {
            const uint32_t s = (uint32_t)sym & 15u;
            used = length + s;
            int value = 0;
            if (s) {
                value = (int)((bits << length) >> (32u - s));
                if (value < (1 << (s - 1))) value -= (1 << s) - 1;
            }
            bool done = false;
            if (k == 0) {      // DC difference
                sink.coefficient(n, 0, value);
                k = 1;
            } else {
                const uint32_t r = (uint32_t)sym >> 4;
                if (s) {
                    k += r;
                    if (k > 63) k = 63;
                    sink.coefficient(n, k, value);
                    ++k;
                    done = k > 63;
                } else if (r == 15) {      // ZRL
                    k += 16;
                    done = k > 63;
                } else {      // EOB
                    done = true;
                }
            }
            if (done) {
                k = 0;
                b = b + 1 == (uint32_t)bpm ? 0 : b + 1;
                ++n;
            }
        }
        o += used;
        const uint32_t whole = o >> 3;      // at most 4
#pragma unroll
        for (uint32_t j = 0; j < 4; ++j)
            if (j < whole) B += ((uint32_t)(w >> (32u - 8u * j)) & 255u) == 0xFFu ? 2u : 1u;
        o &= 7u;
    }
    return pack_state(B * 8u + o, b, k, n);
}

struct DecodeShared {
    uint32_t tables[kTableBytes / 4];
    uint32_t scan[(kRows * kRowStride + 3) / 4];
    uint64_t state[kRows];
};

// what every decoding kernel starts with: the image's tables and the workgroup's window in LDS -> (window, end of this
// thread's subsequence, index of the subsequence, clamped scan length)
__device__ __forceinline__ Window stage(DecodeShared& sh, const DecodeArgs& a, int img, uint32_t& len) {
    len = a.lengths[img];
    if (len > a.capacity) len = a.capacity;
    const uint32_t base = blockIdx.x * (uint32_t)(kThreads * kSubseqBytes);
    const uint32_t* tb = (const uint32_t*)(a.tables + (size_t)img * kTableBytes);
    for (int i = threadIdx.x; i < kTableBytes / 4; i += kThreads) sh.tables[i] = tb[i];
    load_window((uint8_t*)sh.scan, a.scans + (size_t)img * a.capacity, base, len, a.capacity);
    Window w;
    w.bytes = (const uint8_t*)sh.scan;
    w.base = base;
    w.span = len > base ? (len - base < (uint32_t)kSpanBytes ? len - base : (uint32_t)kSpanBytes) : 0u;
    return w;
}

// whether subsequence i is a link of the chain: the first one always, the others if the scan reaches them.  The capacity
// fixes the number of threads, the length the number of links: states behind the scan are neither decoded nor compared.
__device__ __forceinline__ bool has_data(uint32_t i, uint32_t len) { return i == 0 || i * (uint32_t)kSubseqBytes < len; }

__device__ __forceinline__ uint32_t subsequence_end(uint32_t i, uint32_t len) {
    const uint32_t e = (i + 1u) * (uint32_t)kSubseqBytes;
    return e < len ? e : len;
}

__global__ __launch_bounds__(kThreads) void jpegdec_blind_kernel(DecodeArgs a) {
    __shared__ DecodeShared sh;
    const int img = blockIdx.y;
    uint32_t len;
    const Window win = stage(sh, a, img, len);
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i == 0) a.status[img] = a.lengths[img] > a.capacity ? (uint32_t)T2V_JPEGDEC_CORRUPT : 0u;
    if (i >= (uint32_t)a.nsub) return;
    uint32_t B = i * (uint32_t)kSubseqBytes;
    if (!has_data(i, len)) {      // behind the scan: no link of the chain
        a.state_out[(size_t)img * a.nsub + i] = 0;
        return;
    }
    if (i > 0 && a.scans[(size_t)img * a.capacity + B - 1] == 0xFFu) ++B;      // starts on the 00 of an FF 00 pair
    NullSink sink;
    a.state_out[(size_t)img * a.nsub + i] =
        run_subsequence(win, (const uint8_t*)sh.tables, a.ny, a.bpm, pack_state(B * 8u, 0, 0, 0), subsequence_end(i, len), sink);
}

__global__ __launch_bounds__(kThreads) void jpegdec_sync_kernel(DecodeArgs a) {
    __shared__ DecodeShared sh;
    const int img = blockIdx.y;
    uint32_t len;
    const Window win = stage(sh, a, img, len);
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    const bool live = i < (uint32_t)a.nsub && has_data(i, len);
    const uint64_t* in = a.state_in + (size_t)img * a.nsub;
    // state[j]: the end state of the subsequence before thread j's; state[0] of the first workgroup is the true start
    if (threadIdx.x == 0) sh.state[0] = i == 0 ? 0 : in[i - 1];
    sh.state[threadIdx.x + 1] = i < (uint32_t)a.nsub ? in[i] : 0;
    __syncthreads();
    const uint32_t end = subsequence_end(i, len);
    for (int round = 0; round < kRounds; ++round) {
        const uint64_t from = state_only(sh.state[threadIdx.x]);
        uint64_t now = sh.state[threadIdx.x + 1];
        int changed = 0;
        if (live) {
            NullSink sink;
            const uint64_t got = run_subsequence(win, (const uint8_t*)sh.tables, a.ny, a.bpm, from, end, sink);
            changed = got != now;
            now = got;
        }
        __syncthreads();      // every thread has read its predecessor's state
        sh.state[threadIdx.x + 1] = now;
        if (!__syncthreads_or(changed)) break;
    }
    if (i < (uint32_t)a.nsub) a.state_out[(size_t)img * a.nsub + i] = sh.state[threadIdx.x + 1];
}

__global__ __launch_bounds__(kThreads) void jpegdec_write_kernel(DecodeArgs a) {
    __shared__ DecodeShared sh;
    const int img = blockIdx.y;
    uint32_t len;
    const Window win = stage(sh, a, img, len);
    __syncthreads();
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= (uint32_t)a.nsub || !has_data(i, len)) return;
    const uint64_t* in = a.state_in + (size_t)img * a.nsub;
    CoefSink sink;
    sink.coef = a.coef + (size_t)img * a.nblocks * 64;
    sink.first = a.first[(size_t)img * a.nsub + i];
    sink.nblocks = (uint32_t)a.nblocks;
    sink.bad = false;
    const uint64_t from = i == 0 ? 0 : state_only(in[i - 1]);
    const uint64_t got = run_subsequence(win, (const uint8_t*)sh.tables, a.ny, a.bpm, from, subsequence_end(i, len), sink);
    uint32_t flags = 0;
    if (got != in[i]) flags |= (uint32_t)T2V_JPEGDEC_NOT_CONVERGED;
    if (sink.bad) flags |= (uint32_t)T2V_JPEGDEC_CORRUPT;
    if (flags) atomicOr(a.status + img, flags);
}

// exclusive prefix sum over 256 per-thread totals (in place in `part`), returns the grand total
__device__ __forceinline__ int block_exclusive_scan(int* part, int mine) {
    part[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < kThreads; d <<= 1) {
        const int v = threadIdx.x >= (unsigned)d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const int total = part[kThreads - 1];
    const int before = part[threadIdx.x] - mine;
    __syncthreads();
    part[threadIdx.x] = before;      // (read back by its own thread only)
    return total;
}

__global__ __launch_bounds__(kThreads) void jpegdec_scan_kernel(const uint64_t* state, uint32_t* first, uint32_t* status,
                                                                const uint32_t* lengths, uint32_t capacity, int nsub, int nblocks) {
    __shared__ int part[kThreads];
    const int img = blockIdx.x;
    const uint64_t* st = state + (size_t)img * nsub;
    uint32_t* out = first + (size_t)img * nsub;
    const int per = (nsub + kThreads - 1) / kThreads;
    const int lo = threadIdx.x * per, hi = lo + per < nsub ? lo + per : nsub;
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += (int)state_n(st[i]);
    const int total = block_exclusive_scan(part, sum);
    int run = part[threadIdx.x];
    for (int i = lo; i < hi; ++i) {
        out[i] = (uint32_t)run;
        run += (int)state_n(st[i]);
    }
    if (threadIdx.x == 0) {
        uint32_t len = lengths[img];
        if (len > capacity) len = capacity;
        const uint32_t links = len ? (len + kSubseqBytes - 1) / kSubseqBytes : 1u;      // (<= nsub: len <= capacity)
        const uint64_t last = st[links - 1];
        if (total != nblocks || state_b(last) != 0 || state_k(last) != 0) atomicOr(status + img, (uint32_t)T2V_JPEGDEC_CORRUPT);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// reconstruction
// ---------------------------------------------------------------------------------------------------------------------
struct ImageArgs {
    int16_t* coef;
    const uint8_t* tables;
    uint8_t* planes;
    uint8_t* dst;
    size_t plane_bytes;
    int H, W, dst_cs;
    int hs, vs, ny, bpm, mw, nmcu, nblocks;
    int yw, yh, cwp, chp, cw, ch;
};

__global__ __launch_bounds__(kThreads) void jpegdec_dc_kernel(ImageArgs p) {
    __shared__ int part[kThreads];
    const int c = blockIdx.x, img = blockIdx.y;
    int16_t* coef = p.coef + (size_t)img * p.nblocks * 64;
    const int count = c == 0 ? p.nmcu * p.ny : p.nmcu;
    auto ordinal = [&](int e) { return c == 0 ? (e / p.ny) * p.bpm + e % p.ny : e * p.bpm + p.ny + c - 1; };
    const int per = (count + kThreads - 1) / kThreads;
    const int lo = threadIdx.x * per, hi = lo + per < count ? lo + per : count;
    int sum = 0;
    for (int e = lo; e < hi; ++e) sum += coef[(size_t)ordinal(e) * 64];
    block_exclusive_scan(part, sum);
    int run = part[threadIdx.x];
    for (int e = lo; e < hi; ++e) {
        int16_t* dc = coef + (size_t)ordinal(e) * 64;
        run += *dc;
        *dc = (int16_t)run;
    }
}

// one 1-D pass of jpeg_idct_islow over x[0..7], descaled by `shift`
__device__ __forceinline__ void idct_pass(int (&x)[8], int shift) {
    int z2 = x[2], z3 = x[6];
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 - z3 * 15137;
    int tmp3 = z1 + z2 * 6270;
    int tmp0 = (int)((uint32_t)(x[0] + x[4]) << 13);
    int tmp1 = (int)((uint32_t)(x[0] - x[4]) << 13);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = x[7];
    tmp1 = x[5];
    tmp2 = x[3];
    tmp3 = x[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446;
    tmp1 *= 16819;
    tmp2 *= 25172;
    tmp3 *= 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    const int half = 1 << (shift - 1);
    x[0] = (tmp10 + tmp3 + half) >> shift;
    x[7] = (tmp10 - tmp3 + half) >> shift;
    x[1] = (tmp11 + tmp2 + half) >> shift;
    x[6] = (tmp11 - tmp2 + half) >> shift;
    x[2] = (tmp12 + tmp1 + half) >> shift;
    x[5] = (tmp12 - tmp1 + half) >> shift;
    x[3] = (tmp13 + tmp0 + half) >> shift;
    x[4] = (tmp13 - tmp0 + half) >> shift;
}

__global__ __launch_bounds__(kThreads) void jpegdec_idct_kernel(ImageArgs p) {
    __shared__ int ws[32][8][9];
    const int img = blockIdx.y;
    const int local = threadIdx.x >> 3, lane = threadIdx.x & 7;
    const int ordinal = blockIdx.x * 32 + local;
    const bool live = ordinal < p.nblocks;
    const int mcu = ordinal / p.bpm, bi = ordinal % p.bpm;
    const int c = bi < p.ny ? 0 : bi - p.ny + 1;
    int x[8];
    if (live) {      // column `lane`
        const int16_t* coef = p.coef + ((size_t)img * p.nblocks + ordinal) * 64;
        const uint16_t* q = (const uint16_t*)(p.tables + (size_t)img * kTableBytes) + c * 64;
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (int)coef[r * 8 + lane] * (int)q[r * 8 + lane];
        idct_pass(x, 11);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[local][r][lane] = x[r];
    }
    __syncthreads();
    if (!live) return;
#pragma unroll
    for (int col = 0; col < 8; ++col) x[col] = ws[local][lane][col];      // row `lane`
    idct_pass(x, 18);
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int col = 0; col < 4; ++col) {
        int a = x[col] + 128, b = x[col + 4] + 128;
        a = a < 0 ? 0 : (a > 255 ? 255 : a);
        b = b < 0 ? 0 : (b > 255 ? 255 : b);
        lo |= (uint32_t)a << (8 * col);
        hi |= (uint32_t)b << (8 * col);
    }
    const int mx = mcu % p.mw, my = mcu / p.mw;
    uint8_t* plane = p.planes + (size_t)img * p.plane_bytes;
    int stride, bx, by;
    if (c == 0) {
        stride = p.yw;
        bx = mx * p.hs + (bi % p.hs);
        by = my * p.vs + (bi / p.hs);
    } else {
        plane += (size_t)p.yw * p.yh + (size_t)(c - 1) * p.cwp * p.chp;
        stride = p.cwp;
        bx = mx;
        by = my;
    }
    *(uint2*)(plane + (size_t)(by * 8 + lane) * stride + bx * 8) = make_uint2(lo, hi);      // (8-byte aligned: strides are 8 n)
}

// one up-sampled chroma sample at pixel (x, y): libjpeg's fancy filters with neighbours clamped to the real cw x ch extent
__device__ __forceinline__ int chroma_at(const uint8_t* pl, int stride, int x, int y, int hs, int vs, int cw, int ch) {
    if (hs == 1) return pl[(size_t)y * stride + x];
    const int cx = x >> 1;
    const int nx = (x & 1) ? (cx + 1 < cw ? cx + 1 : cw - 1) : (cx > 0 ? cx - 1 : 0);
    if (vs == 1) {
        const uint8_t* row = pl + (size_t)y * stride;
        return (3 * row[cx] + row[nx] + ((x & 1) ? 2 : 1)) >> 2;
    }
    const int cy = y >> 1;
    const int fy = (y & 1) ? (cy + 1 < ch ? cy + 1 : ch - 1) : (cy > 0 ? cy - 1 : 0);
    const uint8_t* near = pl + (size_t)cy * stride;
    const uint8_t* far = pl + (size_t)fy * stride;
    const int here = 3 * near[cx] + far[cx], there = 3 * near[nx] + far[nx];
    return (3 * here + there + ((x & 1) ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(kThreads) void jpegdec_colour_kernel(ImageArgs p) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6), img = blockIdx.z;
    if (x >= p.W || y >= p.H) return;
    const uint8_t* plane = p.planes + (size_t)img * p.plane_bytes;
    const uint8_t* cbp = plane + (size_t)p.yw * p.yh;
    const uint8_t* crp = cbp + (size_t)p.cwp * p.chp;
    const int Y = plane[(size_t)y * p.yw + x];
    const int cb = chroma_at(cbp, p.cwp, x, y, p.hs, p.vs, p.cw, p.ch) - 128;
    const int cr = chroma_at(crp, p.cwp, x, y, p.hs, p.vs, p.cw, p.ch) - 128;
    // jdcolor.c: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 32768
    int r = Y + ((91881 * cr + 32768) >> 16);
    int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
    int b = Y + ((116130 * cb + 32768) >> 16);
    r = r < 0 ? 0 : (r > 255 ? 255 : r);
    g = g < 0 ? 0 : (g > 255 ? 255 : g);
    b = b < 0 ? 0 : (b > 255 ? 255 : b);
    uint8_t* d = p.dst + (((size_t)img * p.H + y) * p.W + x) * p.dst_cs;
    d[0] = (uint8_t)r;
    d[1] = (uint8_t)g;
    d[2] = (uint8_t)b;
    if (p.dst_cs == 4) d[3] = 0;
}

}  // namespace

extern "C" {

int t2v_jpegdec_abi_version(void) { return T2V_JPEGDEC_ABI_VERSION; }

const char* t2v_jpegdec_last_error(void) { return g_error; }

int t2v_jpegdec_supported(int H, int W, int sampling) { return supported(H, W, sampling) ? 1 : 0; }

size_t t2v_jpegdec_table_bytes(void) { return kTableBytes; }

size_t t2v_jpegdec_workspace_bytes(int H, int W, int sampling, int nimg, size_t scan_capacity) {
    if (!supported(H, W, sampling) || nimg < 1 || nimg > T2V_JPEGDEC_MAX_IMAGES || !capacity_ok(scan_capacity)) return 0;
    return carve(geometry(H, W, sampling, scan_capacity), nimg, nullptr).bytes;
}

int t2v_jpegdec_decode_u8(void* stream, const uint8_t* scans, size_t scan_capacity, const uint32_t* scan_lengths,
                          const uint8_t* tables, int H, int W, int sampling, int nimg, void* workspace, uint8_t* dst, int dst_cs,
                          uint32_t* status) {
    JPEGDEC_REQUIRE(H >= T2V_JPEGDEC_MIN_DIM && H <= T2V_JPEGDEC_MAX_DIM && W >= T2V_JPEGDEC_MIN_DIM && W <= T2V_JPEGDEC_MAX_DIM,
                    "t2v_jpegdec_decode_u8: %dx%d is outside %d..%d per dimension", H, W, T2V_JPEGDEC_MIN_DIM, T2V_JPEGDEC_MAX_DIM);
    JPEGDEC_REQUIRE(sampling >= 0 && sampling <= 2, "t2v_jpegdec_decode_u8: sampling %d (0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0)", sampling);
    JPEGDEC_REQUIRE(dst_cs == 3 || dst_cs == 4, "t2v_jpegdec_decode_u8: dst_cs %d (3 or 4)", dst_cs);
    JPEGDEC_REQUIRE(nimg >= 1 && nimg <= T2V_JPEGDEC_MAX_IMAGES, "t2v_jpegdec_decode_u8: %d images (1..%d)", nimg,
                    T2V_JPEGDEC_MAX_IMAGES);
    JPEGDEC_REQUIRE(capacity_ok(scan_capacity), "t2v_jpegdec_decode_u8: scan_capacity %zu (a multiple of 16, 16..%zu)", scan_capacity,
                    kMaxScanCapacity);
    JPEGDEC_REQUIRE(scans && scan_lengths && tables && workspace && dst && status, "t2v_jpegdec_decode_u8: null pointer");
    JPEGDEC_REQUIRE(((uintptr_t)workspace & 255u) == 0, "t2v_jpegdec_decode_u8: the workspace must be 256-byte aligned");
    JPEGDEC_REQUIRE(((uintptr_t)scans & 15u) == 0 && ((uintptr_t)tables & 3u) == 0 && ((uintptr_t)scan_lengths & 3u) == 0 &&
                        ((uintptr_t)status & 3u) == 0,
                    "t2v_jpegdec_decode_u8: scans must be 16-byte aligned, tables, scan_lengths and status 4-byte aligned");
    const hipStream_t s = (hipStream_t)stream;
    const Geom g = geometry(H, W, sampling, scan_capacity);
    const Workspace w = carve(g, nimg, workspace);

    JPEGDEC_HIP_CHECK(hipMemsetAsync(w.coef, 0, w.coef_bytes, s));

    DecodeArgs a;
    a.scans = scans;
    a.lengths = scan_lengths;
    a.tables = tables;
    a.state_in = nullptr;
    a.state_out = w.state_a;
    a.first = w.first;
    a.coef = w.coef;
    a.status = status;
    a.capacity = (uint32_t)scan_capacity;
    a.nsub = g.nsub;
    a.ny = g.ny;
    a.bpm = g.bpm;
    a.nblocks = g.nblocks;
    const dim3 grid(g.nwg, nimg);
    hipLaunchKernelGGL(jpegdec_blind_kernel, grid, dim3(kThreads), 0, s, a);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    a.state_in = w.state_a;
    a.state_out = w.state_b;
    hipLaunchKernelGGL(jpegdec_sync_kernel, grid, dim3(kThreads), 0, s, a);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    a.state_in = w.state_b;
    a.state_out = w.state_a;
    hipLaunchKernelGGL(jpegdec_sync_kernel, grid, dim3(kThreads), 0, s, a);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_scan_kernel, dim3(nimg), dim3(kThreads), 0, s, (const uint64_t*)w.state_a, w.first, status,
                       scan_lengths, (uint32_t)scan_capacity, g.nsub, g.nblocks);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    a.state_in = w.state_a;
    a.state_out = nullptr;
    hipLaunchKernelGGL(jpegdec_write_kernel, grid, dim3(kThreads), 0, s, a);
    JPEGDEC_HIP_CHECK(hipGetLastError());

    ImageArgs p;
    p.coef = w.coef;
    p.tables = tables;
    p.planes = w.planes;
    p.dst = dst;
    p.plane_bytes = g.plane_bytes;
    p.H = H;
    p.W = W;
    p.dst_cs = dst_cs;
    p.hs = g.hs;
    p.vs = g.vs;
    p.ny = g.ny;
    p.bpm = g.bpm;
    p.mw = g.mw;
    p.nmcu = g.nmcu;
    p.nblocks = g.nblocks;
    p.yw = g.yw;
    p.yh = g.yh;
    p.cwp = g.cwp;
    p.chp = g.chp;
    p.cw = g.cw;
    p.ch = g.ch;
    hipLaunchKernelGGL(jpegdec_dc_kernel, dim3(3, nimg), dim3(kThreads), 0, s, p);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_idct_kernel, dim3((g.nblocks + 31) / 32, nimg), dim3(kThreads), 0, s, p);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpegdec_colour_kernel, dim3((W + 63) / 64, (H + 3) / 4, nimg), dim3(kThreads), 0, s, p);
    JPEGDEC_HIP_CHECK(hipGetLastError());
    return T2V_JPEGDEC_OK;
}

}  // extern "C"
