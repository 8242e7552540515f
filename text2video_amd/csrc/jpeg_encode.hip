// libt2v_jpeg.so (include/t2v_jpeg.h): baseline JPEG encoding of uint8 RGB images on the GPU, byte for byte the scan
// libjpeg / Pillow writes (4:2:0, Annex K tables, integer "islow" DCT).  DESIGN.md section 4.10 has the format rules.
//
// One call = one memset and seven launches, the same for every content:
//   1. jpeg_mcu_kernel          one wave per 16x16 MCU.  Every lane converts one 2x2 quad (edge-replicated) to Y / Cb / Cr,
//                               down-samples its chroma quad and stages the six 8x8 blocks in LDS minus 128; 48 lanes run the
//                               row passes, then the column passes of the forward DCT in place; every lane then quantises
//                               one zigzag position of the six blocks and writes int16 coefficients [img][mcu][6][64].
//                               Dummy Y blocks (beyond the image's own block grid) get the DC of their predecessor, no AC.
//   2. jpeg_block_bits_kernel   one thread per block: DC difference against the component's previous block in coding order,
//                               then the block's Huffman bit count.
//   3. jpeg_scan_kernel         one workgroup per image: exclusive prefix sum of the bit counts (+ the total).
//   4. jpeg_block_pack_kernel   one thread per block: the same walk as 2, now writing the code words MSB-first at the block's
//                               bit offset into the zeroed dword stream.  Dwords that lie wholly inside the block are plain
//                               stores; the first and the last may be shared with a neighbour and are OR-ed in (atomicOr: the
//                               result does not depend on the order).
//   5. jpeg_ff_count_kernel     one workgroup per 4096 bytes of the packed stream: its number of 0xFF bytes (the final byte
//                               seen with its 1-bit padding).
//   6. jpeg_scan_kernel         again, over those counts.
//   7. jpeg_stuff_kernel        the same 4096-byte chunks: every thread writes its 16 bytes, each 0xFF followed by 0x00, at
//                               chunk base + 0xFF bytes before it, never past out_capacity; lengths[img] = bytes + 0xFF count.
// Integer arithmetic only, no float, no inline assembly; every store is a vector store.  2 and 4 share one block walk
// (code_block) with two sinks, so a bit counted is a bit written.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/t2v_jpeg.h"

namespace {

thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define JPEG_HIP_CHECK(expr)                                                                          \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));           \
            return T2V_JPEG_ERR_HIP;                                                                  \
        }                                                                                             \
    } while (0)
#define JPEG_REQUIRE(cond, ...)           \
    do {                                  \
        if (!(cond)) {                    \
            set_error(__VA_ARGS__);       \
            return T2V_JPEG_ERR_INVALID;  \
        }                                 \
    } while (0)

constexpr int kBlockBytes = 208;       // ceil(1660 bits / 8): include/t2v_jpeg.h, t2v_jpeg_scan_capacity
constexpr int kChunkBytes = 4096;      // of the packed stream per workgroup of the stuffing kernels (256 threads x 16)

// ---------------------------------------------------------------------------------------------------------------------
// tables (ITU-T T.81 Annex K), built at compile time
// ---------------------------------------------------------------------------------------------------------------------
struct Huff {
    uint16_t code[256];
    uint8_t len[256];      // 0: no such symbol
};

constexpr int hex_digit(char c) { return c <= '9' ? c - '0' : c - 'a' + 10; }

// BITS[16] and HUFFVAL as a hex string -> code and length per symbol (T.81 Annex C)
constexpr Huff make_huff(const int (&bits)[16], const char* vals_hex) {
    Huff h{};
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) {
            const int sym = hex_digit(vals_hex[2 * k]) * 16 + hex_digit(vals_hex[2 * k + 1]);
            h.code[sym] = (uint16_t)code++;
            h.len[sym] = (uint8_t)len;
        }
        code <<= 1;
    }
    return h;
}

constexpr int kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr int kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr int kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125};
constexpr int kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119};
constexpr char kDcVals[] = "000102030405060708090a0b";
constexpr char kAcLumaVals[] =
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa";
constexpr char kAcChromaVals[] =
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a3536373839"
    "3a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7"
    "a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa";

// [0] DC luma, [1] AC luma, [2] DC chroma, [3] AC chroma
__constant__ Huff kHuff[4] = {make_huff(kDcLumaBits, kDcVals), make_huff(kAcLumaBits, kAcLumaVals),
                              make_huff(kDcChromaBits, kDcVals), make_huff(kAcChromaBits, kAcChromaVals)};

// natural index of the k-th coefficient in coding order
__constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Annex K.1 / K.2 quantisation tables, natural order
__constant__ uint8_t kBaseQuant[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// ---------------------------------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------------------------------
struct Geom {
    int H, W, mw, mh, bw, bh;      // MCUs per row / column; real Y blocks per row / column
    int nmcu, nblocks;             // per image; nblocks = 6 nmcu
    int nchunks;                   // kChunkBytes chunks of the packed stream per image
};

Geom geometry(int H, int W) {
    Geom g;
    g.H = H;
    g.W = W;
    g.mw = (W + 15) / 16;
    g.mh = (H + 15) / 16;
    g.bw = (W + 7) / 8;
    g.bh = (H + 7) / 8;
    g.nmcu = g.mw * g.mh;
    g.nblocks = 6 * g.nmcu;
    g.nchunks = (g.nblocks * kBlockBytes + kChunkBytes - 1) / kChunkBytes;
    return g;
}

struct Workspace {
    int16_t* coef;         // [nimg][nblocks][64]
    uint32_t* bits;        // [nimg][nblocks]
    uint32_t* bit_off;     // [nimg][nblocks]
    uint8_t* packed;       // [nimg][nchunks * kChunkBytes], as big-endian dwords while it is packed
    uint32_t* ff_count;    // [nimg][nchunks]
    uint32_t* ff_off;      // [nimg][nchunks]
    uint32_t* bit_total;   // [nimg]
    uint32_t* ff_total;    // [nimg]
    size_t bytes;
};

inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }

Workspace carve(const Geom& g, int nimg, void* base) {
    Workspace w;
    uint8_t* p = (uint8_t*)base;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t* q = p + off;
        off += round256(bytes);
        return q;
    };
    const size_t n = (size_t)nimg;
    w.coef = (int16_t*)take(n * g.nblocks * 64 * sizeof(int16_t));
    w.bits = (uint32_t*)take(n * g.nblocks * sizeof(uint32_t));
    w.bit_off = (uint32_t*)take(n * g.nblocks * sizeof(uint32_t));
    w.packed = take(n * g.nchunks * kChunkBytes);
    w.ff_count = (uint32_t*)take(n * g.nchunks * sizeof(uint32_t));
    w.ff_off = (uint32_t*)take(n * g.nchunks * sizeof(uint32_t));
    w.bit_total = (uint32_t*)take(n * sizeof(uint32_t));
    w.ff_total = (uint32_t*)take(n * sizeof(uint32_t));
    w.bytes = off;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. colour, down-sampling, forward DCT, quantisation
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// libjpeg jfdctint.c, one 1-D pass over d0..d7 in place.  kFirst: the row pass (DC path << 2, the rest descaled by 11);
// else the column pass (DC path descaled by 2, the rest by 15).
template <bool kFirst>
__device__ __forceinline__ void fdct_pass(int& d0, int& d1, int& d2, int& d3, int& d4, int& d5, int& d6, int& d7) {
    constexpr int n = kFirst ? 11 : 15;
    const int t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (kFirst) {
        d0 = (t10 + t11) * 4;
        d4 = (t10 - t11) * 4;
    } else {
        d0 = descale(t10 + t11, 2);
        d4 = descale(t10 - t11, 2);
    }
    int z1 = (t12 + t13) * 4433;
    d2 = descale(z1 + t13 * 6270, n);
    d6 = descale(z1 - t12 * 15137, n);
    z1 = t4 + t7;
    int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int u4 = t4 * 2446, u5 = t5 * 16819, u6 = t6 * 25172, u7 = t7 * 12299;
    z1 *= -7373;
    z2 *= -20995;
    z3 = z3 * -16069 + z5;
    z4 = z4 * -3196 + z5;
    d7 = descale(u4 + z1 + z3, n);
    d5 = descale(u5 + z2 + z4, n);
    d3 = descale(u6 + z2 + z3, n);
    d1 = descale(u7 + z1 + z4, n);
}

struct McuArgs {
    const uint8_t* src;
    int16_t* coef;
    int H, W, cs, mw, bw, bh, nmcu;
    int scale;      // the IJG quality scaling: 5000 / Q below 50, 200 - 2 Q from 50 on
};

constexpr int kPitch = 9;      // ints per staged row: the column pass reads down a column

__global__ __launch_bounds__(64) void jpeg_mcu_kernel(McuArgs p) {
    __shared__ int s[6][8][kPitch];      // Y00, Y01, Y10, Y11, Cb, Cr
    const int lane = threadIdx.x, mcu = blockIdx.x, img = blockIdx.y;
    const int mx = mcu % p.mw, my = mcu / p.mw;
    const uint8_t* im = p.src + (size_t)img * p.H * p.W * p.cs;
    const int qx = lane & 7, qy = lane >> 3;      // this lane's 2x2 quad of the MCU

    // luma: the plane is edge-replicated in both directions
    for (int dy = 0; dy < 2; ++dy)
        for (int dx = 0; dx < 2; ++dx) {
            const int ly = 2 * qy + dy, lx = 2 * qx + dx;
            const int y = min(16 * my + ly, p.H - 1), x = min(16 * mx + lx, p.W - 1);
            const uint8_t* px = im + ((size_t)y * p.W + x) * p.cs;
            const int r = px[0], g = px[1], b = px[2];
            s[(ly >> 3) * 2 + (lx >> 3)][ly & 7][lx & 7] = ((19595 * r + 38470 * g + 7471 * b + 32768) >> 16) - 128;
        }
    // chroma: the full-resolution plane's last column is replicated all the way, its last row only to an even height;
    // below that the last DOWN-SAMPLED row repeats
    {
        const int rc = min(8 * my + qy, (p.H + 1) / 2 - 1);
        int cb = 0, cr = 0;
        for (int dy = 0; dy < 2; ++dy)
            for (int dx = 0; dx < 2; ++dx) {
                const int y = min(2 * rc + dy, p.H - 1), x = min(2 * (8 * mx + qx) + dx, p.W - 1);
                const uint8_t* px = im + ((size_t)y * p.W + x) * p.cs;
                const int r = px[0], g = px[1], b = px[2];
                cb += (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
                cr += (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
            }
        const int bias = 1 + (qx & 1);      // 1 on even output columns, 2 on odd ones (8 mx is even)
        s[4][qy][qx] = ((cb + bias) >> 2) - 128;
        s[5][qy][qx] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    if (lane < 48) {
        int* row = s[lane >> 3][lane & 7];
        fdct_pass<true>(row[0], row[1], row[2], row[3], row[4], row[5], row[6], row[7]);
    }
    __syncthreads();
    if (lane < 48) {
        int(*blk)[kPitch] = s[lane >> 3];
        const int c = lane & 7;
        fdct_pass<false>(blk[0][c], blk[1][c], blk[2][c], blk[3][c], blk[4][c], blk[5][c], blk[6][c], blk[7][c]);
    }
    __syncthreads();

    // lane k: coefficient k (coding order) of the six blocks
    const int nat = kZigzag[lane];
    int16_t* dst = p.coef + ((size_t)img * p.nmcu + mcu) * 6 * 64;
    int prev = 0;      // (lane 0) the quantised DC of the block before
    for (int b = 0; b < 6; ++b) {
        const int comp = b < 4 ? 0 : 1;
        const int q = min(max(((int)kBaseQuant[comp][nat] * p.scale + 50) / 100, 1), 255);
        const int d = s[b][nat >> 3][nat & 7];
        const int a = d < 0 ? -d : d;
        int v = (a + 4 * q) / (8 * q);
        v = d < 0 ? -v : v;
        const bool real = b >= 4 || (2 * mx + (b & 1) < p.bw && 2 * my + (b >> 1) < p.bh);
        if (!real) v = lane == 0 ? prev : 0;      // block 0 of an MCU is always real
        prev = v;
        dst[b * 64 + lane] = (int16_t)v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// 2 / 4. entropy coding of one block, into a sink that counts or writes
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int bit_length(int a) { return 32 - __clz(a); }      // of a >= 0; 0 for 0

template <class Sink>
__device__ __forceinline__ void code_value(Sink& sink, const Huff& t, int run, int v, int max_size) {
    const int a = v < 0 ? -v : v;
    const int size = min(bit_length(a), max_size);
    const int sym = (run << 4) | size;
    sink.put(t.code[sym], t.len[sym]);
    if (size) sink.put((unsigned)(v < 0 ? v + (1 << size) - 1 : v) & ((1u << size) - 1u), size);
}

// c: the block's 64 coefficients in coding order (16-byte aligned); pred: the DC of the component's previous block
template <class Sink>
__device__ __forceinline__ void code_block(const int16_t* c, int pred, int chroma, Sink& sink) {
    const Huff& dc = kHuff[2 * chroma];
    const Huff& ac = kHuff[2 * chroma + 1];
    int run = 0;
    auto step = [&](int v) {
        if (v == 0) {
            ++run;
            return;
        }
        for (; run > 15; run -= 16) sink.put(ac.code[0xF0], ac.len[0xF0]);      // ZRL
        code_value(sink, ac, run, v, 10);
        run = 0;
    };
    for (int g = 0; g < 8; ++g) {
        const uint4 w = reinterpret_cast<const uint4*>(c)[g];
        if (g == 0)
            code_value(sink, dc, 0, (int)(int16_t)(w.x & 0xffffu) - pred, 11);
        else
            step((int)(int16_t)(w.x & 0xffffu));
        step((int)(int16_t)(w.x >> 16));
        step((int)(int16_t)(w.y & 0xffffu));
        step((int)(int16_t)(w.y >> 16));
        step((int)(int16_t)(w.z & 0xffffu));
        step((int)(int16_t)(w.z >> 16));
        step((int)(int16_t)(w.w & 0xffffu));
        step((int)(int16_t)(w.w >> 16));
    }
    if (run) sink.put(ac.code[0x00], ac.len[0x00]);      // EOB
}

// the DC this block's difference is taken against: Y blocks follow each other through the MCUs, Cb and Cr step by MCU
__device__ __forceinline__ int dc_predecessor(const int16_t* img_coef, int b) {
    const int k = b % 6, mcu = b / 6;
    if (k >= 1 && k <= 3) return img_coef[(size_t)(b - 1) * 64];
    if (mcu == 0) return 0;
    return img_coef[(size_t)((mcu - 1) * 6 + (k == 0 ? 3 : k)) * 64];
}

struct CountSink {
    unsigned n = 0;
    __device__ __forceinline__ void put(unsigned, int len) { n += (unsigned)len; }
};

// MSB-first into big-endian dwords, starting at any bit offset
struct PackSink {
    uint32_t* words;       // the image's stream
    uint32_t w, limit;     // next dword, dwords in the stream
    uint64_t acc;          // the low n bits are pending (the first dword's leading bits, a neighbour's, count as zeros)
    int n;
    bool first;
    __device__ __forceinline__ void put(unsigned code, int len) {
        acc = (acc << len) | code;
        n += len;
        if (n >= 32) {
            n -= 32;
            const uint32_t v = __builtin_bswap32((uint32_t)(acc >> n));
            if (w < limit) {
                if (first)
                    atomicOr(&words[w], v);
                else
                    words[w] = v;
            }
            first = false;
            ++w;
            acc &= (1ull << n) - 1ull;
        }
    }
    __device__ __forceinline__ void finish() {
        if (n > 0 && w < limit) atomicOr(&words[w], __builtin_bswap32((uint32_t)(acc << (32 - n))));
    }
};

struct BlockArgs {
    const int16_t* coef;
    uint32_t* bits;              // 2: out
    const uint32_t* bit_off;     // 4: in
    uint8_t* packed;             // 4: out
    int nblocks;
    uint32_t packed_dwords;      // per image
};

__global__ __launch_bounds__(256) void jpeg_block_bits_kernel(BlockArgs p) {
    const int b = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (b >= p.nblocks) return;
    const int16_t* img_coef = p.coef + (size_t)img * p.nblocks * 64;
    CountSink sink;
    code_block(img_coef + (size_t)b * 64, dc_predecessor(img_coef, b), (b % 6) >= 4, sink);
    p.bits[(size_t)img * p.nblocks + b] = sink.n;
}

__global__ __launch_bounds__(256) void jpeg_block_pack_kernel(BlockArgs p) {
    const int b = blockIdx.x * 256 + threadIdx.x, img = blockIdx.y;
    if (b >= p.nblocks) return;
    const int16_t* img_coef = p.coef + (size_t)img * p.nblocks * 64;
    const uint32_t off = p.bit_off[(size_t)img * p.nblocks + b];
    PackSink sink;
    sink.words = reinterpret_cast<uint32_t*>(p.packed) + (size_t)img * p.packed_dwords;
    sink.w = off >> 5;
    sink.limit = p.packed_dwords;
    sink.acc = 0;
    sink.n = (int)(off & 31u);
    sink.first = true;
    code_block(img_coef + (size_t)b * 64, dc_predecessor(img_coef, b), (b % 6) >= 4, sink);
    sink.finish();
}

// ---------------------------------------------------------------------------------------------------------------------
// 3 / 6. exclusive prefix sum of n values per image, one workgroup per image, in a fixed order
// ---------------------------------------------------------------------------------------------------------------------
// inclusive scan of one value per thread over the 256 threads of a block
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t add = tid >= d ? red[tid - d] : 0u;
        __syncthreads();
        red[tid] += add;
        __syncthreads();
    }
    return red[tid];
}

__global__ __launch_bounds__(256) void jpeg_scan_kernel(const uint32_t* in, uint32_t* out, uint32_t* total, int n) {
    __shared__ uint32_t red[256];
    const int tid = threadIdx.x, img = blockIdx.x;
    in += (size_t)img * n;
    out += (size_t)img * n;
    const int per = (n + 255) / 256;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    uint32_t sum = 0;
    for (int i = lo; i < hi; ++i) sum += in[i];
    const uint32_t incl = block_inclusive_scan(sum, red);
    uint32_t run = incl - sum;
    for (int i = lo; i < hi; ++i) {
        const uint32_t v = in[i];
        out[i] = run;
        run += v;
    }
    if (tid == 255) total[img] = incl;
}

// ---------------------------------------------------------------------------------------------------------------------
// 5 / 7. byte stuffing
// ---------------------------------------------------------------------------------------------------------------------
struct StuffArgs {
    const uint8_t* packed;
    const uint32_t* bit_total;
    uint32_t* ff_count;            // 5: out
    const uint32_t* ff_off;        // 7: in
    const uint32_t* ff_total;      // 7: in
    uint8_t* out;                  // 7
    uint32_t* lengths;             // 7
    size_t out_capacity;
    int nchunks;
};

// this thread's 16 bytes of the packed stream (the last byte of the stream with its 1-bit padding) and how many of them
// belong to the stream
__device__ __forceinline__ int load_packed16(const StuffArgs& p, int img, uint32_t bits, uint32_t (&w)[4]) {
    const uint32_t nbytes = (bits + 7u) >> 3;
    const uint32_t i0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    if (i0 >= nbytes) return 0;
    const uint4 v = *reinterpret_cast<const uint4*>(p.packed + (size_t)img * p.nchunks * kChunkBytes + i0);
    w[0] = v.x;
    w[1] = v.y;
    w[2] = v.z;
    w[3] = v.w;
    const int valid = (int)min(16u, nbytes - i0);
    if ((bits & 7u) && nbytes - i0 <= 16u) {
        const uint32_t j = nbytes - 1u - i0, pad = (1u << (8u - (bits & 7u))) - 1u;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((int)(j >> 2) == k) w[k] |= pad << (8u * (j & 3u));
    }
    return valid;
}

__global__ __launch_bounds__(256) void jpeg_ff_count_kernel(StuffArgs p) {
    __shared__ uint32_t red[256];
    const int img = blockIdx.y;
    uint32_t w[4] = {0, 0, 0, 0};
    const int valid = load_packed16(p, img, p.bit_total[img], w);
    uint32_t count = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) count += (j < valid && ((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0xffu) ? 1u : 0u;
    const uint32_t incl = block_inclusive_scan(count, red);
    if (threadIdx.x == 255) p.ff_count[(size_t)img * p.nchunks + blockIdx.x] = incl;
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(StuffArgs p) {
    __shared__ uint32_t red[256];
    const int img = blockIdx.y;
    const uint32_t bits = p.bit_total[img];
    uint32_t w[4] = {0, 0, 0, 0};
    const int valid = load_packed16(p, img, bits, w);
    uint32_t count = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) count += (j < valid && ((w[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0xffu) ? 1u : 0u;
    const uint32_t incl = block_inclusive_scan(count, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) p.lengths[img] = ((bits + 7u) >> 3) + p.ff_total[img];
    if (valid == 0) return;
    uint8_t* dst = p.out + (size_t)img * p.out_capacity;
    size_t o = (size_t)(blockIdx.x * 256u + threadIdx.x) * 16u + p.ff_off[(size_t)img * p.nchunks + blockIdx.x] + (incl - count);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < valid) {
            const uint32_t byte = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
            if (o < p.out_capacity) dst[o] = (uint8_t)byte;
            ++o;
            if (byte == 0xffu) {
                if (o < p.out_capacity) dst[o] = 0;
                ++o;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// staging copy
// ---------------------------------------------------------------------------------------------------------------------
struct StageArgs {
    const uint8_t* src;
    uint8_t* dst;
    long npix;
    int src_cs, dst_cs;
    uint32_t lut[64];      // 256 bytes, little-endian
};

__global__ __launch_bounds__(256) void jpeg_stage_u8_kernel(StageArgs p) {
    __shared__ uint32_t lut[64];
    if (threadIdx.x < 64) lut[threadIdx.x] = p.lut[threadIdx.x];
    __syncthreads();
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.npix; i += stride) {
        const uint8_t* s = p.src + i * p.src_cs;
        uint8_t* d = p.dst + i * p.dst_cs;
        for (int ch = 0; ch < 3; ++ch) {
            const uint32_t v = s[ch];
            d[ch] = (uint8_t)((lut[v >> 2] >> (8u * (v & 3u))) & 0xffu);
        }
        if (p.dst_cs == 4) d[3] = 0;
    }
}

bool supported(int H, int W) {
    return H >= T2V_JPEG_MIN_DIM && H <= T2V_JPEG_MAX_DIM && W >= T2V_JPEG_MIN_DIM && W <= T2V_JPEG_MAX_DIM;
}

}  // namespace

extern "C" {

int t2v_jpeg_abi_version(void) { return T2V_JPEG_ABI_VERSION; }

const char* t2v_jpeg_last_error(void) { return g_error; }

int t2v_jpeg_supported(int H, int W) { return supported(H, W) ? 1 : 0; }

size_t t2v_jpeg_workspace_bytes(int H, int W, int nimg) {
    if (!supported(H, W) || nimg < 1 || nimg > T2V_JPEG_MAX_IMAGES) return 0;
    return carve(geometry(H, W), nimg, nullptr).bytes;
}

size_t t2v_jpeg_scan_capacity(int H, int W) {
    if (!supported(H, W)) return 0;
    return (size_t)geometry(H, W).nblocks * kBlockBytes * 2;
}

int t2v_jpeg_stage_u8(void* stream, const uint8_t* src, int src_cs, uint8_t* dst, int dst_cs, long npix, const uint8_t* lut) {
    JPEG_REQUIRE(src && dst, "t2v_jpeg_stage_u8: null image");
    JPEG_REQUIRE((src_cs == 3 || src_cs == 4) && (dst_cs == 3 || dst_cs == 4), "t2v_jpeg_stage_u8: channel strides %d -> %d (3 or 4)",
                 src_cs, dst_cs);
    JPEG_REQUIRE(npix >= 1 && npix <= (long)T2V_JPEG_MAX_DIM * T2V_JPEG_MAX_DIM, "t2v_jpeg_stage_u8: %ld pixels", npix);
    StageArgs a;
    a.src = src;
    a.dst = dst;
    a.npix = npix;
    a.src_cs = src_cs;
    a.dst_cs = dst_cs;
    for (int i = 0; i < 64; ++i) {
        uint32_t v = 0;
        for (int j = 0; j < 4; ++j) v |= (uint32_t)(lut ? lut[4 * i + j] : 4 * i + j) << (8 * j);
        a.lut[i] = v;
    }
    const long blocks = (npix + 255) / 256;
    hipLaunchKernelGGL(jpeg_stage_u8_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, (hipStream_t)stream, a);
    JPEG_HIP_CHECK(hipGetLastError());
    return T2V_JPEG_OK;
}

int t2v_jpeg_encode_u8(void* stream, const uint8_t* src, int src_cs, int H, int W, int nimg, int quality, void* workspace,
                       uint8_t* out, size_t out_capacity, uint32_t* lengths) {
    JPEG_REQUIRE(supported(H, W), "t2v_jpeg_encode_u8: %dx%d is outside %d..%d per dimension", H, W, T2V_JPEG_MIN_DIM,
                 T2V_JPEG_MAX_DIM);
    JPEG_REQUIRE(src_cs == 3 || src_cs == 4, "t2v_jpeg_encode_u8: src_cs %d (3 or 4)", src_cs);
    JPEG_REQUIRE(nimg >= 1 && nimg <= T2V_JPEG_MAX_IMAGES, "t2v_jpeg_encode_u8: %d images (1..%d)", nimg, T2V_JPEG_MAX_IMAGES);
    JPEG_REQUIRE(quality >= 1 && quality <= 100, "t2v_jpeg_encode_u8: quality %d (1..100)", quality);
    JPEG_REQUIRE(src && workspace && out && lengths, "t2v_jpeg_encode_u8: null pointer");
    JPEG_REQUIRE(((uintptr_t)workspace & 255u) == 0, "t2v_jpeg_encode_u8: the workspace must be 256-byte aligned");
    JPEG_REQUIRE(out_capacity >= 1, "t2v_jpeg_encode_u8: out_capacity 0");
    const hipStream_t s = (hipStream_t)stream;
    const Geom g = geometry(H, W);
    const Workspace w = carve(g, nimg, workspace);
    const size_t packed_bytes = (size_t)g.nchunks * kChunkBytes;

    JPEG_HIP_CHECK(hipMemsetAsync(w.packed, 0, (size_t)nimg * packed_bytes, s));

    McuArgs m;
    m.src = src;
    m.coef = w.coef;
    m.H = H;
    m.W = W;
    m.cs = src_cs;
    m.mw = g.mw;
    m.bw = g.bw;
    m.bh = g.bh;
    m.nmcu = g.nmcu;
    m.scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    hipLaunchKernelGGL(jpeg_mcu_kernel, dim3(g.nmcu, nimg), dim3(64), 0, s, m);
    JPEG_HIP_CHECK(hipGetLastError());

    BlockArgs b;
    b.coef = w.coef;
    b.bits = w.bits;
    b.bit_off = w.bit_off;
    b.packed = w.packed;
    b.nblocks = g.nblocks;
    b.packed_dwords = (uint32_t)(packed_bytes / 4);
    const dim3 block_grid((g.nblocks + 255) / 256, nimg);
    hipLaunchKernelGGL(jpeg_block_bits_kernel, block_grid, dim3(256), 0, s, b);
    JPEG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(nimg), dim3(256), 0, s, (const uint32_t*)w.bits, w.bit_off, w.bit_total, g.nblocks);
    JPEG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_block_pack_kernel, block_grid, dim3(256), 0, s, b);
    JPEG_HIP_CHECK(hipGetLastError());

    StuffArgs f;
    f.packed = w.packed;
    f.bit_total = w.bit_total;
    f.ff_count = w.ff_count;
    f.ff_off = w.ff_off;
    f.ff_total = w.ff_total;
    f.out = out;
    f.lengths = lengths;
    f.out_capacity = out_capacity;
    f.nchunks = g.nchunks;
    const dim3 chunk_grid(g.nchunks, nimg);
    hipLaunchKernelGGL(jpeg_ff_count_kernel, chunk_grid, dim3(256), 0, s, f);
    JPEG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(nimg), dim3(256), 0, s, (const uint32_t*)w.ff_count, w.ff_off, w.ff_total, g.nchunks);
    JPEG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(jpeg_stuff_kernel, chunk_grid, dim3(256), 0, s, f);
    JPEG_HIP_CHECK(hipGetLastError());
    return T2V_JPEG_OK;
}

}  // extern "C"
