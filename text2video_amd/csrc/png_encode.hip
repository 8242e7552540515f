// libt2v_png.so (include/t2v_png.h): lossless PNG files of uint8 RGB images on the GPU, byte for byte the file of the
// numpy restatement tests/png_reference.py.  DESIGN.md section 4.12 has the format rules.
//
// One call = one memset and seven launches, the same for every content:
//   1. png_filter_kernel     one wave per row: the five filter types' sums of absolute residuals, the chosen row into the
//                            workspace, and the row's Adler-32 partial sums.
//   2. png_hist_kernel       one workgroup per band of 8 rows: the band in LDS, run boundaries by a segmented look-up over
//                            the threads' segments, the literal/length histogram in LDS (integer atomics).
//   3. png_code_kernel       one wave per band: all lanes rank the used symbols by (count, symbol), deal out the lengths,
//                            assign the canonical codes and add up the band's bit count from the histogram; lane 0 runs
//                            the chains: the limited minimum-redundancy lengths, the run-length coded lengths with their
//                            own limit-7 code, the packed block header.
//   4. png_prepare_kernel    one workgroup per image: prefix sum of the bands' bit counts, the rows' Adler sums combined.
//   5. png_pack_kernel       one workgroup per band: the header is OR-ed in at the band's bit offset, every thread counts
//                            the bits of its segment's tokens, a prefix sum, then the same walk writes the codes LSB-first
//                            into the zeroed dword stream.  Dwords that lie wholly inside a thread's bits are plain stores;
//                            its first and last may be shared and are OR-ed in (atomicOr: the order does not matter).
//   6. png_crc_copy_kernel   4096-byte chunks of "IDAT" + 78 01 + stream + Adler: copied to the file (never past
//                            out_capacity); every thread's CRC of its 16 bytes times x^(8 x bytes behind it) mod P is
//                            XOR-ed into the image's CRC (atomicXor: the order does not matter).
//   7. png_close_kernel      signature, IHDR, the IDAT's length, its CRC, IEND, lengths[img].
// Integer arithmetic only, no inline assembly; every store is a vector store.  2 and 5 share one token walk
// (walk_segment) with three sinks, so a token counted is a token written.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/t2v_png.h"

namespace {

thread_local char g_error[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
}

#define PNG_HIP_CHECK(expr)                                                                           \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) {                                                                       \
            set_error("%s:%d: %s -> %s", __FILE__, __LINE__, #expr, hipGetErrorString(_e));           \
            return T2V_PNG_ERR_HIP;                                                                   \
        }                                                                                             \
    } while (0)
#define PNG_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            set_error(__VA_ARGS__);       \
            return T2V_PNG_ERR_INVALID;   \
        }                                 \
    } while (0)
#define PNG_HD __host__ __device__ __forceinline__

constexpr int kBandRows = T2V_PNG_BAND_ROWS;
constexpr int kSyms = 286;             // literal/length symbols
constexpr int kSymPitch = 288;         // per-band table pitch (dwords)
constexpr int kEob = 256;
constexpr int kHdrWords = 68;          // >= ceil(2083 / 32) + 1 dwords of packed block header
constexpr int kHdrPitch = 72;          // [kHdrWords]: header bits, [kHdrWords + 1]: the band's bits (header .. EOB)
constexpr int kHeaderBitsMax = 2083;   // include/t2v_png.h, t2v_png_file_capacity
constexpr int kMaxBandBytes = kBandRows * (1 + 3 * T2V_PNG_MAX_DIM);      // 49160
constexpr int kChunkBytes = 4096;      // of the IDAT per workgroup of the CRC / copy kernel (256 threads x 16)
constexpr int kHeadBytes = 37;         // signature 8, IHDR 25, the IDAT's length 4: the file offset of "IDAT"
constexpr uint32_t kAdlerMod = 65521u;
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// ---------------------------------------------------------------------------------------------------------------------
// geometry and workspace
// ---------------------------------------------------------------------------------------------------------------------
struct Geom {
    int H, W, row, nbands;       // row = 1 + 3 W filtered bytes
    size_t filt_bytes;           // H * row
    size_t deflate_cap;          // bytes no Deflate stream exceeds
    size_t packed_bytes;         // per image, a multiple of 256, >= deflate_cap + 8
    int nchunks;                 // kChunkBytes chunks of the longest IDAT (type, zlib header, stream, Adler)
};

Geom geometry(int H, int W) {
    Geom g;
    g.H = H;
    g.W = W;
    g.row = 1 + 3 * W;
    g.nbands = (H + kBandRows - 1) / kBandRows;
    g.filt_bytes = (size_t)H * g.row;
    const size_t bits = (size_t)g.nbands * (kHeaderBitsMax + 15) + 15 * g.filt_bytes;
    g.deflate_cap = (bits + 7) / 8;
    g.packed_bytes = (g.deflate_cap + 8 + 255) / 256 * 256;
    g.nchunks = (int)((g.deflate_cap + 10 + kChunkBytes - 1) / kChunkBytes);
    return g;
}

struct Workspace {
    uint8_t* zeroed;         // packed [nimg][packed_bytes], then crc [nimg]: one memset
    size_t zeroed_bytes;
    uint8_t* packed;
    uint32_t* crc;           // [nimg]
    uint8_t* filt;           // [nimg][round256(filt_bytes)]
    size_t filt_pitch;
    uint32_t* hist;          // [nimg][nbands][kSymPitch]
    uint32_t* table;         // [nimg][nbands][kSymPitch]: bit-reversed code | length << 16
    uint32_t* hdr;           // [nimg][nbands][kHdrPitch]
    uint32_t* band_off;      // [nimg][nbands]
    uint32_t* rowsum;        // [nimg][H][2]
    uint32_t* meta;          // [nimg][4]: total bits, Adler-32
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
    w.zeroed_bytes = n * g.packed_bytes + round256(n * sizeof(uint32_t));
    w.zeroed = take(w.zeroed_bytes);
    w.packed = w.zeroed;
    w.crc = (uint32_t*)(w.zeroed + n * g.packed_bytes);
    w.filt_pitch = round256(g.filt_bytes);
    w.filt = take(n * w.filt_pitch);
    w.hist = (uint32_t*)take(n * g.nbands * kSymPitch * sizeof(uint32_t));
    w.table = (uint32_t*)take(n * g.nbands * kSymPitch * sizeof(uint32_t));
    w.hdr = (uint32_t*)take(n * g.nbands * kHdrPitch * sizeof(uint32_t));
    w.band_off = (uint32_t*)take(n * g.nbands * sizeof(uint32_t));
    w.rowsum = (uint32_t*)take(n * g.H * 2 * sizeof(uint32_t));
    w.meta = (uint32_t*)take(n * 4 * sizeof(uint32_t));
    w.bytes = off;
    return w;
}

// ---------------------------------------------------------------------------------------------------------------------
// 1. row filters
// ---------------------------------------------------------------------------------------------------------------------
// the five residuals of byte x with left a, up b, up-left c
PNG_HD void filter_residuals(int x, int a, int b, int c, int (&r)[5]) {
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    r[0] = x;
    r[1] = (x - a) & 255;
    r[2] = (x - b) & 255;
    r[3] = (x - ((a + b) >> 1)) & 255;
    r[4] = (x - paeth) & 255;
}

// byte i of row y's 3 W colour bytes; 0 left of or above the image
PNG_HD int image_byte(const uint8_t* im, int W, int cs, int y, int i) {
    if (y < 0 || i < 0) return 0;
    return im[((size_t)y * W + i / 3) * cs + i % 3];
}

struct FilterArgs {
    const uint8_t* src;
    uint8_t* filt;
    uint32_t* rowsum;
    size_t filt_pitch;
    int H, W, cs, row;
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(64) void png_filter_kernel(FilterArgs p) {
    const int lane = threadIdx.x, y = blockIdx.x, img = blockIdx.y;
    const uint8_t* im = p.src + (size_t)img * p.H * p.W * p.cs;
    const int n3 = 3 * p.W;
    uint64_t cost[5] = {0, 0, 0, 0, 0};
    for (int i = lane; i < n3; i += 64) {
        int r[5];
        filter_residuals(image_byte(im, p.W, p.cs, y, i), image_byte(im, p.W, p.cs, y, i - 3), image_byte(im, p.W, p.cs, y - 1, i),
                         y > 0 ? image_byte(im, p.W, p.cs, y - 1, i - 3) : 0, r);
#pragma unroll
        for (int t = 0; t < 5; ++t) cost[t] += (uint64_t)(r[t] < 256 - r[t] ? r[t] : 256 - r[t]);
    }
    int type = 0;
    uint64_t best = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
        const uint64_t c = wave_sum(cost[t]);
        if (t == 0 || c < best) {      // the lowest type on a tie
            best = c;
            type = t;
        }
    }
    uint8_t* dst = p.filt + (size_t)img * p.filt_pitch + (size_t)y * p.row;
    uint64_t a = 0, b = 0;      // sum of the bytes; sum of (row - index) * byte
    if (lane == 0) {
        dst[0] = (uint8_t)type;
        a = (uint64_t)type;
        b = (uint64_t)type * (uint64_t)p.row;
    }
    for (int i = lane; i < n3; i += 64) {
        int r[5];
        filter_residuals(image_byte(im, p.W, p.cs, y, i), image_byte(im, p.W, p.cs, y, i - 3), image_byte(im, p.W, p.cs, y - 1, i),
                         y > 0 ? image_byte(im, p.W, p.cs, y - 1, i - 3) : 0, r);
        int v = r[0];
#pragma unroll
        for (int t = 1; t < 5; ++t) v = type == t ? r[t] : v;
        dst[1 + i] = (uint8_t)v;
        a += (uint64_t)v;
        b += (uint64_t)v * (uint64_t)(p.row - 1 - i);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) {
        uint32_t* rs = p.rowsum + ((size_t)img * p.H + y) * 2;
        rs[0] = (uint32_t)(a % kAdlerMod);
        rs[1] = (uint32_t)(b % kAdlerMod);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// tokens: literals and distance-1 matches over the maximal runs of a band
// ---------------------------------------------------------------------------------------------------------------------
// match length 3..258 -> literal/length symbol, number of extra bits, their value (RFC 1951 3.2.5)
PNG_HD void length_symbol(int len, int& sym, int& xbits, int& xval) {
    if (len == 258) {
        sym = 285;
        xbits = xval = 0;
        return;
    }
    const int l = len - 3;
    if (l < 8) {
        sym = 257 + l;
        xbits = xval = 0;
        return;
    }
    int lg = 3;      // floor(log2 l), l in 8..254
    while ((l >> (lg + 1)) > 0) ++lg;
    const int e = lg - 2;
    sym = 257 + 4 * (e + 1) + ((l >> e) & 3);
    xbits = e;
    xval = l & ((1 << e) - 1);
}

PNG_HD int symbol_extra_bits(int sym) { return (sym >= 265 && sym <= 284) ? (sym - 261) >> 2 : 0; }

// The tokens that START in [lo, hi) of a band of n bytes.  rs: the start of the run that holds lo; next_fb: the first run
// boundary at or behind hi (n: none).  Every index read lies in [lo, hi); every length follows from rs, next_fb and those.
template <class Sink>
PNG_HD void walk_segment(const uint8_t* band, int lo, int hi, int rs, int next_fb, Sink& sink) {
    int i = lo;
    while (i < hi) {
        const int v = band[i];
        int re = i + 1;
        while (re < hi && band[re] == v) ++re;
        if (re == hi) re = next_fb;
        const int R = re - rs - 1;
        const int end = re < hi ? re : hi;
        while (i < end) {
            const int j = i - rs;
            if (j == 0) {
                sink.literal(v);
                ++i;
                continue;
            }
            const int k = j - 1, c = k - k % 258;
            const int len = R - c < 258 ? R - c : 258;
            if (len < 3) {
                sink.literal(v);
                ++i;
            } else {
                if (k == c) sink.match(len);
                i = rs + 1 + c + len;      // the next chunk of the run, or its end
            }
        }
        rs = re;
    }
}

// first and last run boundary of [lo, hi) (a boundary: position 0, or a byte unlike the one before); n / -1: none
PNG_HD void segment_boundaries(const uint8_t* band, int n, int lo, int hi, int& first, int& last) {
    first = n;
    last = -1;
    for (int i = lo; i < hi; ++i)
        if (i == 0 || band[i] != band[i - 1]) {
            if (first == n) first = i;
            last = i;
        }
}

struct HistSink {
    uint32_t* hist;
    __device__ __forceinline__ void literal(int v) { atomicAdd(&hist[v], 1u); }
    __device__ __forceinline__ void match(int len) {
        int sym, xb, xv;
        length_symbol(len, sym, xb, xv);
        atomicAdd(&hist[sym], 1u);
    }
};

struct CountSink {
    const uint32_t* table;
    uint32_t n = 0;
    PNG_HD void literal(int v) { n += table[v] >> 16; }
    PNG_HD void match(int len) {
        int sym, xb, xv;
        length_symbol(len, sym, xb, xv);
        n += (table[sym] >> 16) + (uint32_t)xb + 1u;
    }
};

// LSB-first into little-endian dwords, starting at any bit offset.  kAtomic false: a host build for checks.
template <bool kAtomic>
struct PackSink {
    const uint32_t* table;
    uint32_t* words;       // the image's stream
    uint32_t w, limit;     // next dword, dwords in the stream
    uint64_t acc;          // the low n bits are pending (the first dword's low bits, a neighbour's, count as zeros)
    int n;
    bool first;
    PNG_HD void or_in(uint32_t v) {
        if (w >= limit) return;
#if defined(__HIP_DEVICE_COMPILE__)
        if (kAtomic) {
            atomicOr(&words[w], v);
            return;
        }
#endif
        words[w] |= v;
    }
    PNG_HD void begin(uint32_t bit_offset) {
        w = bit_offset >> 5;
        n = (int)(bit_offset & 31u);
        acc = 0;
        first = true;
    }
    PNG_HD void put(uint32_t v, int len) {
        acc |= (uint64_t)v << n;
        n += len;
        if (n >= 32) {
            if (first)
                or_in((uint32_t)acc);
            else if (w < limit)
                words[w] = (uint32_t)acc;
            first = false;
            ++w;
            acc >>= 32;
            n -= 32;
        }
    }
    PNG_HD void finish() {
        if (n > 0) or_in((uint32_t)acc);
    }
    PNG_HD void literal(int v) { put(table[v] & 0xffffu, (int)(table[v] >> 16)); }
    PNG_HD void match(int len) {
        int sym, xb, xv;
        length_symbol(len, sym, xb, xv);
        const int cl = (int)(table[sym] >> 16);
        // the length code, its extra bits, the 1-bit distance code 0: at most 15 + 5 + 1 bits
        put((table[sym] & 0xffffu) | ((uint32_t)xv << cl), cl + xb + 1);
    }
};

// ---------------------------------------------------------------------------------------------------------------------
// 3. codes
// ---------------------------------------------------------------------------------------------------------------------
struct CodeScratch {
    uint32_t cnt[kSymPitch];
    uint32_t A[kSymPitch];
    uint16_t order[kSymPitch];
    uint8_t len[kSymPitch];
    uint8_t seq[kSymPitch];      // the HLIT + 1 code lengths that are run-length coded
    uint32_t num[16];
    uint32_t next[16];
    uint32_t sums[4];
    uint32_t cl_cnt[19], cl_table[19];
    uint16_t cl_order[19];
    uint8_t cl_len[19];
    uint32_t hdr[kHdrPitch];
};

PNG_HD uint32_t reverse_bits(uint32_t v, int n) {
#if defined(__HIP_DEVICE_COMPILE__)
    return n ? __brev(v) >> (32 - n) : 0u;
#endif
    uint32_t r = 0;
    for (int i = 0; i < n; ++i) r |= ((v >> i) & 1u) << (n - 1 - i);
    return r;
}

// the used symbols of cnt[0..nsym) ascending by (count, symbol): insertion sort, for small alphabets and host checks
PNG_HD int sort_used_serial(const uint32_t* cnt, int nsym, uint16_t* order) {
    int n = 0;
    for (int s = 0; s < nsym; ++s) {
        if (!cnt[s]) continue;
        int i = n++;
        while (i > 0 && cnt[order[i - 1]] > cnt[s]) {      // equal counts keep symbol order
            order[i] = order[i - 1];
            --i;
        }
        order[i] = (uint16_t)s;
    }
    return n;
}

// The number of codes of every length 1..limit (<= 15), num[0..15], for the n >= 1 used symbols order[0..n) (ascending by
// (count, symbol)): Moffat and Katajainen's in-place minimum-redundancy lengths on A, then the Kraft repair of the
// restatement.  Serial: one thread.
PNG_HD void length_counts(const uint32_t* cnt, const uint16_t* order, int n, int limit, uint32_t* A, uint32_t* num) {
    if (n == 1) {
        for (int i = 0; i <= 15; ++i) num[i] = i == 1 ? 1u : 0u;
        return;
    }
    for (int i = 0; i < n; ++i) A[i] = cnt[order[i]];
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) {
            A[next] = A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] = A[leaf++];
        }
        if (leaf >= n || (root < next && A[root] < A[leaf])) {
            A[next] += A[root];
            A[root++] = (uint32_t)next;
        } else {
            A[next] += A[leaf++];
        }
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next]] + 1;
    {
        int avbl = 1, used = 0, dpth = 0, r = n - 2, next = n - 1;
        while (avbl > 0) {
            while (r >= 0 && (int)A[r] == dpth) {
                ++used;
                --r;
            }
            while (avbl > used) {
                A[next--] = (uint32_t)dpth;
                --avbl;
            }
            avbl = 2 * used;
            ++dpth;
            used = 0;
        }
    }
    for (int i = 0; i <= 15; ++i) num[i] = 0;
    for (int i = 0; i < n; ++i) num[(int)A[i] > limit ? limit : (int)A[i]] += 1;
    uint32_t total = 0;
    for (int i = 1; i <= limit; ++i) total += num[i] << (limit - i);
    while (total > (1u << limit)) {      // (a minimum-redundancy code is complete: folding can only overfill)
        num[limit] -= 1;
        for (int i = limit - 1; i > 0; --i)
            if (num[i]) {
                num[i] -= 1;
                num[i + 1] += 2;
                break;
            }
        total -= 1;
    }
}

// the length of the symbol at place j of the sorted order: the lengths are dealt out shortest first from the frequent end
PNG_HD int dealt_length(const uint32_t* num, int n, int j) {
    const uint32_t e = (uint32_t)(n - 1 - j);
    int len = 1;
    uint32_t cum = num[1];
    while (e >= cum && len < 15) cum += num[++len];
    return len;
}

// Code lengths <= limit for a small alphabet, serially; len[0..nsym) is written.
PNG_HD void limited_lengths(const uint32_t* cnt, const uint16_t* order, int n, int nsym, int limit, uint32_t* A, uint32_t* num,
                            uint8_t* len) {
    for (int s = 0; s < nsym; ++s) len[s] = 0;
    if (n == 0) return;
    length_counts(cnt, order, n, limit, A, num);
    for (int j = 0; j < n; ++j) len[order[j]] = (uint8_t)dealt_length(num, n, j);
}

// RFC 1951 3.2.2; table[s] = bit-reversed code | length << 16
PNG_HD void canonical_table(const uint8_t* len, int nsym, uint32_t* num, uint32_t* next, uint32_t* table) {
    for (int i = 0; i <= 15; ++i) num[i] = 0;
    for (int s = 0; s < nsym; ++s) num[len[s]] += 1;
    num[0] = 0;
    uint32_t code = 0;
    next[0] = 0;
    for (int bits = 1; bits <= 15; ++bits) {
        code = (code + num[bits - 1]) << 1;
        next[bits] = code;
    }
    for (int s = 0; s < nsym; ++s) {
        const int l = len[s];
        table[s] = l ? (reverse_bits(next[l]++, l) | ((uint32_t)l << 16)) : 0u;
    }
}

// the fixed greedy run-length rule of the restatement over seq[0..n)
template <class Sink>
PNG_HD void rle_walk(const uint8_t* seq, int n, Sink& sink) {
    int i = 0;
    while (i < n) {
        const int v = seq[i];
        int j = i;
        while (j < n && seq[j] == v) ++j;
        int r = j - i;
        i = j;
        if (v == 0) {
            while (r >= 11) {
                const int m = r < 138 ? r : 138;
                sink.emit(18, 7, m - 11);
                r -= m;
            }
            if (r >= 3) {
                sink.emit(17, 3, r - 3);
                r = 0;
            }
        } else {
            sink.emit(v, 0, 0);
            r -= 1;
            while (r >= 3) {
                const int m = r < 6 ? r : 6;
                sink.emit(16, 2, m - 3);
                r -= m;
            }
        }
        for (; r > 0; --r) sink.emit(v, 0, 0);
    }
}

struct ClCountSink {
    uint32_t* cnt;
    PNG_HD void emit(int sym, int, int) { cnt[sym] += 1; }
};

struct HeaderBits {
    uint32_t* words;      // kHdrWords, zeroed
    uint32_t pos = 0;
    PNG_HD void put(uint32_t v, int n) {
        if (n == 0) return;
        const uint32_t w = pos >> 5, s = pos & 31u;
        if (w < (uint32_t)kHdrWords) words[w] |= v << s;
        if (s + (uint32_t)n > 32u && w + 1 < (uint32_t)kHdrWords) words[w + 1] |= v >> (32u - s);
        pos += (uint32_t)n;
    }
};

struct ClEmitSink {
    HeaderBits* bits;
    const uint32_t* table;
    PNG_HD void emit(int sym, int xbits, int xval) {
        bits->put(table[sym] & 0xffffu, (int)(table[sym] >> 16));
        bits->put((uint32_t)xval, xbits);
    }
};

struct NoSync {
    PNG_HD void operator()() const {}
};

PNG_HD void shared_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

PNG_HD void shared_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}

// One band's block, from its histogram s.cnt (end-of-block counted) and the sorted used symbols s.order[0..n): the code
// table into table[0..kSymPitch), and s.hdr = the packed header, its bit count and the block's bit count.  Run by `nlanes`
// threads (lane 0 .. nlanes - 1, all of them), `sync` a barrier between them: what is per symbol is spread over the lanes,
// what is a chain (the minimum-redundancy lengths, the run-length coding, the header's bits) is lane 0's.
template <class Sync>
PNG_HD void build_block(CodeScratch& s, int n, bool final, uint32_t* table, int lane, int nlanes, Sync sync) {
    const uint8_t kClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int sym = lane; sym < kSymPitch; sym += nlanes) s.len[sym] = 0;
    if (lane == 0) {
        length_counts(s.cnt, s.order, n, 15, s.A, s.num);
        // RFC 1951 3.2.2: the first code of every length (s.num is the count per length)
        uint32_t code = 0;
        s.next[0] = 0;
        for (int bits = 1; bits <= 15; ++bits) {
            code = (code + (bits > 1 ? s.num[bits - 1] : 0u)) << 1;
            s.next[bits] = code;
        }
        s.sums[0] = s.sums[1] = 0;      // the block's token bits, its matches
        s.sums[2] = 257;                // HLIT
    }
    sync();
    for (int j = lane; j < n; j += nlanes) s.len[s.order[j]] = (uint8_t)dealt_length(s.num, n, j);
    sync();
    for (int sym = lane; sym < kSymPitch; sym += nlanes) {
        const int l = sym < kSyms ? s.len[sym] : 0;
        uint32_t before = 0;      // symbols of the same length in front of this one: codes of a length go in symbol order
        if (l)
            for (int t = 0; t < sym; ++t) before += s.len[t] == l ? 1u : 0u;
        table[sym] = l ? (reverse_bits(s.next[l] + before, l) | ((uint32_t)l << 16)) : 0u;
        if (l) {
            shared_add(&s.sums[0], s.cnt[sym] * ((uint32_t)l + (uint32_t)symbol_extra_bits(sym)));
            if (sym >= 257) {
                shared_add(&s.sums[1], s.cnt[sym]);
                shared_max(&s.sums[2], (uint32_t)sym + 1u);
            }
        }
    }
    sync();
    const int hlit = (int)s.sums[2];
    for (int i = lane; i < hlit; i += nlanes) s.seq[i] = s.len[i];
    for (int i = lane; i < kHdrPitch; i += nlanes) s.hdr[i] = 0;
    sync();
    if (lane != 0) return;
    const uint32_t matches = s.sums[1], bits = s.sums[0] + matches;      // (+ the 1-bit distance code of every match)
    s.seq[hlit] = matches ? 1 : 0;
    for (int i = 0; i < 19; ++i) s.cl_cnt[i] = 0;
    ClCountSink count{s.cl_cnt};
    rle_walk(s.seq, hlit + 1, count);
    const int ncl = sort_used_serial(s.cl_cnt, 19, s.cl_order);
    limited_lengths(s.cl_cnt, s.cl_order, ncl, 19, 7, s.A, s.num, s.cl_len);
    canonical_table(s.cl_len, 19, s.num, s.next, s.cl_table);
    int hclen = 4;
    for (int i = 0; i < 19; ++i)
        if (s.cl_len[kClOrder[i]] && i + 1 > hclen) hclen = i + 1;
    HeaderBits h{s.hdr};
    h.put(final ? 1u : 0u, 1);
    h.put(2u, 2);
    h.put((uint32_t)(hlit - 257), 5);
    h.put(0u, 5);
    h.put((uint32_t)(hclen - 4), 4);
    for (int i = 0; i < hclen; ++i) h.put(s.cl_len[kClOrder[i]], 3);
    ClEmitSink emit{&h, s.cl_table};
    rle_walk(s.seq, hlit + 1, emit);
    s.hdr[kHdrWords] = h.pos;
    s.hdr[kHdrWords + 1] = h.pos + bits;
}

// ---------------------------------------------------------------------------------------------------------------------
// CRC-32 arithmetic (reflected, polynomial 0xEDB88320): products and powers of x modulo P, as zlib's crc32_combine does
// ---------------------------------------------------------------------------------------------------------------------
PNG_HD uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t m = 1u << 31, p = 0;
    for (;;) {
        if (a & m) {
            p ^= b;
            if ((a & (m - 1)) == 0) break;
        }
        m >>= 1;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}

struct X2n {
    uint32_t v[32];      // x^(2^k) mod P
};

X2n make_x2n() {
    X2n t;
    uint32_t p = 1u << 30;      // x^1
    t.v[0] = p;
    for (int k = 1; k < 32; ++k) t.v[k] = p = multmodp(p, p);
    return t;
}

// x^(8 n) mod P
PNG_HD uint32_t x8nmodp(const uint32_t* x2n, uint32_t n) {
    uint32_t p = 1u << 31;      // x^0
    int k = 3;
    while (n) {
        if (n & 1u) p = multmodp(x2n[k & 31], p);
        n >>= 1;
        ++k;
    }
    return p;
}

// the register after one more byte; no initial value, no final complement (the linear part of the CRC)
PNG_HD uint32_t crc_byte(uint32_t c, uint32_t byte) {
    c ^= byte;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
    return c;
}

uint32_t host_crc32(const uint8_t* d, size_t n) {
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = crc_byte(c, d[i]);
    return c ^ 0xFFFFFFFFu;
}

// byte j of "IDAT", 78 01, the nd bytes of the stream, Adler-32 (big-endian)
PNG_HD uint32_t idat_byte(const uint8_t* packed, uint32_t nd, uint32_t adler, uint32_t j) {
    if (j < 4) return (uint32_t)("IDAT"[j]);
    if (j < 6) return j == 4 ? 0x78u : 0x01u;
    if (j < 6 + nd) return packed[j - 6];
    return (adler >> (8u * (3u - (j - 6u - nd)))) & 0xffu;
}

// ---------------------------------------------------------------------------------------------------------------------
// kernels 2 .. 7
// ---------------------------------------------------------------------------------------------------------------------
struct BandArgs {
    const uint8_t* filt;
    size_t filt_pitch;
    uint32_t* hist;
    uint32_t* table;
    uint32_t* hdr;
    const uint32_t* band_off;
    uint8_t* packed;
    size_t packed_bytes;
    int H, row, nbands;
};

// the band into LDS; its byte count
__device__ __forceinline__ int load_band(const BandArgs& p, int band, int img, uint8_t* lds) {
    const int rows = min(kBandRows, p.H - band * kBandRows);
    const int n = rows * p.row;
    const uint8_t* src = p.filt + (size_t)img * p.filt_pitch + (size_t)band * kBandRows * p.row;
    for (int i = threadIdx.x; i < n; i += 256) lds[i] = src[i];
    return n;
}

// this thread's segment [lo, hi) of the band, the start of the run that holds lo and the first boundary at or behind hi
__device__ __forceinline__ void thread_segment(const uint8_t* band, int n, int* first_of, int* last_of, int& lo, int& hi, int& rs,
                                               int& next_fb) {
    const int tid = threadIdx.x, per = (n + 255) / 256;
    lo = min(tid * per, n);
    hi = min(lo + per, n);
    int first, last;
    segment_boundaries(band, n, lo, hi, first, last);
    first_of[tid] = first;
    last_of[tid] = last;
    __syncthreads();
    rs = 0;
    if (lo < hi && first != lo)      // (position 0 is a boundary: thread 0 never looks back)
        for (int t = tid - 1; t >= 0; --t)
            if (last_of[t] >= 0) {
                rs = last_of[t];
                break;
            }
    if (first == lo) rs = lo;
    next_fb = n;
    for (int t = tid + 1; t < 256; ++t)
        if (first_of[t] < n) {
            next_fb = first_of[t];
            break;
        }
}

__global__ __launch_bounds__(256) void png_hist_kernel(BandArgs p) {
    __shared__ uint8_t band[kMaxBandBytes];
    __shared__ uint32_t hist[kSymPitch];
    __shared__ int first_of[256], last_of[256];
    const int b = blockIdx.x, img = blockIdx.y;
    const int n = load_band(p, b, img, band);
    for (int i = threadIdx.x; i < kSymPitch; i += 256) hist[i] = i == kEob ? 1u : 0u;
    __syncthreads();
    int lo, hi, rs, next_fb;
    thread_segment(band, n, first_of, last_of, lo, hi, rs, next_fb);
    HistSink sink{hist};
    walk_segment(band, lo, hi, rs, next_fb, sink);
    __syncthreads();
    uint32_t* dst = p.hist + ((size_t)img * p.nbands + b) * kSymPitch;
    for (int i = threadIdx.x; i < kSymPitch; i += 256) dst[i] = hist[i];
}

struct BlockSync {
    __device__ __forceinline__ void operator()() const { __syncthreads(); }
};

__global__ __launch_bounds__(64) void png_code_kernel(BandArgs p) {
    __shared__ CodeScratch s;
    __shared__ uint32_t table[kSymPitch];
    __shared__ int used;
    const int lane = threadIdx.x, b = blockIdx.x, img = blockIdx.y;
    const size_t slot = (size_t)img * p.nbands + b;
    const uint32_t* hist = p.hist + slot * kSymPitch;
    for (int i = lane; i < kSymPitch; i += 64) s.cnt[i] = i < kSyms ? hist[i] : 0u;
    if (lane == 0) used = 0;
    __syncthreads();
    // rank of every used symbol by (count, symbol): its place in the sorted order
    for (int sym = lane; sym < kSyms; sym += 64) {
        const uint32_t c = s.cnt[sym];
        if (!c) continue;
        int rank = 0;
        for (int t = 0; t < kSyms; ++t) {
            const uint32_t ct = s.cnt[t];
            rank += (ct != 0u && (ct < c || (ct == c && t < sym))) ? 1 : 0;
        }
        s.order[rank] = (uint16_t)sym;
        atomicAdd(&used, 1);
    }
    __syncthreads();
    build_block(s, used, b == p.nbands - 1, table, lane, 64, BlockSync());
    __syncthreads();
    uint32_t* tdst = p.table + slot * kSymPitch;
    for (int i = lane; i < kSymPitch; i += 64) tdst[i] = table[i];
    uint32_t* hdst = p.hdr + slot * kHdrPitch;
    for (int i = lane; i < kHdrPitch; i += 64) hdst[i] = s.hdr[i];
}

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

struct PrepareArgs {
    const uint32_t* hdr;
    const uint32_t* rowsum;
    uint32_t* band_off;
    uint32_t* meta;
    int H, row, nbands;
};

__global__ __launch_bounds__(256) void png_prepare_kernel(PrepareArgs p) {
    __shared__ uint32_t red[256];
    __shared__ uint32_t sums[2 * T2V_PNG_MAX_DIM];
    const int tid = threadIdx.x, img = blockIdx.x;
    // nbands <= 256: one band per thread
    const uint32_t bits = tid < p.nbands ? p.hdr[((size_t)img * p.nbands + tid) * kHdrPitch + kHdrWords + 1] : 0u;
    const uint32_t incl = block_inclusive_scan(bits, red);
    if (tid < p.nbands) p.band_off[(size_t)img * p.nbands + tid] = incl - bits;
    for (int i = tid; i < 2 * p.H; i += 256) sums[i] = p.rowsum[(size_t)img * p.H * 2 + i];
    __syncthreads();
    if (tid == 255) p.meta[(size_t)img * 4] = incl;
    if (tid == 0) {
        // Adler-32 over the rows in order: b gains row * a for the bytes of the row, then the row's own weighted sum
        uint32_t a = 1, b = 0;
        const uint32_t n = (uint32_t)p.row % kAdlerMod;
        for (int y = 0; y < p.H; ++y) {
            b = ((n * a) % kAdlerMod + b + sums[2 * y + 1]) % kAdlerMod;      // n, a < 65521: the product fits 32 bits
            a = (a + sums[2 * y]) % kAdlerMod;
        }
        p.meta[(size_t)img * 4 + 1] = (b << 16) | a;
    }
}

__global__ __launch_bounds__(256) void png_pack_kernel(BandArgs p) {
    __shared__ uint8_t band[kMaxBandBytes];
    __shared__ uint32_t table[kSymPitch];
    __shared__ uint32_t red[256];
    __shared__ int first_of[256], last_of[256];
    const int tid = threadIdx.x, b = blockIdx.x, img = blockIdx.y;
    const size_t slot = (size_t)img * p.nbands + b;
    const int n = load_band(p, b, img, band);
    for (int i = tid; i < kSymPitch; i += 256) table[i] = p.table[slot * kSymPitch + i];
    __syncthreads();
    int lo, hi, rs, next_fb;
    thread_segment(band, n, first_of, last_of, lo, hi, rs, next_fb);
    CountSink count{table};
    walk_segment(band, lo, hi, rs, next_fb, count);
    const uint32_t incl = block_inclusive_scan(count.n, red);

    const uint32_t* hdr = p.hdr + slot * kHdrPitch;
    const uint32_t hdr_bits = min(hdr[kHdrWords], (uint32_t)kHeaderBitsMax), band_bits = hdr[kHdrWords + 1];
    const uint32_t off = p.band_off[slot];
    PackSink<true> sink;
    sink.table = table;
    sink.words = reinterpret_cast<uint32_t*>(p.packed + (size_t)img * p.packed_bytes);
    sink.limit = (uint32_t)(p.packed_bytes / 4);
    // the header: dword k of it at bit off + 32 k
    if ((uint32_t)tid * 32u < hdr_bits) {
        sink.begin(off + (uint32_t)tid * 32u);
        sink.put(hdr[tid], (int)min(32u, hdr_bits - (uint32_t)tid * 32u));
        sink.finish();
    }
    sink.begin(off + hdr_bits + (incl - count.n));
    walk_segment(band, lo, hi, rs, next_fb, sink);
    sink.finish();
    if (tid == 255) {      // the end-of-block symbol closes the band: its place follows from the histogram's bit count
        const int eob_len = (int)(table[kEob] >> 16);
        sink.begin(off + band_bits - (uint32_t)eob_len);
        sink.put(table[kEob] & 0xffffu, eob_len);
        sink.finish();
    }
}

struct CloseArgs {
    const uint8_t* packed;
    size_t packed_bytes;
    const uint32_t* meta;
    uint32_t* crc;
    uint8_t* out;
    uint32_t* lengths;
    size_t out_capacity;
    uint32_t deflate_cap;
    uint32_t ihdr_crc;
    int H, W;
    X2n x2n;
};

__global__ __launch_bounds__(256) void png_crc_copy_kernel(CloseArgs p) {
    __shared__ uint32_t red[256];
    const int tid = threadIdx.x, img = blockIdx.y;
    const uint32_t nd = min((p.meta[(size_t)img * 4] + 7u) >> 3, p.deflate_cap), adler = p.meta[(size_t)img * 4 + 1];
    const uint32_t total = 10u + nd;      // type, zlib header, stream, Adler
    const uint32_t j0 = ((uint32_t)blockIdx.x * 256u + (uint32_t)tid) * 16u;
    const uint8_t* packed = p.packed + (size_t)img * p.packed_bytes;
    uint8_t* dst = p.out + (size_t)img * p.out_capacity;
    uint32_t c = 0;
    if (j0 < total) {
        const uint32_t valid = min(16u, total - j0);
        for (uint32_t k = 0; k < valid; ++k) {
            const uint32_t j = j0 + k, byte = idat_byte(packed, nd, adler, j);
            // the CRC's initial value is the first four bytes complemented
            c = crc_byte(c, j < 4 ? byte ^ 0xffu : byte);
            const size_t o = (size_t)kHeadBytes + j;
            if (o < p.out_capacity) dst[o] = (uint8_t)byte;
        }
        c = multmodp(x8nmodp(p.x2n.v, total - (j0 + valid)), c);
    }
    red[tid] = c;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if (tid < d) red[tid] ^= red[tid + d];
        __syncthreads();
    }
    if (tid == 0 && red[0]) atomicXor(&p.crc[img], red[0]);
}

__global__ __launch_bounds__(64) void png_close_kernel(CloseArgs p) {
    const int tid = threadIdx.x, img = blockIdx.x;
    const uint32_t nd = min((p.meta[(size_t)img * 4] + 7u) >> 3, p.deflate_cap);
    const uint32_t total = 10u + nd, idat_len = 6u + nd, crc = p.crc[img] ^ 0xFFFFFFFFu;
    uint8_t* dst = p.out + (size_t)img * p.out_capacity;
    if (tid < kHeadBytes) {
        uint32_t v;
        if (tid < 8)
            v = (uint32_t)(uint8_t)("\x89PNG\r\n\x1a\n"[tid]);
        else if (tid < 16)
            v = (uint32_t)(uint8_t)("\0\0\0\x0dIHDR"[tid - 8]);
        else if (tid < 20)
            v = ((uint32_t)p.W >> (8 * (19 - tid))) & 0xffu;
        else if (tid < 24)
            v = ((uint32_t)p.H >> (8 * (23 - tid))) & 0xffu;
        else if (tid < 29)
            v = tid == 24 ? 8u : tid == 25 ? 2u : 0u;
        else if (tid < 33)
            v = (p.ihdr_crc >> (8 * (32 - tid))) & 0xffu;
        else
            v = (idat_len >> (8 * (36 - tid))) & 0xffu;
        if ((size_t)tid < p.out_capacity) dst[tid] = (uint8_t)v;
    } else if (tid < kHeadBytes + 16) {
        const int k = tid - kHeadBytes;      // the IDAT's CRC, then IEND
        const uint32_t v = k < 4 ? (crc >> (8 * (3 - k))) & 0xffu : (uint32_t)(uint8_t)("\0\0\0\0IEND\xae\x42\x60\x82"[k - 4]);
        const size_t o = (size_t)kHeadBytes + total + (size_t)k;
        if (o < p.out_capacity) dst[o] = (uint8_t)v;
    }
    if (tid == 0) p.lengths[img] = (uint32_t)kHeadBytes + total + 16u;
}

bool supported(int H, int W) {
    return H >= T2V_PNG_MIN_DIM && H <= T2V_PNG_MAX_DIM && W >= T2V_PNG_MIN_DIM && W <= T2V_PNG_MAX_DIM;
}

}  // namespace

extern "C" {

int t2v_png_abi_version(void) { return T2V_PNG_ABI_VERSION; }

const char* t2v_png_last_error(void) { return g_error; }

int t2v_png_supported(int H, int W) { return supported(H, W) ? 1 : 0; }

size_t t2v_png_workspace_bytes(int H, int W, int nimg) {
    if (!supported(H, W) || nimg < 1 || nimg > T2V_PNG_MAX_IMAGES) return 0;
    return carve(geometry(H, W), nimg, nullptr).bytes;
}

size_t t2v_png_file_capacity(int H, int W) {
    if (!supported(H, W)) return 0;
    return geometry(H, W).deflate_cap + 63;
}

int t2v_png_encode_u8(void* stream, const uint8_t* src, int src_cs, int H, int W, int nimg, void* workspace, uint8_t* out,
                      size_t out_capacity, uint32_t* lengths) {
    PNG_REQUIRE(supported(H, W), "t2v_png_encode_u8: %dx%d is outside %d..%d per dimension", H, W, T2V_PNG_MIN_DIM, T2V_PNG_MAX_DIM);
    PNG_REQUIRE(src_cs == 3 || src_cs == 4, "t2v_png_encode_u8: src_cs %d (3 or 4)", src_cs);
    PNG_REQUIRE(nimg >= 1 && nimg <= T2V_PNG_MAX_IMAGES, "t2v_png_encode_u8: %d images (1..%d)", nimg, T2V_PNG_MAX_IMAGES);
    PNG_REQUIRE(src && workspace && out && lengths, "t2v_png_encode_u8: null pointer");
    PNG_REQUIRE(((uintptr_t)workspace & 255u) == 0, "t2v_png_encode_u8: the workspace must be 256-byte aligned");
    PNG_REQUIRE(out_capacity >= 1, "t2v_png_encode_u8: out_capacity 0");
    const hipStream_t s = (hipStream_t)stream;
    const Geom g = geometry(H, W);
    const Workspace w = carve(g, nimg, workspace);

    PNG_HIP_CHECK(hipMemsetAsync(w.zeroed, 0, w.zeroed_bytes, s));

    FilterArgs f;
    f.src = src;
    f.filt = w.filt;
    f.rowsum = w.rowsum;
    f.filt_pitch = w.filt_pitch;
    f.H = H;
    f.W = W;
    f.cs = src_cs;
    f.row = g.row;
    hipLaunchKernelGGL(png_filter_kernel, dim3(H, nimg), dim3(64), 0, s, f);
    PNG_HIP_CHECK(hipGetLastError());

    BandArgs b;
    b.filt = w.filt;
    b.filt_pitch = w.filt_pitch;
    b.hist = w.hist;
    b.table = w.table;
    b.hdr = w.hdr;
    b.band_off = w.band_off;
    b.packed = w.packed;
    b.packed_bytes = g.packed_bytes;
    b.H = H;
    b.row = g.row;
    b.nbands = g.nbands;
    const dim3 band_grid(g.nbands, nimg);
    hipLaunchKernelGGL(png_hist_kernel, band_grid, dim3(256), 0, s, b);
    PNG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(png_code_kernel, band_grid, dim3(64), 0, s, b);
    PNG_HIP_CHECK(hipGetLastError());

    PrepareArgs q;
    q.hdr = w.hdr;
    q.rowsum = w.rowsum;
    q.band_off = w.band_off;
    q.meta = w.meta;
    q.H = H;
    q.row = g.row;
    q.nbands = g.nbands;
    hipLaunchKernelGGL(png_prepare_kernel, dim3(nimg), dim3(256), 0, s, q);
    PNG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(png_pack_kernel, band_grid, dim3(256), 0, s, b);
    PNG_HIP_CHECK(hipGetLastError());

    CloseArgs c;
    c.packed = w.packed;
    c.packed_bytes = g.packed_bytes;
    c.meta = w.meta;
    c.crc = w.crc;
    c.out = out;
    c.lengths = lengths;
    c.out_capacity = out_capacity;
    c.deflate_cap = (uint32_t)g.deflate_cap;
    c.H = H;
    c.W = W;
    static const X2n x2n = make_x2n();
    c.x2n = x2n;
    uint8_t ihdr[17] = {'I', 'H', 'D', 'R', 0, 0, 0, 0, 0, 0, 0, 0, 8, 2, 0, 0, 0};
    for (int k = 0; k < 4; ++k) {
        ihdr[4 + k] = (uint8_t)((uint32_t)W >> (8 * (3 - k)));
        ihdr[8 + k] = (uint8_t)((uint32_t)H >> (8 * (3 - k)));
    }
    c.ihdr_crc = host_crc32(ihdr, sizeof(ihdr));
    hipLaunchKernelGGL(png_crc_copy_kernel, dim3(g.nchunks, nimg), dim3(256), 0, s, c);
    PNG_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(png_close_kernel, dim3(nimg), dim3(64), 0, s, c);
    PNG_HIP_CHECK(hipGetLastError());
    return T2V_PNG_OK;
}

}  // extern "C"
