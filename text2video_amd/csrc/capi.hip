// capi.hip -- extern "C" surface of libt2v_hip.so (declared in include/t2v.h) and the conv planner.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <utility>
#include <vector>

#include "conv_plan.h"

namespace t2v {

static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// ---- environment switches, read once ----
static Options g_opts;
static std::once_flag g_opts_once;
static int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}
static thread_local int g_overlap = 0;
int set_overlap_hint(int on) {
    const int prev = g_overlap;
    g_overlap = on == 2 ? 2 : (on ? 1 : 0);
    return prev;
}
bool overlap_hint() { return g_overlap == 1 && options().overlap_hint != 0; }
int sk_launch_blocks() {
    const int two = wino_gemm_sk_grid_blocks(), mode = options().sk_blocks_per_cu;
    const bool one = mode == 1 || (mode == 0 && g_overlap == 2 && options().overlap_hint != 0);
    return one && two % 16 == 0 ? two / 2 : two;
}
void options_reload() {
    Options o;
    o.wino_gemm_sk = env_int("T2V_WINO_GEMM_SK", 1);
    o.wino_gemm_sk_ragged = env_int("T2V_WINO_GEMM_SK_RAGGED", 2);
    o.overlap_hint = env_int("T2V_OVERLAP_HINT", 1);
    o.overlap_hint_single = env_int("T2V_OVERLAP_HINT_SINGLE", 0);
    o.wgrad_sk = env_int("T2V_WGRAD_SK", 1);
    o.wgrad_combine = env_int("T2V_WGRAD_COMBINE", 1);
    o.wgrad_combine_max = env_int("T2V_WGRAD_COMBINE_MAX", 4);
    o.chain_lazy = env_int("T2V_CHAIN_LAZY", 1);
    o.finalize_direct = env_int("T2V_FINALIZE_DIRECT", 1);
    o.streams = env_int("T2V_STREAMS", 0);
    o.conv_tile = env_int("T2V_CONV_TILE", 0);
    o.xcd_slices = env_int("T2V_XCD_SLICES", 1);
    o.sk_blocks_per_cu = env_int("T2V_SK_BLOCKS_PER_CU", 0);
    g_opts = o;
}
const Options& options() {
    std::call_once(g_opts_once, options_reload);
    return g_opts;
}

// ---- fixed-grid hand-over: sticky error word + dispatch-order self-test ----
static unsigned* g_err_word = nullptr;            // pinned, mapped host memory: kernels store to it, the host reads it
static std::atomic<int> g_fixed_grid_on{1};
static std::mutex g_fg_mutex;
static char g_fg_why[160] = "";
unsigned* async_error_word() { return g_err_word; }
bool fixed_grid_enabled() { return g_fixed_grid_on.load(std::memory_order_relaxed) != 0; }
void fixed_grid_disable(const char* why) {
    std::lock_guard<std::mutex> lk(g_fg_mutex);
    if (g_fixed_grid_on.exchange(0)) {
        snprintf(g_fg_why, sizeof(g_fg_why), "%s", why);
        fprintf(stderr, "libt2v_hip: fixed-grid kernels switched off (%s); running one block per tile\n", why);
    }
}
int check_async_errors() {
    if (!g_err_word || *reinterpret_cast<volatile unsigned*>(g_err_word) == 0) return T2V_OK;
    *reinterpret_cast<volatile unsigned*>(g_err_word) = 0;
    fixed_grid_disable("an accumulator hand-over timed out");
    set_error("a fixed-grid kernel's accumulator hand-over timed out in an earlier launch: the output of that launch holds "
              "NaNs (re-run it); the fixed-grid kernels are now off for this process");
    return T2V_ERR_HANDOVER;
}

// blocks shaped like the fixed-grid kernels' (512 threads, 64 KiB of LDS: two per CU), four rounds of them: each draws a
// ticket as it starts and stays resident for some microseconds
__global__ __launch_bounds__(512) void dispatch_order_kernel(unsigned* counter, unsigned* order) {
    extern __shared__ char smem[];
    if (threadIdx.x == 0) {
        order[blockIdx.x] = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        smem[0] = 0;
    }
    for (int i = 0; i < 64; ++i) __builtin_amdgcn_s_sleep(32);
}
static int fixed_grid_selftest() {
    const int grid = 4 * wino_gemm_sk_grid_blocks();
    unsigned* buf = nullptr;
    T2V_HIP_CHECK(hipMalloc(&buf, (size_t)(grid + 1) * sizeof(unsigned)));
    int st = T2V_OK;
    std::vector<unsigned> host(grid + 1);
    if (hipMemset(buf, 0, (size_t)(grid + 1) * sizeof(unsigned)) != hipSuccess ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(dispatch_order_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            65536) != hipSuccess)
        st = T2V_ERR_HIP;
    if (st == T2V_OK) {
        hipLaunchKernelGGL(dispatch_order_kernel, dim3(grid), dim3(512), 65536, 0, buf, buf + 1);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemcpy(host.data(), buf, (size_t)(grid + 1) * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess)
            st = T2V_ERR_HIP;
    }
    (void)hipFree(buf);
    if (st != T2V_OK) {
        fixed_grid_disable("the dispatch-order self-test could not run");
        return T2V_OK;      // not fatal: the tile-per-block kernels need no such guarantee
    }
    // Start order per XCD (blocks b = x, x + 8, x + 16, ... run on XCD x under round-robin dispatch).  Blocks dispatched
    // within a microsecond of each other draw their tickets in any order, so the check is on DISPLACEMENT: with in-order
    // dispatch a block's rank among its XCD's tickets differs from its index there by less than the blocks the XCD holds
    // at once (a quarter of this launch's blocks per XCD; the limit is twice that); a queue served out of order (LIFO,
    // random, reversed) displaces by the whole over-subscribed length.
    const int per_xcd = grid / 8, limit = per_xcd / 2;
    for (int x = 0; x < 8 && fixed_grid_enabled(); ++x) {
        std::vector<std::pair<unsigned, int>> t(per_xcd);
        for (int q = 0; q < per_xcd; ++q) t[q] = {host[1 + q * 8 + x], q};
        std::sort(t.begin(), t.end());
        for (int r = 0; r < per_xcd; ++r)
            if (abs(t[r].second - r) > limit) {
                char why[160];
                snprintf(why, sizeof(why), "dispatch-order self-test: block %d of XCD %d started %d places from its index",
                         t[r].second * 8 + x, x, abs(t[r].second - r));
                fixed_grid_disable(why);
                break;
            }
    }
    return T2V_OK;
}

int build_conv_plan(const t2v_conv_desc* d, int x_cs, bool need_stats, ConvPlan* out) {
    T2V_REQUIRE(d && out, "null conv descriptor");
    T2V_REQUIRE(d->H > 0 && d->W > 0 && d->Cin > 0 && d->Cout > 0, "conv: bad dims H=%d W=%d Cin=%d Cout=%d", d->H,
                d->W, d->Cin, d->Cout);
    T2V_REQUIRE(x_cs % 4 == 0 && x_cs >= d->Cin, "conv: input channel storage %d must be a multiple of 4 >= Cin=%d",
                x_cs, d->Cin);
    ConvPlan& pl = *out;
    memset(&pl, 0, sizeof(pl));
    pl.Cin = d->Cin;
    ConvKParams& k = pl.kp;
    // the small-Cout tile has no statistics epilogue; weights are always packed to the 128-row
    // granule so either tile can read them
    // narrow outputs (<= 64 channels: the 1024x1024 local enhancer's stems) use the 64x64 tile: half of a 128-wide
    // tile would be padding
    pl.tile = need_stats ? (d->Cout <= 64 ? kTileQ : kTileL) : (d->Cout > 16 && d->Cout <= 64 ? kTileQ : conv_tile_for(d->Cout));
    conv_tile_dims(pl.tile, &pl.BM, &pl.BN);
    k.Hin = d->H;
    k.Win = d->W;
    k.Cin_s = x_cs;
    k.Cout = d->Cout;
    k.act = d->act;
    k.act_scale = d->act_scale;
    k.ntiles = (d->Cout + pl.BN - 1) / pl.BN;
    pl.Cout_p = round_up(d->Cout, 128);
    int Hm, Wm;
    if (!d->transposed) {
        T2V_REQUIRE(d->kH * d->kW <= kMaxTaps, "conv: kernel %dx%d too large", d->kH, d->kW);
        T2V_REQUIRE(d->stride >= 1 && d->pad >= 0, "conv: bad stride/pad");
        pl.Hout = (d->H + 2 * d->pad - d->kH) / d->stride + 1;
        pl.Wout = (d->W + 2 * d->pad - d->kW) / d->stride + 1;
        T2V_REQUIRE(pl.Hout > 0 && pl.Wout > 0, "conv: empty output");
        if (d->pad_mode == T2V_PAD_REFLECT)
            T2V_REQUIRE(d->pad < d->H && d->pad < d->W, "reflection pad %d needs H,W > pad (H=%d W=%d)", d->pad, d->H,
                        d->W);
        Hm = pl.Hout;
        Wm = pl.Wout;
        k.stride = d->stride;
        k.ostride = 1;
        k.pad_mode = d->pad_mode;
        k.nphases = 1;
        k.KW = d->kW;
        k.pad = d->pad;
        ConvPhase& ph = k.ph[0];
        ph.ntaps = d->kH * d->kW;
        ph.tap0 = 0;
        ph.Kp = round_up(ph.ntaps * x_cs, kBK);
        ph.nk = ph.Kp / kBK;
        ph.w_off = 0;
        ph.oy0 = ph.ox0 = 0;
        for (int kh = 0; kh < d->kH; ++kh)
            for (int kw = 0; kw < d->kW; ++kw) {
                k.tdy[kh * d->kW + kw] = kh - d->pad;
                k.tdx[kh * d->kW + kw] = kw - d->pad;
            }
        pl.wfloats = (size_t)pl.Cout_p * ph.Kp;
    } else {
        T2V_REQUIRE(d->kH == d->kW && (d->kH == 3 || d->kH == 4) && d->stride == 2 && d->pad >= 0 && d->pad <= 2 &&
                        d->output_padding >= 0 && d->output_padding <= 1,
                    "transposed conv: k in {3,4}, stride 2, padding <= 2, output_padding <= 1 are on the path");
        pl.Hout = (d->H - 1) * 2 - 2 * d->pad + d->kH + d->output_padding;
        pl.Wout = (d->W - 1) * 2 - 2 * d->pad + d->kW + d->output_padding;
        T2V_REQUIRE(pl.Hout > 0 && pl.Wout > 0, "transposed conv: empty output");
        T2V_REQUIRE(!need_stats || (pl.Hout % 2 == 0 && pl.Wout % 2 == 0),
                    "transposed conv with fused norm statistics needs an even output (got %dx%d)", pl.Hout, pl.Wout);
        Hm = (pl.Hout + 1) / 2;   // phase grid; odd outputs: the odd phase's last row/col is masked at the store
        Wm = (pl.Wout + 1) / 2;
        k.stride = 1;
        k.ostride = 2;
        k.pad_mode = T2V_PAD_ZERO;
        k.nphases = 4;
        k.KW = 3;
        k.pad = 0;
        int tap0 = 0;
        long woff = 0;
        for (int p = 0; p < 4; ++p) {
            int nt, kh[4], kw[4], dy[4], dx[4], a, b;
            convT_phase_taps_host(p, d->kH, d->pad, &nt, kh, kw, dy, dx, &a, &b);
            ConvPhase& ph = k.ph[p];
            ph.ntaps = nt;
            ph.tap0 = tap0;
            ph.Kp = round_up(nt * x_cs, kBK);
            ph.nk = ph.Kp / kBK;
            ph.w_off = woff;
            ph.oy0 = a;
            ph.ox0 = b;
            for (int t = 0; t < nt; ++t) {
                k.tdy[tap0 + t] = dy[t];
                k.tdx[tap0 + t] = dx[t];
            }
            tap0 += nt;
            woff += (long)pl.Cout_p * ph.Kp;
        }
        pl.wfloats = (size_t)woff;
    }
    k.group_mtiles = 1 << 30;
    k.group_w_stride = 0;
    k.Wm = Wm;
    k.M = Hm * Wm;
    k.Wout = pl.Wout;
    k.Hout = pl.Hout;
    k.mtiles = (k.M + pl.BM - 1) / pl.BM;
    if (pl.tile == kTileL) {
        // tile quantisation: with 128x128 tiles a grid that fills the last wave of 256 CUs poorly
        // (e.g. 160 or 344 tiles at the real fadg0 geometries 512x320 / 512x680) idles a third of
        // the chip; 64x64 tiles (several co-resident blocks per CU) even that out
        const long nb = (long)k.mtiles * k.ntiles * k.nphases;
        const double fill = (double)nb / (double)(((nb + 255) / 256) * 256);
        // transposed convs with few blocks: the four phases have 1/2/2/4 taps, and one 128x128 block per CU cannot
        // balance such unequal blocks (1024->512 up-sampling: 0.317 -> 0.286 ms with 64x64 tiles)
        // ... or when four times as many 64x64 blocks fill the chip's rounds clearly better (864 tiles of the 64x85
        // Winograd GEMM: 0.84 -> 0.96, 0.259 -> 0.244 ms)
        const long nbq = 4 * nb;
        const double fillq = (double)nbq / (double)(((nbq + 255) / 256) * 256);
        // (rule against forced tiles, per layer, at 512x320 / 512x680 / 512x512: within 1.3 / 2.8 / 1.0 % of the best forced
        // choice -- profiles/r04_ab_s2_tiles.txt; the forcing switch is gone)
        // (T2V_ALGO_DIRECT_BF16X2 has the one 128x128 form: conv_igemm_split.hip)
        const int force = is_direct_split(d->algo) ? 1 : options().conv_tile;
        if (force == 2 || (force != 1 && ((fill < 0.8 && nb < 1024) || (k.nphases > 1 && nb <= 512) || (fillq - fill >= 0.1 && nb < 2048)))) {
            pl.tile = kTileQ;
            conv_tile_dims(pl.tile, &pl.BM, &pl.BN);
            k.ntiles = (d->Cout + pl.BN - 1) / pl.BN;
            k.mtiles = (k.M + pl.BM - 1) / pl.BM;
        }
    }
    if (need_stats && !d->transposed && d->kH == 7 && d->kW == 7 && d->stride == 1 && d->pad == 3 &&
        d->pad_mode == T2V_PAD_REFLECT && d->act == T2V_ACT_NONE && conv_stem7x7_supported(d->H, d->W, x_cs, d->Cout)) {
        // the 7x7 stems: halo-in-LDS MFMA kernel (conv_stem.hip); statistics per 16x16 pixel tile
        pl.tile = kTileStem;
        pl.BM = 256;
        pl.BN = d->Cout;
        k.mtiles = ((d->H + 15) / 16) * ((d->W + 15) / 16);
        k.ntiles = 1;
    }
    pl.nparts = k.nphases * k.mtiles;
    T2V_REQUIRE((long)k.mtiles * k.ntiles * k.nphases < (1L << 31), "conv: grid too large");
    // buffer addressing: 32-bit byte offsets below the out-of-range marker 0x7fff0000
    T2V_REQUIRE((long)d->H * d->W * x_cs * 4 < 0x7fff0000L, "conv: input tensor too large for 32-bit buffer offsets");
    for (int ph = 0; ph < k.nphases; ++ph)
        T2V_REQUIRE((long)pl.Cout_p * k.ph[ph].Kp * 4 < 0x7fff0000L, "conv: weight too large for 32-bit buffer offsets");
    return T2V_OK;
}

bool winograd_supported(const t2v_conv_desc* d, int x_cs, int algo) {
    if (!d || !is_winograd(algo)) return false;
    if (d->transposed || d->kH != 3 || d->kW != 3 || d->stride != 1) return false;
    // ReflectionPad2d(1) (forward ResnetBlock conv) or zero padding 0..2 (pad 2: that conv's data gradient)
    if (d->pad_mode == T2V_PAD_REFLECT ? d->pad != 1 : (d->pad < 0 || d->pad > 2)) return false;
    if (wino_out_h(d) < 1 || wino_out_w(d) < 1) return false;
    // any H, W >= 2 (reflection needs 2): ragged tiles are masked, the tile count is padded to 128
    if (d->Cin % 32 != 0 || x_cs != d->Cin || d->Cout % 4 != 0 || d->H < 2 || d->W < 2) return false;
    // the split-bf16 GEMM works on whole 128-wide N tiles (Cin % 32 == 0, its K stage, is asked of every form above)
    if (is_split(algo) && d->Cout % 128 != 0) return false;
    // the F(4x4) output transform can apply a (Leaky)ReLU (convs without a norm: the VGG19 loss network)
    return d->act == T2V_ACT_NONE || (is_f4(algo) && d->act == T2V_ACT_LRELU);
}
// Training is fp32: every backward, weight-gradient and data-gradient entry turns a split-bf16 descriptor away by name
static bool refuses_split(const t2v_conv_desc* d, const char* entry) {
    if (d && is_direct_split(d->algo)) {
        set_error("%s: T2V_ALGO_DIRECT_BF16X2 (algo 6) is a forward-only form; gradients run in fp32 (algo %d)", entry,
                  T2V_ALGO_DIRECT);
        return true;
    }
    if (d && is_poly_split(d->algo)) {
        set_error("%s: T2V_ALGO_POLYPHASE_BF16X2 (algo 5) is a forward-only form; gradients run in fp32 (algo %d)", entry,
                  T2V_ALGO_POLYPHASE);
        return true;
    }
    if (!d || !is_split(d->algo)) return false;
    set_error("%s: T2V_ALGO_WINOGRAD_F4_BF16X2 (algo 4) is a forward-only form; gradients run in fp32 (algo %d)", entry,
              T2V_ALGO_WINOGRAD_F4);
    return true;
}
#define T2V_REFUSE_SPLIT(d, entry)                       \
    do {                                                 \
        if (refuses_split(d, entry)) return T2V_ERR_INVALID; \
    } while (0)

// F(4x4) unless the zero tiles that pad its coarser grid to 128 make F(2x2) the smaller GEMM (tiny maps); direct
// when neither beats 9 rows per output pixel
int best_conv_algo(const t2v_conv_desc* d, int x_cs, int cap) {
    const bool f4 = cap == 0 && winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD_F4);
    const bool f2 = (cap == 0 || cap == 2) && winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD);
    const long direct_rows = 9L * wino_out_h(d) * wino_out_w(d);
    if (f4 && (!f2 || wino_gemm_rows(d, T2V_ALGO_WINOGRAD_F4) <= wino_gemm_rows(d, T2V_ALGO_WINOGRAD)) &&
        wino_gemm_rows(d, T2V_ALGO_WINOGRAD_F4) < direct_rows)
        return T2V_ALGO_WINOGRAD_F4;
    if (f2 && wino_gemm_rows(d, T2V_ALGO_WINOGRAD) < direct_rows) return T2V_ALGO_WINOGRAD;
    return T2V_ALGO_DIRECT;
}

// ---- the batched per-position GEMM of the Winograd and polyphase paths: C[g] = A[g] B[g]^T for `groups` transform positions,
// A[g] [T][K] (tile rows, the first `rows` of them real), B[g] [N][K], C[g] [T][N].  One place decides which kernel form
// runs it (position_gemm_form: also what t2v_conv_winograd_gemm_form reports) and one place launches it (run_position_gemm).
// The struct is data about the GEMM only; the callers differ in nothing else.
struct PositionGemm {
    int groups = 0;             // transform positions: 16 | 36 | 81
    int rows = 0;               // real tile rows per position; 0: not known (only the whole-tile forms are considered)
    int T = 0, K = 0, N = 0;    // padded tile rows per position, reduction length, output channels (= C's channel pitch)
    int a_pitch = 0;            // tile rows between the positions of A where A is a window of a wider matrix (a kept V, the
                                // weight gradient's batch-wide A dy A^T); 0: T
    bool has_scratch = true;    // the workspace ends in the fixed-grid forms' hand-over scratch (wino_gemm_sk_scratch_floats());
                                // false (F(2x2)): one block per tile
    bool b_kn = false;          // B is [groups][K][N]: the caller has checked wino_gemm_sk_bkn_ok, the whole-tile fixed grid runs
};

// the one-block-per-tile form as a plan of the implicit-GEMM kernel: a 1x1 conv over a `groups` x T image
static int build_position_gemm_plan(const PositionGemm& g, ConvPlan* pl) {
    t2v_conv_desc d;
    memset(&d, 0, sizeof(d));
    d.H = g.groups; d.W = g.T; d.Cin = g.K; d.Cout = g.N; d.kH = d.kW = 1; d.stride = 1; d.pad = 0;
    d.pad_mode = T2V_PAD_ZERO; d.act = T2V_ACT_NONE; d.act_scale = 1.f;
    T2V_TRY(build_conv_plan(&d, g.K, /*need_stats: 128- or 64-row tiles only*/ true, pl));
    // A batch (nimg >= 2: T = 512, 1024, ... rows per position) keeps the 128x128 tiles build_conv_plan's fill rule
    // leaves it with: alone the 64x64 tiles are faster at T = 512 (315 vs 335 us per batch-2 launch), inside two-stream
    // frames they lose (11.80 vs 11.41 ms per frame) -- the big tiles leave wave slots to the other stream's kernels.
    if (g.T % pl->BM != 0 && pl->tile == kTileL) {   // tile count padded to 64 only: the 64x64 tile config
        pl->tile = kTileQ;
        conv_tile_dims(pl->tile, &pl->BM, &pl->BN);
        pl->kp.ntiles = (d.Cout + pl->BN - 1) / pl->BN;
        pl->kp.mtiles = (pl->kp.M + pl->BM - 1) / pl->BM;
        pl->nparts = pl->kp.nphases * pl->kp.mtiles;
    }
    T2V_REQUIRE(g.T % pl->BM == 0, "position gemm: tile rows %d do not divide %d", pl->BM, g.T);
    pl->kp.group_mtiles = g.T / pl->BM;
    pl->kp.group_w_stride = (long)pl->Cout_p * g.K;
    if (g.a_pitch) {   // the [groups][T] "image" of the 1x1 plan is a window of a wider one: input row pitch a_pitch
        T2V_REQUIRE((long)g.groups * g.a_pitch * g.K * 4 < 0x7fff0000L, "position gemm: A too large for 32-bit buffer offsets");
        pl->kp.Win = g.a_pitch;
    }
    return T2V_OK;
}

// Which form runs (T2V_GEMM_*; -1: none, the error is set): tall-ragged -> ragged -> whole-tile fixed grid -> one block per
// tile.  plan (optional) receives the one-block-per-tile plan when that is the answer.
static int position_gemm_form(const PositionGemm& g, ConvPlan* plan = nullptr) {
    if (g.b_kn) return T2V_GEMM_FIXED_GRID_128x128;
    if (g.has_scratch) {
        if (wino_gemm_skt_ok(g.groups, g.rows, g.T, g.K, g.N, g.N)) return T2V_GEMM_FIXED_GRID_RAGGED_TALL;
        if (wino_gemm_skr_ok(g.groups, g.rows, g.T, g.K, g.N, g.N)) return T2V_GEMM_FIXED_GRID_RAGGED;
        if (wino_gemm_sk_ok(g.groups, g.T, g.K, g.N, g.N, g.rows))
            switch (wino_gemm_sk_tall_rows(g.groups, g.rows, g.T, g.N)) {
                case 160: return T2V_GEMM_FIXED_GRID_160x128;
                case 256: return T2V_GEMM_FIXED_GRID_256x128;
                default: return g.T % 128 == 0 ? T2V_GEMM_FIXED_GRID_128x128 : T2V_GEMM_FIXED_GRID_192x64;
            }
    }
    ConvPlan local;
    ConvPlan* pl = plan ? plan : &local;
    if (build_position_gemm_plan(g, pl) != T2V_OK) return -1;
    return pl->tile == kTileL ? T2V_GEMM_TILE_PER_BLOCK_128x128 : T2V_GEMM_TILE_PER_BLOCK_64x64;
}

static int run_position_gemm(t2v_ctx* ctx, hipStream_t s, const PositionGemm& g, const float* a, const float* b, float* c,
                             float* scratch) {
    T2V_REQUIRE(a && b && c && (scratch || !g.has_scratch), "position gemm: null pointer");
    ConvPlan pl;
    const int form = position_gemm_form(g, &pl);
    if (form < 0) return T2V_ERR_INVALID;
    if (form == T2V_GEMM_TILE_PER_BLOCK_128x128 || form == T2V_GEMM_TILE_PER_BLOCK_64x64)
        return run_conv(ctx, s, pl, a, b, nullptr, c, g.N, nullptr);
    SkGemm k;
    k.a = a; k.b = b; k.c = c; k.scratch = scratch;
    k.err = async_error_word();
    k.rows = g.rows;
    k.a_group_stride = (long)(g.a_pitch ? g.a_pitch : g.T) * g.K;
    k.groups = g.groups; k.T = g.T; k.K = g.K; k.N = g.N; k.c_cs = g.N;
    k.b_kn = g.b_kn;
    if (form == T2V_GEMM_FIXED_GRID_RAGGED_TALL) return launch_wino_gemm_skt(s, k, g.rows);
    if (form == T2V_GEMM_FIXED_GRID_RAGGED) return launch_wino_gemm_skr(s, k, g.rows);
    return launch_wino_gemm_sk(s, k);
}

bool conv_plan_is_head7x7(const ConvPlan& pl) {
    const ConvKParams& q = pl.kp;
    return q.nphases == 1 && q.ph[0].ntaps == 49 && q.KW == 7 && q.pad == 3 && q.stride == 1 && q.pad_mode == T2V_PAD_REFLECT &&
           q.Cout <= 3 && q.Cin_s % 16 == 0 && q.Hin >= 4 && q.Win >= 4;
}
int run_head7x7(hipStream_t s, const ConvPlan& pl, const float* x, const float* w, const float* bias, float* y, int y_cs,
                const LazyNorm* lazy) {
    const ConvKParams& q = pl.kp;
    T2V_REQUIRE(conv_plan_is_head7x7(pl), "head7x7: not a 7x7 reflect-padded conv with <= 3 output channels");
    T2V_REQUIRE(!lazy || (lazy->mean_rstd && (lazy->gamma == nullptr) == (lazy->beta == nullptr) && !lazy->res && !lazy->xout),
                "head7x7: a pending norm is (mean, rstd), gamma and beta or neither, no residual");
    HeadParams h;
    h.x = x; h.w = w; h.bias = bias; h.y = y;
    h.H = q.Hin; h.W = q.Win; h.Cin_s = q.Cin_s; h.Kp = q.ph[0].Kp; h.Cout = q.Cout; h.Cout_s = y_cs;
    h.act = q.act; h.act_scale = q.act_scale;
    if (lazy) {
        h.mean_rstd = lazy->mean_rstd; h.gamma = lazy->gamma; h.beta = lazy->beta; h.relu = lazy->relu;
    }
    return launch_conv_head7x7(s, h);
}

// `batch` images in one go (image b at x + b * x_stride, y + b * y_stride, statistics at stats + b * stats_stride, floats):
// the implicit-GEMM kernel takes them as blockIdx.y of ONE launch -- the discriminators' layers of the train step are 67-552
// blocks per image, a fraction of the 1024+ block slots of the chip; the dedicated stem / head / one-channel kernels are
// launched image by image.
int run_conv_batch(t2v_ctx* ctx, hipStream_t s, const ConvPlan& pl, int batch, const float* x, long x_stride, const float* w,
                   const float* bias, float* y, int y_cs, long y_stride, float* stats, long stats_stride) {
    T2V_REQUIRE(ctx && x && w && y, "conv: null pointer");
    T2V_REQUIRE(batch >= 1 && batch <= 65535, "conv: batch %d", batch);
    T2V_REQUIRE(y_cs >= pl.kp.Cout && y_cs <= pl.Cout_p, "conv: output channel storage %d out of range [%d,%d]", y_cs,
                pl.kp.Cout, pl.Cout_p);
    T2V_REQUIRE((long)pl.Hout * pl.Wout * y_cs * 4 < 0x7fff0000L, "conv: output tensor too large for 32-bit buffer offsets");
    if (!stats && conv_plan_is_head7x7(pl)) {      // the generator heads: dedicated halo-tile kernel (conv_head.hip)
        for (int b = 0; b < batch; ++b) T2V_TRY(run_head7x7(s, pl, x + b * x_stride, w, bias, y + b * y_stride, y_cs, nullptr));
        return T2V_OK;
    }
    {
        // one output channel, long K (the discriminators' last layer): a wave per output pixel (conv_head.hip)
        const ConvKParams& q = pl.kp;
        if (!stats && q.nphases == 1 && q.Cout == 1 && q.pad_mode == T2V_PAD_ZERO && q.ostride == 1 &&
            q.ph[0].ntaps == q.KW * q.KW && conv_cout1_supported(q.KW, q.Cin_s) &&
            (q.act == T2V_ACT_NONE || q.act == T2V_ACT_LRELU)) {
            for (int b = 0; b < batch; ++b) {
                Cout1Params c;
                c.x = x + b * x_stride; c.w = w; c.bias = bias; c.y = y + b * y_stride;
                c.H = q.Hin; c.W = q.Win; c.Cin_s = q.Cin_s; c.ksize = q.KW; c.stride = q.stride; c.pad = q.pad;
                c.Hout = pl.Hout; c.Wout = pl.Wout; c.Cout_s = y_cs; c.act = q.act; c.act_scale = q.act_scale;
                T2V_TRY(launch_conv_cout1(s, c));
            }
            return T2V_OK;
        }
    }
    if (pl.tile == kTileStem && stats) {
        for (int b = 0; b < batch; ++b) {
            StemParams sp;
            sp.x = x + b * x_stride; sp.w = w; sp.bias = bias; sp.y = y + b * y_stride; sp.stats = stats + b * stats_stride;
            sp.H = pl.kp.Hin; sp.W = pl.kp.Win; sp.Cin_s = pl.kp.Cin_s; sp.Kp = pl.kp.ph[0].Kp; sp.Cout = pl.kp.Cout; sp.Cout_s = y_cs;
            sp.Cin = pl.Cin;
            T2V_TRY(launch_conv_stem7x7(s, sp));
        }
        return T2V_OK;
    }
    T2V_REQUIRE(pl.tile != kTileStem, "conv: the stem plan needs a statistics buffer");
    ConvKParams k = pl.kp;
    k.x = x;
    k.w = w;
    k.bias = bias;
    k.y = y;
    k.Cout_s = y_cs;
    k.stats = stats;
    k.batch = batch;
    k.x_img_stride = batch > 1 ? x_stride : 0;
    k.y_img_stride = batch > 1 ? y_stride : 0;
    k.stats_img_stride = (batch > 1 && stats) ? stats_stride : 0;
    return launch_conv_igemm(s, k, pl.tile);
}

int run_conv(t2v_ctx* ctx, hipStream_t s, const ConvPlan& pl, const float* x, const float* w, const float* bias,
             float* y, int y_cs, float* stats) {
    return run_conv_batch(ctx, s, pl, 1, x, 0, w, bias, y, y_cs, 0, stats, 0);
}

// all of a Winograd conv (shared with the generator orchestrator): stages bit 1 = input transform,
// 2 = batched GEMM, 4 = output transform
int winograd_forward(t2v_ctx* ctx, hipStream_t s, const t2v_conv_desc* d, const float* x, const float* w_packed,
                     const float* bias, float* y, float* stats_partial, float* workspace, int stages,
                     const WinoBatch* batch) {
    const WinoBatch one;
    const WinoBatch& wb = batch ? *batch : one;
    const int nimg = wb.nimg;
    const bool f4 = is_f4(d->algo), split = is_split(d->algo);
    if (f4) T2V_TRY(check_async_errors());
    T2V_REQUIRE(nimg >= 1 && (f4 || nimg == 1), "winograd: batches are F(4x4,3x3) only");
    const size_t T = (size_t)wino_rows_batch(d, d->algo, nimg);
    const bool keep = wb.keep_v != nullptr;
    T2V_REQUIRE(!keep || (f4 && !split && nimg == 1 && wb.keep_slot >= 0 && wb.keep_slot < wb.keep_total),
                "winograd: V is kept for the weight gradient of single F(4x4,3x3) images only");
    T2V_REQUIRE(!wb.v_in || (f4 && !keep && !(stages & 1)), "winograd: a borrowed V replaces the input transform (F(4x4,3x3))");
    T2V_REQUIRE(!wb.lazy || (f4 && !keep), "winograd: the input transform applies a pending norm for F(4x4,3x3) into the call's own V");
    float* V = keep ? wb.keep_v + (size_t)wb.keep_slot * T * d->Cin : workspace;
    float* Mm = workspace + wino_pos(d->algo) * T * d->Cin;
    if (stages & 1) {
        const int reflect = d->pad_mode == T2V_PAD_REFLECT;
        if (keep) T2V_TRY(launch_winograd4_input(s, x, wb.keep_v, d->H, d->W, d->Cin, d->pad, reflect, wb.keep_total, wb.keep_slot));
        else
        T2V_TRY(f4 ? launch_winograd4_input(s, x, V, d->H, d->W, d->Cin, d->pad, reflect, nimg, 0, nimg, wb.img_stride_x, wb.lazy, split)
                   : launch_winograd_input(s, x, V, d->H, d->W, d->Cin, d->pad, reflect));
    }
    if ((stages & 2) && split) {   // V and w_packed hold bf16 plane pairs: one form, one block per tile (winograd_split.hip)
        T2V_TRY(launch_wino_split_gemm(s, 36, wb.v_in ? wb.v_in : V, w_packed, Mm, (int)T, d->Cin, d->Cout));
    } else if (stages & 2) {
        PositionGemm g;
        g.has_scratch = f4;      // (F(2x2)'s workspace has none: winograd_workspace_floats)
        g.groups = wino_pos(d->algo);
        g.rows = nimg * wino_tiles_real(d, d->algo);      // real tile rows per position (the rest of T is padding)
        g.T = (int)T; g.K = d->Cin; g.N = d->Cout;
        // (kept: slot keep_slot of [36][keep_total * Tp][Cin]; the positions are keep_total * Tp rows apart)
        if (keep) g.a_pitch = wb.keep_total * (int)T;
        T2V_TRY(run_position_gemm(ctx, s, g, wb.v_in ? wb.v_in : V, w_packed, Mm, f4 ? workspace + winograd_vm_floats(d, nimg) : nullptr));
    }
    if (stages & 4) {
        T2V_REQUIRE(d->act == T2V_ACT_NONE || !stats_partial, "winograd: an activation and norm statistics do not combine");
        if (f4)
            T2V_TRY(launch_winograd4_output(s, Mm, bias, y, stats_partial, wino_out_h(d), wino_out_w(d), d->Cout,
                                            d->act == T2V_ACT_LRELU, d->act_scale, nimg));
        else
            T2V_TRY(launch_winograd_output(s, Mm, bias, y, stats_partial, wino_out_h(d), wino_out_w(d), d->Cout));
    }
    return T2V_OK;
}

bool polyphase_supported(const t2v_conv_desc* d, int x_cs) {
    if (!d || d->kH != 3 || d->kW != 3 || d->stride != 2 || d->pad != 1 || d->pad_mode != T2V_PAD_ZERO) return false;
    if (d->act != T2V_ACT_NONE || d->Cin % 32 != 0 || x_cs != d->Cin || d->Cout % 128 != 0) return false;
    // any map: the tile grid is ragged at the bottom / right edge (outputs masked, inputs past the map read as the zeros they
    // are) and padded with empty tiles to the GEMM's row granule; a down conv's input must be even-sized
    if (d->transposed) return d->output_padding == 1 && d->H >= 2 && d->W >= 2;
    return d->H >= 4 && d->W >= 4 && d->H % 2 == 0 && d->W % 2 == 0;
}

// where it measured faster than the implicit-GEMM kernel (scripts/poly_check.py, MI355X): both channel counts >= 256 -- the
// transforms move 81/64 + 81/16 of a layer's input + output, against a GEMM of 0.5625x the direct FLOPs -- and enough tiles to
// fill the fixed grid.  512->1024 @128x128 301 -> 229 us, 1024->512 (transposed) @64x64 325 -> 214, 256->512 @256x256 272 ->
// 245, 512->256 (transposed) @128x128 303 -> 248; 128->256 @512x512 284 -> 362 (no)
bool polyphase_pays(const t2v_conv_desc* d, int x_cs) {
    return polyphase_supported(d, x_cs) && d->Cin >= 256 && d->Cout >= 256 && poly_tiles_real(d) >= 128;
}
// the split-bf16 form: the same layers where the 81-position GEMM takes the shape (Cin % 32 and Cout % 128 are asked above)
bool polyphase_split_supported(const t2v_conv_desc* d, int x_cs) {
    return polyphase_supported(d, x_cs) && wino_split_gemm_ok(81, poly_tiles_padded(d), d->Cin, d->Cout);
}

// the form d->algo names (T2V_ALGO_POLYPHASE | T2V_ALGO_POLYPHASE_BF16X2) takes the layer
static bool poly_form_supported(const t2v_conv_desc* d, int x_cs) {
    return is_poly_split(d->algo) ? polyphase_split_supported(d, x_cs) : polyphase_supported(d, x_cs);
}

// ---- T2V_ALGO_DIRECT_BF16X2 (conv_igemm_split.hip): the 3x3 stride-2 conv (even map) and the transposed conv
// (output_padding 1) with zero padding 1 and no activation, whole 32-deep K stages per tap and whole 128-wide N tiles, every
// operand and the output below the out-of-range marker of the 32-bit buffer offsets
bool direct_split_supported(const t2v_conv_desc* d, int x_cs) {
    if (!d || d->kH != 3 || d->kW != 3 || d->stride != 2 || d->pad != 1 || d->pad_mode != T2V_PAD_ZERO || d->act != T2V_ACT_NONE)
        return false;
    if (x_cs != d->Cin || d->Cin < 32 || d->Cin % 32 != 0 || d->Cout < 128 || d->Cout % 128 != 0 || d->H < 1 || d->W < 1) return false;
    if (d->transposed ? d->output_padding != 1 : (d->H % 2 != 0 || d->W % 2 != 0)) return false;
    const long out_px = d->transposed ? 4L * d->H * d->W : (long)(d->H / 2) * (d->W / 2);
    // (the largest weight block a phase addresses: 9 taps, 4 for a transposed conv)
    return (long)d->H * d->W * d->Cin * 4 < 0x7fff0000L && (long)d->Cout * (d->transposed ? 4 : 9) * d->Cin * 4 < 0x7fff0000L &&
           out_px * d->Cout * 4 < 0x7fff0000L;
}
int check_split_library() {
    const int got = t2v_split_interface();
    T2V_REQUIRE(got == kSplitInterface, "libt2v_split.so speaks interface 0x%x, libt2v_hip.so 0x%x: the two libraries are not of one build",
                got, kSplitInterface);
    return T2V_OK;
}
// n floats (n % 4 == 0) into the pair layout; y == x: in place
int launch_split_pairs(hipStream_t s, const float* x, float* y, long n) {
    T2V_TRY(check_split_library());
    T2V_REQUIRE(n > 0 && n % 4 == 0, "split pass: %ld floats (a positive multiple of 4)", n);
    T2V_HIP_CHECK((hipError_t)t2v_split_launch_pairs(s, x, y, n / 4, capped_grid(n / 4, 256, 4096)));
    return T2V_OK;
}
// p: a kTileL plan of a supported layer (direct_split_supported), x and w in the pair layout
int launch_conv_igemm_split(hipStream_t s, const ConvKParams& p) {
    T2V_REQUIRE(p.Cin_s % kBK == 0 && p.Cout % 128 == 0 && p.Cout_s == p.Cout && p.pad_mode == T2V_PAD_ZERO &&
                    p.act == T2V_ACT_NONE && p.batch <= 1 && p.mtiles == (p.M + 127) / 128 && p.ntiles == p.Cout / 128,
                "split-bf16 direct conv: plan outside the form (Cin %% 32, Cout %% 128, zero padding, no activation, 128x128 tiles)");
    T2V_TRY(check_split_library());
    T2V_HIP_CHECK((hipError_t)t2v_split_launch_conv(s, &p));
    return T2V_OK;
}
int direct_split_forward(hipStream_t s, const t2v_conv_desc* d, const float* x_pairs, const float* w_packed, const float* bias,
                         float* y, float* stats_partial) {
    T2V_REQUIRE(d && is_direct_split(d->algo) && direct_split_supported(d, d->Cin),
                "split-bf16 direct forward: shape not supported (t2v_conv_direct_bf16x2_supported)");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, d->Cin, stats_partial != nullptr, &pl));
    T2V_REQUIRE(pl.tile == kTileL, "internal: the split-bf16 direct conv plans 128x128 tiles");
    ConvKParams k = pl.kp;
    k.x = x_pairs; k.w = w_packed; k.bias = bias; k.y = y; k.Cout_s = d->Cout; k.stats = stats_partial;
    k.batch = 1;
    return launch_conv_igemm_split(s, k);
}

// stages bit 1 = input transform, 2 = the 81 batched GEMMs, 4 = output transform (bias, statistics partials)
int polyphase_forward(t2v_ctx* ctx, hipStream_t s, const t2v_conv_desc* d, const float* x, const float* w_packed,
                      const float* bias, float* y, float* stats_partial, float* workspace, int stages,
                      const LazyNorm* lazy) {
    T2V_TRY(check_async_errors());
    const int up = d->transposed ? 1 : 0;
    const int T = poly_tiles_padded(d), rows = poly_tiles_real(d);
    float* V = workspace;
    float* Mm = workspace + (size_t)81 * T * d->Cin;
    const bool split = is_poly_split(d->algo);
    if (stages & 1) T2V_TRY(launch_polyphase_input(s, x, V, d->H, d->W, d->Cin, up, T, lazy, split));
    if ((stages & 2) && split) {   // V and w_packed hold bf16 plane pairs (polyphase_split.hip); the scratch is left alone
        T2V_TRY(launch_wino_split_gemm(s, 81, V, w_packed, Mm, T, d->Cin, d->Cout));
    } else if (stages & 2) {
        PositionGemm g;
        g.groups = 81; g.rows = rows; g.T = T; g.K = d->Cin; g.N = d->Cout;
        T2V_TRY(run_position_gemm(ctx, s, g, V, w_packed, Mm, workspace + (size_t)81 * T * ((size_t)d->Cin + d->Cout)));
    }
    if (stages & 4)
        T2V_TRY(launch_polyphase_output(s, Mm, bias, y, stats_partial, poly_out_h(d), poly_out_w(d), d->Cout, up, T));
    return T2V_OK;
}

size_t norm_partial_floats(const t2v_conv_desc* d, int x_cs) {
    if (!d) return 0;
    if (is_winograd(d->algo))   // one partial per 128 output-pixel slots of the padded tile grid
        return (size_t)(wino_tiles_padded(d, d->algo) * wino_m(d->algo) * wino_m(d->algo) / 128) * d->Cout * 2;
    if (is_poly(d->algo)) return (size_t)(poly_tiles_padded(d) * poly_m(d) * poly_m(d) / 128) * d->Cout * 2;
    ConvPlan pl;
    if (build_conv_plan(d, x_cs, true, &pl) != T2V_OK) return 0;
    return (size_t)pl.nparts * d->Cout * 2;
}

int finalize_norm(hipStream_t s, const t2v_conv_desc* producer, int x_cs, const float* stats, int pooled_images, float eps,
                  float* mean_rstd, double* scratch, const RunningUpdate* ru, const ConvPlan* plan) {
    if (producer && is_winograd(producer->algo))   // the output transform emits one partial per 128 pixels
        return launch_inorm_finalize_winograd(s, stats, wino_m(producer->algo), wino_out_h(producer), wino_out_w(producer),
                                              producer->Cout, eps, mean_rstd, pooled_images, scratch, ru);
    if (producer && is_poly(producer->algo))
        return launch_inorm_finalize_winograd(s, stats, poly_m(producer), poly_out_h(producer), poly_out_w(producer),
                                              producer->Cout, eps, mean_rstd, pooled_images, scratch, ru);
    ConvPlan own;
    if (!plan) {
        T2V_TRY(build_conv_plan(producer, x_cs, true, &own));
        plan = &own;
    }
    if (plan->tile == kTileStem)
        return launch_inorm_finalize_tiles(s, stats, 16, producer->H, producer->W, producer->Cout, eps, mean_rstd, pooled_images,
                                           scratch, ru);
    // the per-image partial blocks are contiguous: a batch is just `pooled_images` times more partial rows
    return launch_inorm_finalize(s, stats, pooled_images * plan->nparts, plan->kp.mtiles, plan->BM, plan->kp.M, producer->Cout,
                                 eps, mean_rstd, scratch, ru);
}

}  // namespace t2v

using namespace t2v;

extern "C" {

int t2v_abi_version(void) { return T2V_ABI_VERSION; }
const char* t2v_last_error(void) { return g_err; }

int t2v_create(t2v_ctx** out, int device) {
    T2V_REQUIRE(out, "t2v_create: null out");
    int n = 0;
    T2V_HIP_CHECK(hipGetDeviceCount(&n));
    T2V_REQUIRE(device >= 0 && device < n, "t2v_create: device %d out of range (%d visible)", device, n);
    T2V_HIP_CHECK(hipSetDevice(device));
    hipDeviceProp_t prop;
    T2V_HIP_CHECK(hipGetDeviceProperties(&prop, device));
    T2V_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0,
                "libt2v_hip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
    t2v_ctx* c = new t2v_ctx();
    c->device = device;
    c->side = nullptr;
    c->ev_fork = c->ev_join = nullptr;
    if (hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess) {
        t2v_destroy(c);
        set_error("t2v_create: cannot create the side stream / events");
        return T2V_ERR_HIP;
    }
    (void)options();
    {   // once per process: the sticky error word and the dispatch-order self-test of the fixed-grid kernels
        static std::once_flag once;
        int st = T2V_OK;
        std::call_once(once, [&]() {
            void* w = nullptr;
            if (hipHostMalloc(&w, 64, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
                fixed_grid_disable("no pinned error word");
                return;
            }
            memset(w, 0, 64);
            g_err_word = static_cast<unsigned*>(w);
            st = fixed_grid_selftest();
        });
        if (st != T2V_OK) {
            t2v_destroy(c);
            return st;
        }
    }
    *out = c;
    return T2V_OK;
}

void t2v_reload_env(void) { options_reload(); }
int t2v_set_overlap_hint(int on) { return set_overlap_hint(on); }
int t2v_check_async_errors(void) { return check_async_errors(); }
int t2v_fixed_grid_enabled(void) { return fixed_grid_enabled() ? 1 : 0; }
void t2v_debug_async_error(int raise) {
    if (!g_err_word) return;
    if (raise) {
        *reinterpret_cast<volatile unsigned*>(g_err_word) = 1u;      // what a timed-out consumer wave stores
    } else {
        *reinterpret_cast<volatile unsigned*>(g_err_word) = 0u;
        g_fixed_grid_on.store(1);
    }
}

int t2v_destroy(t2v_ctx* ctx) {
    if (!ctx) return T2V_OK;
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    delete ctx;
    return T2V_OK;
}

int t2v_conv_out_dims(const t2v_conv_desc* d, int* Hout, int* Wout) {
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, round_up(d ? d->Cin : 0, 4), false, &pl));
    if (Hout) *Hout = pl.Hout;
    if (Wout) *Wout = pl.Wout;
    return T2V_OK;
}

size_t t2v_conv_packed_weight_floats(const t2v_conv_desc* d, int x_cs) {
    ConvPlan pl;
    if (build_conv_plan(d, x_cs, false, &pl) != T2V_OK) return 0;
    if (is_winograd(d->algo)) return winograd_supported(d, x_cs, d->algo) ? (size_t)wino_pos(d->algo) * pl.Cout_p * x_cs : 0;
    if (is_poly(d->algo)) return poly_form_supported(d, x_cs) ? (size_t)81 * pl.Cout_p * x_cs : 0;
    if (is_direct_split(d->algo) && !direct_split_supported(d, x_cs)) return 0;      // (the bytes of the fp32 packing)
    return pl.wfloats;
}
int t2v_conv_direct_bf16x2_supported(const t2v_conv_desc* d, int x_cs) { return direct_split_supported(d, x_cs) ? 1 : 0; }
int t2v_conv_polyphase_bf16x2_supported(const t2v_conv_desc* d, int x_cs) { return polyphase_split_supported(d, x_cs) ? 1 : 0; }
int t2v_conv_polyphase_supported(const t2v_conv_desc* d, int x_cs) {
    return (polyphase_supported(d, x_cs) ? 1 : 0) | (polyphase_pays(d, x_cs) ? 2 : 0);
}

int t2v_conv_winograd_supported(const t2v_conv_desc* d, int x_cs) {
    return (winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD) ? 1 : 0) | (winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD_F4) ? 2 : 0);
}
int t2v_conv_winograd_bf16x2_supported(const t2v_conv_desc* d, int x_cs) {
    return winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD_F4_BF16X2) ? 1 : 0;
}

int t2v_conv_best_algo(const t2v_conv_desc* d, int x_cs, int cap) { return d ? best_conv_algo(d, x_cs, cap) : T2V_ALGO_DIRECT; }

size_t t2v_conv_winograd_workspace_floats(const t2v_conv_desc* d, int x_cs) {
    // T2V_ALGO_DIRECT_BF16X2: the input in the pair layout, the bytes of x
    if (d && is_direct_split(d->algo)) return direct_split_supported(d, x_cs) ? (size_t)d->H * d->W * d->Cin : 0;
    if (d && is_poly(d->algo)) return poly_form_supported(d, x_cs) ? polyphase_workspace_floats(d) : 0;
    if (!d || !winograd_supported(d, x_cs, d->algo)) return 0;
    return winograd_workspace_floats(d);
}

size_t t2v_conv_winograd_batch_workspace_floats(const t2v_conv_desc* d, int x_cs, int nimg) {
    if (!d || nimg < 1) return 0;
    if (is_direct_split(d->algo)) return nimg == 1 ? t2v_conv_winograd_workspace_floats(d, x_cs) : 0;
    if (is_poly(d->algo)) return nimg == 1 && poly_form_supported(d, x_cs) ? polyphase_workspace_floats(d) : 0;
    if (!winograd_supported(d, x_cs, d->algo) || (nimg > 1 && !is_f4(d->algo))) return 0;
    return winograd_workspace_floats(d, nimg);
}

// The generator's forms of a Winograd / polyphase conv (generator.hip: wino4_conv_stats, conv_norm_one) with the same launchers
// and nothing of its own: nimg packed images (F(4x4) only) and, with `lazy`, the previous layer's norm applied inside the input
// transform.  Both stage entries end here.
static int winograd_stages(t2v_ctx* ctx, hipStream_t s, const t2v_conv_desc* d, int nimg, const float* x, int x_cs, long img_stride,
                           const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial, float* workspace,
                           int stages, const LazyNorm* lazy) {
    if (is_direct_split(d->algo)) {
        // stages bit 1 = the split pass of x into the workspace, 2 | 4 (either) = the conv with its epilogue
        T2V_REQUIRE(direct_split_supported(d, x_cs), "split-bf16 direct forward: shape not supported (t2v_conv_direct_bf16x2_supported)");
        T2V_REQUIRE(y_cs == d->Cout, "split-bf16 direct forward: output channel storage must equal Cout");
        T2V_REQUIRE(nimg == 1 && !lazy, "split-bf16 direct forward: one image with an applied norm");
        if (stages & 1) T2V_TRY(launch_split_pairs(s, x, workspace, (long)d->H * d->W * d->Cin));
        return (stages & 6) ? direct_split_forward(s, d, workspace, w_packed, bias, y, stats_partial) : T2V_OK;
    }
    if (is_poly(d->algo)) {
        T2V_REQUIRE(poly_form_supported(d, x_cs), "polyphase forward: shape not supported (t2v_conv_polyphase_supported, "
                                                  "t2v_conv_polyphase_bf16x2_supported)");
        T2V_REQUIRE(y_cs == d->Cout, "polyphase forward: output channel storage must equal Cout");
        T2V_REQUIRE(nimg == 1 && !(lazy && (lazy->res || lazy->xout)), "polyphase batch forward: one image, no residual");
        return polyphase_forward(ctx, s, d, x, w_packed, bias, y, stats_partial, workspace, stages, lazy);
    }
    T2V_REQUIRE(winograd_supported(d, x_cs, d->algo), "winograd forward: shape/algo not supported (t2v_conv_winograd_supported)");
    T2V_REQUIRE(y_cs == d->Cout, "winograd forward: output channel storage must equal Cout");
    T2V_REQUIRE(is_f4(d->algo) || (nimg == 1 && !lazy), "winograd batch forward: batches and the lazy norm are F(4x4,3x3) only");
    if (lazy && (stages & 1)) T2V_REQUIRE(lazy->relu == 0 || lazy->relu == 1, "winograd batch forward: relu %d", lazy->relu);
    WinoBatch wb;
    wb.nimg = nimg;
    wb.img_stride_x = img_stride;
    wb.lazy = lazy;
    return winograd_forward(ctx, s, d, x, w_packed, bias, y, stats_partial, workspace, stages, &wb);
}

int t2v_conv2d_forward_winograd_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                       const float* w_packed, const float* bias, float* y, int y_cs,
                                       float* stats_partial, float* workspace, int stages) {
    T2V_REQUIRE(ctx && d && x && w_packed && y && workspace, "winograd forward: null pointer");
    return winograd_stages(ctx, (hipStream_t)stream, d, 1, x, x_cs, 0, w_packed, bias, y, y_cs, stats_partial, workspace, stages,
                           nullptr);
}

int t2v_conv2d_forward_winograd_batch_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int nimg, const float* x,
                                             int x_cs, long img_stride, const float* w_packed, const float* bias, float* y,
                                             int y_cs, float* stats_partial, float* workspace, int stages,
                                             const float* mean_rstd, const float* gamma, const float* beta, int relu,
                                             const float* res, float* xout) {
    T2V_REQUIRE(ctx && d && x && w_packed && y && workspace, "winograd batch forward: null pointer");
    T2V_REQUIRE(stages >= 0 && stages <= 7, "winograd batch forward: stages mask %d", stages);
    T2V_REQUIRE(nimg >= 1 && nimg <= 65535, "winograd batch forward: nimg %d", nimg);
    T2V_REQUIRE(nimg == 1 || img_stride >= (long)d->H * d->W * x_cs, "winograd batch forward: image stride %ld below one map",
                img_stride);
    T2V_REQUIRE(mean_rstd || (!gamma && !beta && !res && !xout && relu == 0),
                "winograd batch forward: gamma, beta, relu, res and xout need mean_rstd");
    const LazyNorm ln{mean_rstd, gamma, beta, relu, res, xout};
    return winograd_stages(ctx, (hipStream_t)stream, d, nimg, x, x_cs, img_stride, w_packed, bias, y, y_cs, stats_partial,
                           workspace, stages, mean_rstd ? &ln : nullptr);
}

static bool wgrad_winograd_ok(const t2v_conv_desc* d, int x_cs, int dy_cs);
int t2v_conv2d_forward_winograd_keep_v(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                       const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial,
                                       float* workspace, float* wgrad_workspace, int batch, int slot) {
    T2V_REQUIRE(ctx && d && x && w_packed && y && workspace && wgrad_workspace, "winograd forward (V kept): null pointer");
    T2V_REFUSE_SPLIT(d, "conv2d_forward_winograd_keep_v");
    T2V_REQUIRE(d->algo == T2V_ALGO_WINOGRAD_F4 && winograd_supported(d, x_cs, d->algo) && x_cs == d->Cin &&
                    wgrad_winograd_ok(d, x_cs, d->Cout),
                "winograd forward (V kept): F(4x4,3x3) layers with a Winograd-domain weight gradient only "
                "(t2v_conv_backward_weight_winograd_supported)");
    T2V_REQUIRE(y_cs == d->Cout, "winograd forward: output channel storage must equal Cout");
    T2V_REQUIRE(batch >= 1 && slot >= 0 && slot < batch, "winograd forward (V kept): slot %d of %d", slot, batch);
    T2V_REQUIRE((long)36 * batch * wino_tiles_padded(d, d->algo) * x_cs * 4 < 0x7fff0000L,
                "winograd forward (V kept): batch-wide V too large for 32-bit buffer offsets");
    WinoBatch wb;
    wb.keep_v = wgrad_workspace;     // V is the first tensor of the weight gradient's workspace
    wb.keep_total = batch;
    wb.keep_slot = slot;
    return winograd_forward(ctx, (hipStream_t)stream, d, x, w_packed, bias, y, stats_partial, workspace, 7, &wb);
}

int t2v_conv2d_forward_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial,
                                float* workspace) {
    return t2v_conv2d_forward_winograd_stages(ctx, stream, d, x, x_cs, w_packed, bias, y, y_cs, stats_partial, workspace, 7);
}

static int pack_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* w_torch_dev,
                       float* packed_dev, int adjoint) {
    T2V_REQUIRE(ctx && w_torch_dev && packed_dev, "pack_weight: null pointer");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, false, &pl));
    hipStream_t s = (hipStream_t)stream;
    if (is_poly(d->algo)) {
        T2V_REQUIRE(poly_form_supported(d, x_cs) && !adjoint, "pack_weight: polyphase form not supported for this shape");
        const bool split = is_poly_split(d->algo);
        T2V_REQUIRE(!split || pl.Cout_p == d->Cout, "pack_weight: the split-bf16 planes have no padding rows");
        return launch_polyphase_weight(s, w_torch_dev, packed_dev, d->Cout, d->Cin, pl.Cout_p, x_cs, d->transposed ? 1 : 0, split);
    }
    if (is_winograd(d->algo)) {
        T2V_REQUIRE(winograd_supported(d, x_cs, d->algo), "pack_weight: Winograd not supported for this shape");
        if (is_split(d->algo)) {   // (Cout % 128 == 0: no padding rows)
            T2V_REFUSE_SPLIT(adjoint ? d : nullptr, "conv_pack_weight_adjoint");
            return launch_winograd4_weight_split(s, w_torch_dev, packed_dev, d->Cout, d->Cin, pl.Cout_p, x_cs);
        }
        return (d->algo == T2V_ALGO_WINOGRAD_F4 ? launch_winograd4_weight : launch_winograd_weight)(
            s, w_torch_dev, packed_dev, d->Cout, d->Cin, pl.Cout_p, x_cs, adjoint);
    }
    if (is_direct_split(d->algo))
        T2V_REQUIRE(direct_split_supported(d, x_cs) && !adjoint, "pack_weight: split-bf16 direct form not supported for this shape");
    if (!d->transposed)
        T2V_TRY(launch_pack_conv_weight(s, w_torch_dev, packed_dev, d->Cout, d->Cin, d->kH, d->kW, x_cs, pl.kp.ph[0].Kp,
                                        pl.Cout_p, adjoint));
    else {
        T2V_REQUIRE(!adjoint, "pack_weight_adjoint: stride-1 convolutions only (a transposed conv's data gradient reuses its weight)");
        T2V_TRY(launch_pack_convT_weight(s, w_torch_dev, packed_dev, d->Cin, d->Cout, x_cs, pl.Cout_p, d->kH, d->pad));
    }
    // T2V_ALGO_DIRECT_BF16X2: the fp32 packing, every K pair replaced in place by its two bf16 terms
    return is_direct_split(d->algo) ? launch_split_pairs(s, packed_dev, packed_dev, (long)pl.wfloats) : T2V_OK;
}
int t2v_conv_pack_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* w_torch_dev,
                         float* packed_dev) {
    return pack_weight(ctx, stream, d, x_cs, w_torch_dev, packed_dev, 0);
}
int t2v_conv_pack_weight_adjoint(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* w_forward_dev,
                                 float* packed_dev) {
    T2V_REFUSE_SPLIT(d, "conv_pack_weight_adjoint");      // (before the shape: a forward-only form is refused by name)
    T2V_REQUIRE(d && !d->transposed && d->stride == 1, "pack_weight_adjoint: `d` must be a stride-1 (data-gradient) conv");
    return pack_weight(ctx, stream, d, x_cs, w_forward_dev, packed_dev, 1);
}

size_t t2v_conv_stats_floats(const t2v_conv_desc* d) { return d ? norm_partial_floats(d, round_up(d->Cin, 4)) : 0; }

int t2v_conv2d_forward(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                       const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial) {
    T2V_REQUIRE(d && d->algo == T2V_ALGO_DIRECT, "conv2d_forward: use t2v_conv2d_forward_winograd for algo=WINOGRAD");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, stats_partial != nullptr, &pl));
    return run_conv(ctx, (hipStream_t)stream, pl, x, w_packed, bias, y, y_cs, stats_partial);
}

int t2v_conv2d_forward_head_norm(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                 const float* w_packed, const float* bias, float* y, int y_cs, const float* mean_rstd,
                                 const float* gamma, const float* beta, int relu) {
    T2V_REQUIRE(ctx && d && x && w_packed && y && mean_rstd, "conv2d_forward_head_norm: null pointer");
    T2V_REQUIRE(d->algo == T2V_ALGO_DIRECT, "conv2d_forward_head_norm: direct convolutions only");
    T2V_REQUIRE(relu == 1, "conv2d_forward_head_norm: the pending norm is norm + ReLU (relu must be 1)");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, false, &pl));
    T2V_REQUIRE(y_cs >= pl.kp.Cout && y_cs <= pl.Cout_p, "conv2d_forward_head_norm: output channel storage %d out of range [%d,%d]",
                y_cs, pl.kp.Cout, pl.Cout_p);
    T2V_REQUIRE((long)pl.kp.Hin * pl.kp.Win * x_cs * 4 < 0x7fff0000L, "conv2d_forward_head_norm: input too large for 32-bit buffer offsets");
    const LazyNorm ln{mean_rstd, gamma, beta, relu};
    return run_head7x7((hipStream_t)stream, pl, x, w_packed, bias, y, y_cs, &ln);
}

int t2v_conv2d_forward_batch(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x, int x_cs,
                             const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial) {
    T2V_REQUIRE(d && d->algo == T2V_ALGO_DIRECT, "conv2d_forward_batch: direct convolutions only");
    T2V_REQUIRE(batch >= 1, "conv2d_forward_batch: batch %d", batch);
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, stats_partial != nullptr, &pl));
    return run_conv_batch(ctx, (hipStream_t)stream, pl, batch, x, (long)d->H * d->W * x_cs, w_packed, bias, y, y_cs,
                          (long)pl.Hout * pl.Wout * y_cs, stats_partial, (long)norm_partial_floats(d, round_up(d->Cin, 4)));
}

int t2v_instance_norm_finalize(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, const float* stats_partial,
                               float eps, float* mean_rstd) {
    T2V_REQUIRE(ctx && stats_partial && mean_rstd, "inorm_finalize: null pointer");
    return finalize_norm((hipStream_t)stream, producer, round_up(producer ? producer->Cin : 0, 4), stats_partial, 1, eps, mean_rstd);
}

int t2v_batch_norm_finalize(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                            const float* stats_partial, float eps, float* mean_rstd) {
    T2V_REQUIRE(ctx && stats_partial && mean_rstd && batch >= 1, "batch_norm_finalize: bad arguments");
    return finalize_norm((hipStream_t)stream, producer, round_up(producer ? producer->Cin : 0, 4), stats_partial, batch, eps, mean_rstd);
}
int t2v_batch_norm_finalize_running(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                                    const float* stats_partial, float eps, float* mean_rstd, float* running_mean,
                                    float* running_var, float momentum, int times) {
    T2V_REQUIRE(ctx && producer && stats_partial && mean_rstd && running_mean && running_var && batch >= 1 && times >= 1,
                "batch_norm_finalize_running: bad arguments");
    int ho = 0, wo = 0;
    T2V_TRY(t2v_conv_out_dims(producer, &ho, &wo));
    const long n = (long)batch * ho * wo;
    T2V_REQUIRE(n >= 2, "batch_norm_finalize_running: the unbiased variance needs at least two values per channel");
    const RunningUpdate ru{running_mean, running_var, (float)n, momentum, times};
    return finalize_norm((hipStream_t)stream, producer, round_up(producer->Cin, 4), stats_partial, batch, eps, mean_rstd, nullptr, &ru);
}
// the same with a scratch buffer, which lets a launch of >= 2048 partials pool them in groups (additive to ABI 22)
size_t t2v_norm_finalize_scratch_doubles(const t2v_conv_desc* producer) {
    return producer ? (size_t)kFinalizeMaxGroups * producer->Cout * 4 : 0;
}
int t2v_batch_norm_finalize_scratch(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                                    const float* stats_partial, float eps, float* mean_rstd, float* running_mean,
                                    float* running_var, float momentum, int times, double* scratch, size_t scratch_doubles) {
    T2V_REQUIRE(ctx && producer && stats_partial && mean_rstd && batch >= 1, "batch_norm_finalize_scratch: bad arguments");
    T2V_REQUIRE((running_mean == nullptr) == (running_var == nullptr),
                "batch_norm_finalize_scratch: running_mean and running_var go together");
    T2V_REQUIRE(scratch == nullptr || scratch_doubles >= t2v_norm_finalize_scratch_doubles(producer),
                "batch_norm_finalize_scratch: scratch of %zu doubles, %zu needed", scratch_doubles,
                t2v_norm_finalize_scratch_doubles(producer));
    const int x_cs = round_up(producer->Cin, 4);
    if (!running_mean) return finalize_norm((hipStream_t)stream, producer, x_cs, stats_partial, batch, eps, mean_rstd, scratch);
    T2V_REQUIRE(times >= 1, "batch_norm_finalize_scratch: times %d", times);
    int ho = 0, wo = 0;
    T2V_TRY(t2v_conv_out_dims(producer, &ho, &wo));
    const long n = (long)batch * ho * wo;
    T2V_REQUIRE(n >= 2, "batch_norm_finalize_scratch: the unbiased variance needs at least two values per channel");
    const RunningUpdate ru{running_mean, running_var, (float)n, momentum, times};
    return finalize_norm((hipStream_t)stream, producer, x_cs, stats_partial, batch, eps, mean_rstd, scratch, &ru);
}

// narrow-input regular convs (7x7 stems: 12 / 8 channels; the discriminators' 4x4 first layers: 8): fold the taps
// into the 128-wide channel side of the block tile
static bool wgrad_fold(const t2v_conv_desc* d, int x_cs) {
    return !d->transposed && x_cs < 64 && d->kH * d->kW > 1;
}

// few output channels (the 7x7 heads: 3 -> dy_cs 4) on a wide input: fold the taps onto the dY side
static bool wgrad_fold_n(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    return !d->transposed && d->stride == 1 && dy_cs <= 16 && x_cs >= 64 && d->kH * d->kW > 1 &&
           d->kH * d->kW <= kMaxTaps;
}
static size_t wgrad_padded_floats(const t2v_conv_desc* d, int x_cs, int batch) {
    return (size_t)batch * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) * x_cs;
}

static int wgrad_splits(const t2v_conv_desc* d, int x_cs, int batch, const ConvPlan& pl) {
    // few (tap, channel-tile) blocks but a long pixel reduction (high-resolution, narrow layers): cut the
    // reduction into ranges; partial gradients are summed in a fixed order afterwards
    int ntaps = 0;
    for (int ph = 0; ph < pl.kp.nphases; ++ph) ntaps += pl.kp.ph[ph].ntaps;
    const long blocks = wgrad_fold(d, x_cs) ? (long)((d->Cout + 127) / 128) * ((ntaps * x_cs + 127) / 128)
                                            : (long)ntaps * ((d->Cout + 127) / 128) * ((x_cs + 127) / 128);
    const long nk = ((long)batch * pl.kp.M + 31) / 32;
    // a launch costs rounds x (stages per block + ~3 stages of prologue / epilogue) stage times, a round being
    // one set of resident blocks: a block count just above a whole number of rounds idles most of the chip for
    // the last one.  Fewest stage times wins, ties to the smaller split (less partial-gradient traffic).
    long smax = nk / 8;              // at least 8 stages per block
    if (smax > 256) smax = 256;
    if (smax < 1) smax = 1;
    long s = 1, best = -1;
    const long slots = 2 * 256;      // two blocks (2 x 64 KiB of LDS, 104 VGPRs) are resident per CU
    for (long c = 1; c <= smax; ++c) {
        const long rounds = (blocks * c + slots - 1) / slots;
        // + zeroing, writing and re-reading c partial gradients at ~15 MB per stage time
        const long cost = rounds * ((nk + c - 1) / c + 3) + (c > 1 ? c * (long)pl.wfloats * 12 / 15000000 : 0);
        if (best < 0 || cost < best) { best = cost; s = c; }
        if (blocks * c >= 4096) break;
    }
    return s < 1 ? 1 : (int)s;
}

// arrival counters of the in-kernel combine: one int per (tap, n tile, c tile), rounded up to 256 floats
static size_t wgrad_ticket_floats(const t2v_conv_desc* d, int x_cs, const ConvPlan& pl) {
    int ntaps = 0;
    for (int ph = 0; ph < pl.kp.nphases; ++ph) ntaps += pl.kp.ph[ph].ntaps;
    const size_t tiles = wgrad_fold(d, x_cs) ? (size_t)((d->Cout + 127) / 128) * ((ntaps * x_cs + 127) / 128)
                                            : (size_t)ntaps * ((d->Cout + 127) / 128) * ((x_cs + 127) / 128);
    return (tiles + 255) / 256 * 256;
}
static int wgrad_combine_max_splits() { return options().wgrad_combine_max; }
// T2V_WGRAD_COMBINE=0: split partials zero-filled, written and summed by a reduce launch (the round-1 form)
static bool wgrad_combine_on() { return options().wgrad_combine != 0; }

size_t t2v_conv_backward_weight_workspace_floats(const t2v_conv_desc* d, int x_cs, int batch) {
    ConvPlan pl;
    if (!d || is_bf16x2(d->algo) || build_conv_plan(d, x_cs, true, &pl) != T2V_OK) return 0;
    const int dy_cs = round_up(d->Cout, 4);
    if (wgrad_fold_n(d, x_cs, dy_cs)) {   // padded input copy + the partials of its own split rule
        const long nk = ((long)batch * (d->H + 2 * d->pad) * (d->W + 2 * d->pad) + 31) / 32;
        long s = nk / 16;
        if (s > 256) s = 256;
        if (s < 1) s = 1;
        return wgrad_padded_floats(d, x_cs, batch) + (size_t)s * d->Cout * pl.kp.ph[0].Kp;   // partials: the Cout real rows
    }
    const int s = wgrad_splits(d, x_cs, batch, pl);
    return s > 1 ? (size_t)s * pl.wfloats + wgrad_ticket_floats(d, x_cs, pl) : 0;
}

// x_stride / dy_stride: floats between the images (0: the batch's own pitch)
static int backward_weight_impl(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                                int x_cs, long x_stride, const float* dy, int dy_cs, long dy_stride, float* dw_packed,
                                int accumulate, float* workspace) {
    T2V_REQUIRE(ctx && x && dy && dw_packed && batch >= 1, "backward_weight: bad arguments");
    T2V_REFUSE_SPLIT(d, "conv2d_backward_weight");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, true, &pl));   // 128-row weight granule, plain 128x128 bookkeeping
    T2V_REQUIRE(dy_cs >= d->Cout && dy_cs % 4 == 0, "backward_weight: dy channel storage %d", dy_cs);
    const ConvKParams& k = pl.kp;
    WgradParams w;
    memset(&w, 0, sizeof(w));
    w.x = x; w.dy = dy; w.dw = dw_packed;
    w.batch = batch; w.Hin = d->H; w.Win = d->W; w.Cin_s = x_cs;
    w.Wm = k.Wm; w.M = k.M;
    w.Hout = pl.Hout; w.Wout = pl.Wout; w.Cout = d->Cout; w.Cout_s = dy_cs;
    w.stride = k.stride; w.ostride = k.ostride;
    w.reflect = k.pad_mode == T2V_PAD_REFLECT; w.accumulate = accumulate;
    w.ntiles = (d->Cout + 127) / 128; w.ctiles = (x_cs + 127) / 128;
    int nt = 0;
    for (int ph = 0; ph < k.nphases; ++ph)
        for (int t = 0; t < k.ph[ph].ntaps; ++t, ++nt) {
            w.tdy[nt] = k.tdy[k.ph[ph].tap0 + t]; w.tdx[nt] = k.tdx[k.ph[ph].tap0 + t];
            w.toy[nt] = k.ph[ph].oy0; w.tox[nt] = k.ph[ph].ox0;
            w.tap_woff[nt] = k.ph[ph].w_off; w.tap_Kp[nt] = k.ph[ph].Kp; w.tap_kidx[nt] = t;
        }
    w.ntaps = nt;
    w.x_img_stride = (long)d->H * d->W * x_cs;
    w.dy_img_stride = (long)pl.Hout * pl.Wout * dy_cs;
    if (x_stride || dy_stride) {
        T2V_REQUIRE(!(wgrad_fold_n(d, x_cs, dy_cs) && dy_cs == round_up(d->Cout, 4)) && !wgrad_fold(d, x_cs) && conv_wgrad_strided_ok(w),
                    "backward_weight_strided: this shape keeps its images contiguous (t2v_conv_backward_weight_strided_supported)");
        if (x_stride) w.x_img_stride = x_stride;
        if (dy_stride) w.dy_img_stride = dy_stride;
    }
    if (wgrad_fold_n(d, x_cs, dy_cs) && dy_cs == round_up(d->Cout, 4)) {
        // x -> padded copy (reflection / zeros resolved once), taps folded onto the dY side of the tile
        T2V_REQUIRE(workspace, "backward_weight: this shape needs a workspace of "
                               "t2v_conv_backward_weight_workspace_floats() floats");
        hipStream_t st = (hipStream_t)stream;
        const int Hp = d->H + 2 * d->pad, Wp = d->W + 2 * d->pad;
        float* xp = workspace;
        float* partial = workspace + wgrad_padded_floats(d, x_cs, batch);
        T2V_TRY(launch_pad_copy(st, x, xp, batch, d->H, d->W, x_cs, d->pad, k.pad_mode == T2V_PAD_REFLECT));
        T2V_REQUIRE((long)batch * Hp * Wp * x_cs * 4 < 0x7fff0000L, "backward_weight: padded input too large for 32-bit offsets");
        w.x = xp; w.Hin = Hp; w.Win = Wp; w.Wm = Wp; w.M = Hp * Wp;
        w.reflect = 0;
        w.fold = 2; w.fold_taps = nt; w.KW = d->kW; w.pad = 0;
        w.ntiles = (nt * dy_cs + 127) / 128;
        w.ntaps = 1;
        for (int t = 0; t < kMaxTaps; ++t) w.tdy[t] = w.tdx[t] = 0;
        const long nk = ((long)batch * Hp * Wp + 31) / 32;
        long sp = nk / 16;
        if (sp > 256) sp = 256;
        if (sp < 1) sp = 1;
        w.splits = (int)sp;
        // only the first Cout rows of the packed [Cout_p][Kp] matrix are ever written: partials hold just those
        const long part = (long)d->Cout * k.ph[0].Kp;
        w.dw_floats = part;
        w.dw = partial;
        // (taps folded onto the dY side: tile rows are (tap, channel) pairs -- this shape keeps the reduce launch.  No
        // zero-fill of the slabs: every real element of every partial is stored by exactly one block -- a block with an
        // empty pixel range stores zeros -- and the padding columns are summed and never read)
        w.accumulate = 0;
        T2V_TRY(launch_conv_wgrad(st, w));
        return launch_wgrad_reduce(st, partial, w.splits, part, dw_packed, accumulate);
    }
    if (wgrad_fold(d, x_cs)) {
        w.fold = 1; w.fold_taps = nt; w.KW = d->kW; w.pad = d->pad;
        w.ctiles = (nt * x_cs + 127) / 128;
        w.ntaps = 1;
    }
    T2V_REQUIRE((long)batch * d->H * d->W * x_cs * 4 < 0x7fff0000L && (long)batch * pl.Hout * pl.Wout * dy_cs * 4 < 0x7fff0000L,
                "backward_weight: tensors too large for 32-bit buffer offsets (split the batch)");
    w.splits = wgrad_splits(d, x_cs, batch, pl);
    w.dw_floats = (long)pl.wfloats;
    if (w.splits == 1) return launch_conv_wgrad((hipStream_t)stream, w);
    T2V_REQUIRE(workspace, "backward_weight: this shape needs a workspace of "
                           "t2v_conv_backward_weight_workspace_floats() floats");
    w.dw = workspace;
    if (wgrad_combine_on() && w.splits <= wgrad_combine_max_splits()) {
        // in-kernel combine: no zero-fill of the partial slabs, no reduce launch -- only the arrival counters are cleared.
        // For few partials only: the last arriver of a tile reads them one after the other (T2V_WGRAD_COMBINE_MAX).
        int* tickets = reinterpret_cast<int*>(workspace + (size_t)w.splits * pl.wfloats);
        T2V_HIP_CHECK(hipMemsetAsync(tickets, 0, (size_t)w.ntaps * w.ntiles * w.ctiles * sizeof(int), (hipStream_t)stream));
        w.tickets = tickets;
        w.dw_final = dw_packed;
        w.accumulate = accumulate;
        return launch_conv_wgrad((hipStream_t)stream, w);
    }
    // (no zero-fill of the partial slabs either: every real (n, tap, c) element of every slab is stored by exactly one
    // block, zeros where a split's pixel range is empty; the padding rows / columns of the packed layout are summed as they
    // are and never read -- tests/ run with the workspaces NaN-filled (scripts/run_poisoned.py))
    w.accumulate = 0;
    T2V_TRY(launch_conv_wgrad((hipStream_t)stream, w));
    return launch_wgrad_reduce((hipStream_t)stream, workspace, w.splits, (long)pl.wfloats, dw_packed, accumulate);
}

int t2v_conv2d_backward_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                               int x_cs, const float* dy, int dy_cs, float* dw_packed, int accumulate,
                               float* workspace) {
    return backward_weight_impl(ctx, stream, d, batch, x, x_cs, 0, dy, dy_cs, 0, dw_packed, accumulate, workspace);
}
int t2v_conv_backward_weight_strided_supported(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    ConvPlan pl;
    if (!d || is_bf16x2(d->algo) || build_conv_plan(d, x_cs, true, &pl) != T2V_OK) return 0;
    if ((wgrad_fold_n(d, x_cs, dy_cs) && dy_cs == round_up(d->Cout, 4)) || wgrad_fold(d, x_cs)) return 0;
    WgradParams w;
    memset(&w, 0, sizeof(w));
    w.reflect = pl.kp.pad_mode == T2V_PAD_REFLECT;
    w.Wm = pl.kp.Wm;
    w.M = pl.kp.M;
    return conv_wgrad_strided_ok(w) ? 1 : 0;
}
int t2v_conv2d_backward_weight_strided(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                                       int x_cs, long x_img_stride, const float* dy, int dy_cs, long dy_img_stride,
                                       float* dw_packed, int accumulate, float* workspace) {
    T2V_REQUIRE(x_img_stride != 0 && dy_img_stride != 0, "backward_weight_strided: zero image stride");
    return backward_weight_impl(ctx, stream, d, batch, x, x_cs, x_img_stride, dy, dy_cs, dy_img_stride, dw_packed, accumulate,
                                workspace);
}

// ---- weight gradient in the Winograd domain (F(4x4,3x3)) -------------------------------------------------
static bool wgrad_winograd_ok(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    return !is_bf16x2(d->algo) && winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD_F4) && dy_cs == d->Cout && d->Cout % 4 == 0;
}
int t2v_conv_backward_weight_winograd_supported(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    return d && wgrad_winograd_ok(d, x_cs, dy_cs) ? 1 : 0;
}
size_t t2v_conv_backward_weight_winograd_workspace_floats(const t2v_conv_desc* d, int x_cs, int batch) {
    if (!d || batch < 1 || is_bf16x2(d->algo) || !winograd_supported(d, x_cs, T2V_ALGO_WINOGRAD_F4)) return 0;
    const size_t Tp = (size_t)wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4);
    const size_t Cout_p = (size_t)round_up(d->Cout, 128), Kp = (size_t)round_up(x_cs, kBK);
    // V, M_dy, dU, then the hand-over area of the fixed-grid reduction (conv_wgrad.hip: wino_wgrad_sk_kernel)
    return 36 * batch * Tp * ((size_t)x_cs + d->Cout) + 36 * Cout_p * Kp + wino_gemm_sk_scratch_floats();
}
int t2v_conv_winograd_tile_rows(const t2v_conv_desc* d) {
    return d ? wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4) : 0;
}
int t2v_conv_winograd_gemm_form(const t2v_conv_desc* d, int nimg) {
    if (!d || !is_f4(d->algo) || nimg < 1) return -1;
    if (is_split(d->algo)) return wino_split_gemm_ok(36, wino_rows_batch(d, d->algo, nimg), d->Cin, d->Cout) ? T2V_GEMM_SPLIT_BF16_128x128 : -1;
    PositionGemm g;      // as winograd_forward fills it
    g.groups = 36; g.rows = nimg * wino_tiles_real(d, d->algo); g.T = wino_rows_batch(d, d->algo, nimg);
    g.K = d->Cin; g.N = d->Cout;
    return position_gemm_form(g);
}
int t2v_conv2d_backward_weight_winograd_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int b0,
                                               int nb, const float* x, int x_cs, const float* dy, int dy_cs,
                                               float* dw_torch, int accumulate, float* workspace, int stages) {
    T2V_REQUIRE(ctx && d && workspace && batch >= 1 && b0 >= 0 && nb >= 0 && b0 + nb <= batch,
                "backward_weight_winograd: bad arguments");
    T2V_REFUSE_SPLIT(d, "conv2d_backward_weight_winograd");
    T2V_REQUIRE(wgrad_winograd_ok(d, x_cs, dy_cs), "backward_weight_winograd: shape not supported "
                                                  "(t2v_conv_backward_weight_winograd_supported)");
    hipStream_t s = (hipStream_t)stream;
    const int Ho = wino_out_h(d), Wo = wino_out_w(d);
    const int Tp = wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4), Tt = batch * Tp;
    const int Cout_p = round_up(d->Cout, 128), Kp = round_up(x_cs, kBK);
    float* V = workspace;
    float* Md = V + (size_t)36 * Tt * x_cs;
    float* dU = Md + (size_t)36 * Tt * d->Cout;
    T2V_REQUIRE((long)36 * Tt * x_cs * 4 < 0x7fff0000L && (long)36 * Tt * d->Cout * 4 < 0x7fff0000L,
                "backward_weight_winograd: transformed tensors too large for 32-bit buffer offsets (split the batch)");
    if (stages & 1) {   // transforms of images [b0, b0 + nb) into their slots of the batch-wide tile lists
        // (x == null: the forward pass has put V of these images there -- t2v_conv2d_forward_winograd_keep_v)
        T2V_REQUIRE(dy, "backward_weight_winograd: null image pointers");
        for (int b = 0; b < nb; ++b) {
            if (x)
            T2V_TRY(launch_winograd4_input(s, x + (size_t)b * d->H * d->W * x_cs, V, d->H, d->W, x_cs, d->pad,
                                           d->pad_mode == T2V_PAD_REFLECT, batch, b0 + b));
            T2V_TRY(launch_winograd4_dy(s, dy + (size_t)b * Ho * Wo * dy_cs, Md, Ho, Wo, d->Cout, dy_cs, batch, b0 + b));
        }
    }
    if (!(stages & 2)) return T2V_OK;
    T2V_REQUIRE(dw_torch, "backward_weight_winograd: null gradient pointer");
    // 36 reductions over the tiles on the pixel-reduction GEMM: position xi = row xi of a [36][Tt] image, taken
    // by "tap" xi (input row offset xi, output row offset xi, its own output matrix)
    WgradParams w;
    memset(&w, 0, sizeof(w));
    w.x = V; w.dy = Md; w.dw = dU;
    w.batch = 1; w.Hin = 36; w.Win = Tt; w.Cin_s = x_cs;
    w.x_img_stride = (long)36 * Tt * x_cs; w.dy_img_stride = (long)36 * Tt * d->Cout;
    w.Wm = Tt; w.M = Tt;
    w.Hout = 36; w.Wout = Tt; w.Cout = d->Cout; w.Cout_s = d->Cout;
    w.stride = 1; w.ostride = 1;
    w.reflect = 0; w.accumulate = 0;
    w.ntiles = (d->Cout + 127) / 128; w.ctiles = (x_cs + 127) / 128;
    static_assert(kMaxTaps >= 36, "one tap slot per Winograd transform position");
    for (int xi = 0; xi < 36; ++xi) {
        w.tdy[xi] = xi; w.tdx[xi] = 0;
        w.toy[xi] = xi; w.tox[xi] = 0;
        w.tap_woff[xi] = (long)xi * Cout_p * Kp; w.tap_Kp[xi] = Kp; w.tap_kidx[xi] = 0;
    }
    w.ntaps = 36;
    w.splits = 1;
    w.dw_floats = (long)36 * Cout_p * Kp;
    T2V_TRY(check_async_errors());
    if (wino_wgrad_sk_ok(Tt, x_cs, d->Cout))
        T2V_TRY(launch_wino_wgrad_sk(s, V, Md, dU, dU + (size_t)36 * Cout_p * Kp, Tt, x_cs, d->Cout, Cout_p, Kp));
    else
        T2V_TRY(launch_conv_wgrad(s, w));
    return launch_winograd4_dw(s, dU, dw_torch, d->Cout, d->Cin, Cout_p, Kp, accumulate);
}

int t2v_conv2d_backward_weight_winograd_dy_norm(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                                int x_cs, const float* conv_out, const float* dy, const float* mean_rstd,
                                                const float* gamma, const float* beta, int relu, const float* sums,
                                                float* workspace) {
    T2V_REQUIRE(ctx && d && conv_out && dy && mean_rstd && sums && workspace && batch >= 1 && slot >= 0 && slot < batch,
                "backward_weight_winograd_dy_norm: bad arguments");
    T2V_REFUSE_SPLIT(d, "conv2d_backward_weight_winograd_dy_norm");
    T2V_REQUIRE(wgrad_winograd_ok(d, x_cs, d->Cout), "backward_weight_winograd_dy_norm: shape not supported "
                                                     "(t2v_conv_backward_weight_winograd_supported)");
    const int Tp = wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4), Tt = batch * Tp;
    T2V_REQUIRE((long)36 * Tt * d->Cout * 4 < 0x7fff0000L, "backward_weight_winograd_dy_norm: A dy A^T too large for 32-bit offsets");
    float* Md = workspace + (size_t)36 * Tt * x_cs;
    return launch_winograd4_dy_norm((hipStream_t)stream, dy, conv_out, mean_rstd, gamma, beta, relu, sums, Md, wino_out_h(d),
                                    wino_out_w(d), d->Cout, batch, slot);
}

int t2v_conv2d_backward_weight_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                                        int x_cs, const float* dy, int dy_cs, float* dw_torch, int accumulate,
                                        float* workspace) {
    T2V_REQUIRE(x && dy && dw_torch, "backward_weight_winograd: bad arguments");
    return t2v_conv2d_backward_weight_winograd_stages(ctx, stream, d, batch, 0, batch, x, x_cs, dy, dy_cs, dw_torch,
                                                      accumulate, workspace, 3);
}

// ---- data gradient by the transposed Winograd algorithm (winograd.hip: winograd4_dgrad_output_kernel) -------------------
static bool dgrad_winograd_ok(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    return wgrad_winograd_ok(d, x_cs, dy_cs) && d->pad_mode == T2V_PAD_REFLECT && d->pad == 1 && d->H % 4 == 0 && d->W % 4 == 0 &&
           d->Cout % kBK == 0;
}
int t2v_conv_backward_data_winograd_supported(const t2v_conv_desc* d, int x_cs, int dy_cs) {   // (0 for a split-bf16 desc)
    return d && dgrad_winograd_ok(d, x_cs, dy_cs) ? 1 : 0;
}
size_t t2v_conv_backward_data_winograd_weight_floats(const t2v_conv_desc* d, int x_cs) {
    if (!d) return 0;
    return (size_t)36 * round_up(x_cs, 128) * round_up(d->Cout, kBK);
}
size_t t2v_conv_backward_data_winograd_scratch_floats(const t2v_conv_desc* d, int x_cs) {
    if (!d) return 0;
    return (size_t)36 * wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4) * x_cs + (size_t)(d->H + 2) * (d->W + 2) * x_cs +
           wino_gemm_sk_scratch_floats();
}
int t2v_conv_pack_weight_transposed(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* w_forward_dev,
                                    float* packed_dev) {
    T2V_REQUIRE(ctx && d && w_forward_dev && packed_dev, "pack_weight_transposed: null pointer");
    T2V_REFUSE_SPLIT(d, "conv_pack_weight_transposed");
    T2V_REQUIRE(dgrad_winograd_ok(d, x_cs, d->Cout), "pack_weight_transposed: shape not supported "
                                                     "(t2v_conv_backward_data_winograd_supported)");
    // U^T[xi][c][n]: the rows are the forward layer's INPUT channels, K runs over its OUTPUT channels
    return launch_winograd4_weight((hipStream_t)stream, w_forward_dev, packed_dev, /*rows*/ d->Cin, /*K*/ d->Cout,
                                   round_up(x_cs, 128), round_up(d->Cout, kBK), /*transpose, no flip*/ 2);
}
// the forward layer's own packed U [36][Cout_p][x_cs] serves as the B matrix [K = Cout][N = x_cs] of dV = dM U when the
// fixed-grid GEMM has its [K][N] form for the shape (conv_igemm.hip: wino_gemm_sk_kernel<.., BKN>) and no padding rows sit
// between the positions
static bool dgrad_winograd_forward_weights_ok(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    if (!dgrad_winograd_ok(d, x_cs, dy_cs)) return false;
    t2v_conv_desc f = *d;
    f.algo = T2V_ALGO_WINOGRAD_F4;
    ConvPlan pl;
    if (!winograd_supported(&f, x_cs, f.algo) || build_conv_plan(&f, x_cs, false, &pl) != T2V_OK || pl.Cout_p != d->Cout) return false;
    return wino_gemm_sk_bkn_ok(36, wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4), d->Cout, x_cs, x_cs);
}
int t2v_conv_backward_data_winograd_takes_forward_weights(const t2v_conv_desc* d, int x_cs, int dy_cs) {
    return d && dgrad_winograd_forward_weights_ok(d, x_cs, dy_cs) ? 1 : 0;
}
static int backward_data_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                  const float* wgrad_workspace, int x_cs, const float* ut_packed, bool forward_weights,
                                  float* scratch, float* dx);
int t2v_conv2d_backward_data_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                      const float* wgrad_workspace, int x_cs, const float* ut_packed, float* scratch, float* dx) {
    return backward_data_winograd(ctx, stream, d, batch, slot, wgrad_workspace, x_cs, ut_packed, false, scratch, dx);
}
int t2v_conv2d_backward_data_winograd_fw(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                         const float* wgrad_workspace, int x_cs, const float* u_forward_packed, float* scratch,
                                         float* dx) {
    T2V_REFUSE_SPLIT(d, "conv2d_backward_data_winograd_fw");
    T2V_REQUIRE(d && dgrad_winograd_forward_weights_ok(d, x_cs, d->Cout),
                "backward_data_winograd_fw: shape not supported (t2v_conv_backward_data_winograd_takes_forward_weights)");
    return backward_data_winograd(ctx, stream, d, batch, slot, wgrad_workspace, x_cs, u_forward_packed, true, scratch, dx);
}
static int backward_data_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                  const float* wgrad_workspace, int x_cs, const float* ut_packed, bool forward_weights,
                                  float* scratch, float* dx) {
    T2V_REQUIRE(ctx && d && wgrad_workspace && ut_packed && scratch && dx && batch >= 1 && slot >= 0 && slot < batch,
                "backward_data_winograd: bad arguments");
    T2V_REFUSE_SPLIT(d, "conv2d_backward_data_winograd");
    T2V_REQUIRE(dgrad_winograd_ok(d, x_cs, d->Cout), "backward_data_winograd: shape not supported");
    T2V_TRY(check_async_errors());
    hipStream_t s = (hipStream_t)stream;
    const int Tp = wino_tiles_padded(d, T2V_ALGO_WINOGRAD_F4), Tt = batch * Tp;
    // M_dy = A dy A^T of all `batch` images sits behind V in the weight gradient's workspace ([36][Tt][Cout] each)
    const float* Md = wgrad_workspace + (size_t)36 * Tt * x_cs;
    float* dV = scratch;
    float* dxp = scratch + (size_t)36 * Tp * x_cs;
    // dV[xi][t][c] = sum_n M_dy[xi][slot*Tp + t][n] * U[xi][n][c]: the batched GEMM of a conv with the channel roles swapped,
    // reading its rows out of the batch-wide matrix (input row pitch Tt, Tp rows per position)
    // (rows not given: only the whole-tile fixed grid or one block per tile)
    PositionGemm g;
    g.groups = 36; g.T = Tp; g.K = d->Cout; g.N = x_cs;
    g.a_pitch = Tt;
    g.b_kn = forward_weights;
    T2V_TRY(run_position_gemm(ctx, s, g, Md + (size_t)slot * Tp * d->Cout, ut_packed, dV, dxp + (size_t)(d->H + 2) * (d->W + 2) * x_cs));
    T2V_TRY(launch_winograd4_dgrad_output(s, dV, dxp, d->H, d->W, x_cs));
    return launch_reflect_pad_backward(s, dxp, dx, d->H, d->W, x_cs, 1);
}

int t2v_conv_unpack_weight_into(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* packed_dev,
                                float* w_torch_dev, int accumulate) {
    T2V_REQUIRE(ctx && packed_dev && w_torch_dev, "unpack_weight: null pointer");
    T2V_REFUSE_SPLIT(d, "conv_unpack_weight");
    ConvPlan pl;
    T2V_TRY(build_conv_plan(d, x_cs, false, &pl));
    if (!d->transposed)
        return launch_unpack_conv_weight((hipStream_t)stream, packed_dev, w_torch_dev, d->Cout, d->Cin, d->kH, d->kW, x_cs,
                                         pl.kp.ph[0].Kp, accumulate);
    return launch_unpack_convT_weight((hipStream_t)stream, packed_dev, w_torch_dev, d->Cin, d->Cout, x_cs, pl.Cout_p,
                                      d->kH, d->pad, accumulate);
}
int t2v_conv_unpack_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* packed_dev,
                           float* w_torch_dev) {
    return t2v_conv_unpack_weight_into(ctx, stream, d, x_cs, packed_dev, w_torch_dev, 0);
}
int t2v_accumulate(t2v_ctx* ctx, void* stream, float* dst, const float* src, long n, int overwrite) {
    T2V_REQUIRE(ctx && dst && src && n > 0, "accumulate: bad arguments");
    return launch_accumulate((hipStream_t)stream, dst, src, n, overwrite);
}
int t2v_scale(t2v_ctx* ctx, void* stream, float* x, long n, float s) {
    T2V_REQUIRE(ctx && x && n > 0, "scale: bad arguments");
    return launch_scale((hipStream_t)stream, x, n, s);
}
int t2v_unzip2(t2v_ctx* ctx, void* stream, const float* src, float* dst0, float* dst1, int C, int overwrite) {
    T2V_REQUIRE(ctx && src && dst0 && dst1 && C > 0, "unzip2: bad arguments");
    return launch_unzip2((hipStream_t)stream, src, dst0, dst1, C, overwrite);
}
int t2v_zero(t2v_ctx* ctx, void* stream, void* ptr, size_t bytes) {
    T2V_REQUIRE(ctx && ptr, "zero: null pointer");
    T2V_HIP_CHECK(hipMemsetAsync(ptr, 0, bytes, (hipStream_t)stream));
    return T2V_OK;
}

int t2v_channel_sum(t2v_ctx* ctx, void* stream, const float* x, long npix, int C, int cs, float* scratch, float* out) {
    T2V_REQUIRE(ctx && x && out && scratch && C > 0 && cs >= C, "channel_sum: bad arguments");
    return launch_channel_sum((hipStream_t)stream, x, npix, C, cs, scratch, out);
}

int t2v_reflect_pad_backward(t2v_ctx* ctx, void* stream, const float* dxp, float* dx, int H, int W, int C, int pad) {
    T2V_REQUIRE(ctx && dxp && dx && pad >= 0 && H > 2 * pad && W > 2 * pad, "reflect_pad_backward: bad arguments");
    return launch_reflect_pad_backward((hipStream_t)stream, dxp, dx, H, W, C, pad);
}
int t2v_instance_norm_backward(t2v_ctx* ctx, void* stream, const float* x, const float* dy, const float* mean_rstd,
                               const float* gamma, const float* beta, int relu, long npix, int C, float* scratch,
                               float* dx, float* dbeta_dgamma) {
    // (dx == null: the two sums only -- the gradient itself is formed by its consumer, t2v_conv2d_backward_weight_winograd_dy_norm)
    T2V_REQUIRE(ctx && x && dy && mean_rstd && scratch && dbeta_dgamma && npix > 0 && C > 0,
                "instance_norm_backward: bad arguments");
    return launch_inorm_backward((hipStream_t)stream, x, dy, mean_rstd, gamma, beta, relu, npix, C, scratch, dx,
                                 dbeta_dgamma);
}
int t2v_instance_norm_backward_affine(t2v_ctx* ctx, void* stream, const float* x, const float* dy, const float* mean_rstd,
                                      const float* gamma, const float* beta, int relu, long npix, int C, float* scratch,
                                      float* dx, float* dbeta_dgamma, float* d_beta, float* d_gamma, int overwrite) {
    T2V_REQUIRE(ctx && x && dy && mean_rstd && scratch && dbeta_dgamma && d_beta && d_gamma && npix > 0 && C > 0,
                "instance_norm_backward_affine: bad arguments");
    return launch_inorm_backward((hipStream_t)stream, x, dy, mean_rstd, gamma, beta, relu, npix, C, scratch, dx,
                                 dbeta_dgamma, d_beta, d_gamma, overwrite);
}
int t2v_act_backward(t2v_ctx* ctx, void* stream, const float* dy, const float* y, int act, float slope, long n,
                     float* dpre) {
    T2V_REQUIRE(ctx && dy && y && dpre && n > 0, "act_backward: bad arguments");
    return launch_act_backward((hipStream_t)stream, dy, y, act, slope, n, dpre);
}
int t2v_avgpool3x3s2_backward(t2v_ctx* ctx, void* stream, const float* dy, float* dx, int H, int W, int C) {
    T2V_REQUIRE(ctx && dy && dx, "avgpool_backward: null pointer");
    return launch_avgpool3s2_backward((hipStream_t)stream, dy, dx, H, W, C);
}
int t2v_maxpool2x2(t2v_ctx* ctx, void* stream, const float* x, float* y, int H, int W, int C) {
    T2V_REQUIRE(ctx && x && y && H >= 2 && W >= 2 && C >= 1, "maxpool2x2: bad arguments");
    return launch_maxpool2x2((hipStream_t)stream, x, y, H, W, C);
}
int t2v_maxpool2x2_backward(t2v_ctx* ctx, void* stream, const float* x, const float* dy, float* dx, int H, int W, int C) {
    T2V_REQUIRE(ctx && x && dy && dx && H >= 2 && W >= 2 && C >= 1, "maxpool2x2_backward: bad arguments");
    return launch_maxpool2x2_backward((hipStream_t)stream, x, dy, dx, H, W, C);
}
int t2v_sum_sq_diff_const_backward(t2v_ctx* ctx, void* stream, const float* x, float c, float scale, long n, float* dx) {
    T2V_REQUIRE(ctx && x && dx && n > 0, "mse backward: bad arguments");
    return launch_loss_backward((hipStream_t)stream, 0, x, nullptr, c, scale, n, dx);
}
int t2v_sum_abs_diff_backward(t2v_ctx* ctx, void* stream, const float* a, const float* b, float scale, long n, float* da) {
    T2V_REQUIRE(ctx && a && b && da && n > 0, "l1 backward: bad arguments");
    return launch_loss_backward((hipStream_t)stream, 1, a, b, 0.f, scale, n, da);
}

int t2v_sum_sq_diff_const(t2v_ctx* ctx, void* stream, const float* x, float c, long n, float* scratch, float* out) {
    T2V_REQUIRE(ctx && x && scratch && out && n > 0, "sum_sq_diff_const: bad arguments");
    return launch_reduce((hipStream_t)stream, 0, x, nullptr, c, n, scratch, out);
}
int t2v_sum_abs_diff(t2v_ctx* ctx, void* stream, const float* a, const float* b, long n, float* scratch, float* out) {
    T2V_REQUIRE(ctx && a && b && scratch && out && n > 0, "sum_abs_diff: bad arguments");
    return launch_reduce((hipStream_t)stream, 1, a, b, 0.f, n, scratch, out);
}
int t2v_sum_abs_diff_masked(t2v_ctx* ctx, void* stream, const float* a, const float* b, const float* mask, long npix,
                            int c0, int C, int cs, float* scratch, float* out) {
    T2V_REQUIRE(ctx && a && scratch && out && npix > 0 && c0 >= 0 && C > 0 && cs >= c0 + C,
                "sum_abs_diff_masked: bad arguments");
    return launch_masked_l1((hipStream_t)stream, a, b, mask, npix, c0, C, cs, scratch, out);
}
int t2v_sum_abs_diff_masked_backward(t2v_ctx* ctx, void* stream, const float* a, const float* b, const float* mask,
                                     float scale, long npix, int c0, int C, int cs, float* da) {
    T2V_REQUIRE(ctx && a && da && npix > 0 && c0 >= 0 && C > 0 && cs >= c0 + C,
                "sum_abs_diff_masked_backward: bad arguments");
    return launch_masked_l1_backward((hipStream_t)stream, a, b, mask, scale, npix, c0, C, cs, da);
}
int t2v_loss_terms(t2v_ctx* ctx, void* stream, const int64_t* term_ptrs, const int32_t* term_ints, const float* term_floats,
                   const int32_t* chunk_term, const int64_t* chunk_off, const int32_t* term_chunk0, int nterms, int nchunks,
                   int chunk, float* partials, float* out) {
    T2V_REQUIRE(ctx && term_ptrs && term_ints && term_floats && chunk_term && chunk_off && term_chunk0 && partials && out,
                "loss_terms: null pointer");
    T2V_REQUIRE(nterms > 0 && nchunks > 0 && chunk > 0 && chunk % 4 == 0, "loss_terms: nterms %d nchunks %d chunk %d", nterms,
                nchunks, chunk);
    return launch_loss_terms((hipStream_t)stream, reinterpret_cast<const long long*>(term_ptrs), term_ints, term_floats,
                             chunk_term, reinterpret_cast<const long long*>(chunk_off), term_chunk0, nterms, nchunks, chunk,
                             partials, out);
}
int t2v_adam_step(t2v_ctx* ctx, void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  long n, double lr, double beta1, double beta2, double eps, int step) {
    T2V_REQUIRE(ctx && param && grad && exp_avg && exp_avg_sq && n > 0 && step >= 1, "adam_step: bad arguments");
    return launch_adam((hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, step);
}

int t2v_adam_step_multi(t2v_ctx* ctx, void* stream, const int64_t* ptrs, const int64_t* nelem, const float* step_size,
                        const int32_t* chunk_tensor, const int64_t* chunk_off, int nchunks, int chunk, double beta1,
                        double beta2, double eps) {
    T2V_REQUIRE(ctx && ptrs && nelem && step_size && chunk_tensor && chunk_off && nchunks > 0 && chunk > 0,
                "adam_step_multi: bad arguments");
    return launch_adam_multi((hipStream_t)stream, reinterpret_cast<const long long*>(ptrs),
                             reinterpret_cast<const long long*>(nelem), step_size, chunk_tensor,
                             reinterpret_cast<const long long*>(chunk_off), nchunks, chunk, beta1, beta2, eps);
}

int t2v_batch_norm_update_running(t2v_ctx* ctx, void* stream, const float* mean_rstd, float* running_mean,
                                  float* running_var, long n, int C, float momentum, float eps) {
    T2V_REQUIRE(ctx && mean_rstd && running_mean && running_var && C > 0 && n > 1,
                "batch_norm_update_running: bad arguments (needs more than one value per channel)");
    return launch_bn_running_update((hipStream_t)stream, mean_rstd, running_mean, running_var, n, momentum, eps, C);
}

int t2v_instance_norm_apply(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd, const float* gamma,
                            const float* beta, const float* res1, const float* res2, float* y, long npix, int C,
                            int relu) {
    T2V_REQUIRE(ctx && x && mean_rstd && y, "inorm_apply: null pointer");
    T2V_REQUIRE((gamma == nullptr) == (beta == nullptr), "inorm_apply: gamma and beta must both be given or both NULL");
    return launch_inorm_apply((hipStream_t)stream, x, mean_rstd, gamma, beta, res1, res2, y, npix, C, relu);
}
// the batch form, the encoder join and the plain sum of the norm-apply kernels (additive to the ABI): the launches the
// generator's frames make, callable on their own
int t2v_instance_norm_apply_bf16x2(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd, const float* gamma,
                                   const float* beta, float* y, long npix, int C, int relu) {
    T2V_REQUIRE(ctx && x && mean_rstd && y, "instance_norm_apply_bf16x2: null pointer");
    T2V_REQUIRE(C > 0 && C % 4 == 0 && npix >= 1, "instance_norm_apply_bf16x2: C=%d (a multiple of 4), npix=%ld", C, npix);
    T2V_REQUIRE((gamma == nullptr) == (beta == nullptr), "instance_norm_apply_bf16x2: gamma and beta must both be given or both NULL");
    return launch_inorm_apply_split((hipStream_t)stream, x, mean_rstd, gamma, beta, nullptr, y, npix, C, relu);
}
int t2v_instance_norm_apply_batch(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd, const float* gamma,
                                  const float* beta, const float* res1, const float* res2, float* y, long npix, int C,
                                  int relu, int nimg) {
    T2V_REQUIRE(ctx && x && mean_rstd && y, "inorm_apply_batch: null pointer");
    T2V_REQUIRE((gamma == nullptr) == (beta == nullptr), "inorm_apply_batch: gamma and beta must both be given or both NULL");
    T2V_REQUIRE(C > 0 && C % 4 == 0, "inorm_apply_batch: C=%d must be a positive multiple of 4", C);
    T2V_REQUIRE(npix >= 1 && nimg >= 1 && nimg <= 65535, "inorm_apply_batch: npix=%ld nimg=%d", npix, nimg);
    T2V_REQUIRE(relu >= 0 && relu <= 2, "inorm_apply_batch: relu=%d", relu);
    return launch_inorm_apply((hipStream_t)stream, x, mean_rstd, gamma, beta, res1, res2, y, npix, C, relu, nimg);
}
int t2v_instance_norm_join(t2v_ctx* ctx, void* stream, const float* a_y, const float* a_mean_rstd, const float* a_gamma,
                           const float* a_beta, const float* a_res, const float* b_y, const float* b_mean_rstd,
                           const float* b_gamma, const float* b_beta, const float* b_res, float* y, long npix, int C,
                           int nimg) {
    T2V_REQUIRE(ctx && a_y && a_mean_rstd && a_res && b_y && b_mean_rstd && b_res && y, "inorm_join: null pointer");
    T2V_REQUIRE((a_gamma == nullptr) == (a_beta == nullptr) && (b_gamma == nullptr) == (b_beta == nullptr),
                "inorm_join: gamma and beta must both be given or both NULL");
    T2V_REQUIRE(C > 0 && C % 4 == 0, "inorm_join: C=%d must be a positive multiple of 4", C);
    T2V_REQUIRE(npix >= 1 && nimg >= 1 && nimg <= 65535, "inorm_join: npix=%ld nimg=%d", npix, nimg);
    NormJoinSide a, b;
    a.y = a_y; a.mean_rstd = a_mean_rstd; a.gamma = a_gamma; a.beta = a_beta; a.res = a_res;
    b.y = b_y; b.mean_rstd = b_mean_rstd; b.gamma = b_gamma; b.beta = b_beta; b.res = b_res;
    return launch_inorm_join((hipStream_t)stream, a, b, y, npix, C, nimg);
}
int t2v_add(t2v_ctx* ctx, void* stream, const float* a, const float* b, float* y, long n) {
    T2V_REQUIRE(ctx && a && b && y, "add: null pointer");
    T2V_REQUIRE(n >= 4 && n % 4 == 0, "add: n=%ld must be a positive multiple of 4", n);
    return launch_add((hipStream_t)stream, a, b, y, n);
}

int t2v_flow_warp_composite(t2v_ctx* ctx, void* stream, const float* raw, const float* fw, const float* prev,
                            int prev_cs, int prev_c0, float* out, float* warp_out, int H, int W) {
    T2V_REQUIRE(ctx && fw && prev && (out || warp_out), "flow_warp_composite: null pointer");
    T2V_REQUIRE(raw == nullptr || out != nullptr, "flow_warp_composite: raw without out");
    T2V_REQUIRE(H > 1 && W > 1, "flow_warp_composite: H,W must be > 1");
    T2V_REQUIRE(prev_c0 >= 0 && prev_c0 + 3 <= prev_cs, "flow_warp_composite: prev_c0 + 3 > prev_cs");
    return launch_warp_composite((hipStream_t)stream, raw, fw, prev, prev_cs, prev_c0, out, warp_out, H, W);
}
int t2v_flow_warp_composite_backward(t2v_ctx* ctx, void* stream, const float* d_out, const float* d_warp,
                                     const float* raw, const float* fw, const float* prev, int prev_cs, int prev_c0,
                                     float* d_raw, float* d_fw, float* d_prev, int H, int W) {
    T2V_REQUIRE(ctx && fw && prev && d_fw && (d_out || d_warp), "flow_warp_composite_backward: null pointer");
    T2V_REQUIRE(d_out == nullptr || raw != nullptr, "flow_warp_composite_backward: d_out needs raw (the blend's operands)");
    T2V_REQUIRE(H > 1 && W > 1, "flow_warp_composite_backward: H,W must be > 1");
    T2V_REQUIRE(prev_c0 >= 0 && prev_c0 + 3 <= prev_cs, "flow_warp_composite_backward: prev_c0 + 3 > prev_cs");
    return launch_warp_composite_backward((hipStream_t)stream, d_out, d_warp, raw, fw, prev, prev_cs, prev_c0, d_raw,
                                          d_fw, d_prev, H, W);
}

int t2v_avgpool3x3s2(t2v_ctx* ctx, void* stream, const float* x, float* y, int H, int W, int C) {
    T2V_REQUIRE(ctx && x && y, "avgpool: null pointer");
    return launch_avgpool3s2((hipStream_t)stream, x, y, H, W, C);
}

int t2v_nchw_to_nhwc(t2v_ctx* ctx, void* stream, const float* src, float* dst, int C, int H, int W, int dst_cs) {
    T2V_REQUIRE(ctx && src && dst && dst_cs >= C, "nchw_to_nhwc: bad arguments");
    return launch_nchw_to_nhwc((hipStream_t)stream, src, dst, C, H, W, dst_cs);
}
int t2v_nhwc_to_nchw(t2v_ctx* ctx, void* stream, const float* src, float* dst, int C, int H, int W, int src_cs) {
    T2V_REQUIRE(ctx && src && dst && src_cs >= C, "nhwc_to_nchw: bad arguments");
    return launch_nhwc_to_nchw((hipStream_t)stream, src, dst, C, H, W, src_cs);
}
int t2v_pose_u8_to_f32(t2v_ctx* ctx, void* stream, const uint8_t* src_hwc3, float* dst, long npix, int dst_cs,
                       int c0) {
    T2V_REQUIRE(ctx && src_hwc3 && dst && c0 + 3 <= dst_cs, "pose_u8_to_f32: bad arguments");
    return launch_u8_pose_to_f32((hipStream_t)stream, src_hwc3, dst, npix, dst_cs, c0);
}
int t2v_tensor2im_u8(t2v_ctx* ctx, void* stream, const float* x, uint8_t* y, long n) {
    T2V_REQUIRE(ctx && x && y, "tensor2im: null pointer");
    return launch_to_u8((hipStream_t)stream, x, y, n);
}
int t2v_copy_channels(t2v_ctx* ctx, void* stream, const float* src, int src_cs, int src_c0, float* dst, int dst_cs,
                      int dst_c0, int nc, long npix) {
    T2V_REQUIRE(ctx && src && dst && src_c0 + nc <= src_cs && dst_c0 + nc <= dst_cs, "copy_channels: bad arguments");
    return launch_copy_channels((hipStream_t)stream, src, src_cs, src_c0, dst, dst_cs, dst_c0, nc, npix);
}

// ---- dense optical flow (ABI 20) ----
size_t t2v_optical_flow_workspace_floats(int H, int W, int levels) {
    return optical_flow_shape_ok(H, W, levels) ? optical_flow_workspace_floats(H, W, levels) : 0;
}
int t2v_optical_flow(t2v_ctx* ctx, void* stream, const float* cur, int cur_cs, int cur_c0, const float* prev, int prev_cs,
                     int prev_c0, int H, int W, int levels, int iters, int radius, float lambda, float* workspace,
                     float* flow_out) {
    T2V_REQUIRE(ctx && cur && prev && workspace && flow_out, "optical_flow: null pointer");
    T2V_REQUIRE(H >= 8 && W >= 8, "optical_flow: H, W must be >= 8 (got %d x %d)", H, W);
    T2V_REQUIRE(optical_flow_shape_ok(H, W, levels), "optical_flow: unsupported size %d x %d or level count %d", H, W, levels);
    T2V_REQUIRE(radius >= 1 && radius <= 7, "optical_flow: radius must be in 1..7 (got %d)", radius);
    T2V_REQUIRE(iters >= 1, "optical_flow: iters must be >= 1 (got %d)", iters);
    T2V_REQUIRE(lambda > 0.f, "optical_flow: lambda must be > 0");
    T2V_REQUIRE(cur_c0 >= 0 && cur_c0 + 3 <= cur_cs && prev_c0 >= 0 && prev_c0 + 3 <= prev_cs,
                "optical_flow: the three channels from c0 must lie inside the channel stride");
    return launch_optical_flow((hipStream_t)stream, cur, cur_cs, cur_c0, prev, prev_cs, prev_c0, H, W, levels, iters, radius,
                               lambda, workspace, flow_out);
}

// the same flow on uint8 HWC frames (additive to ABI 22): only the grey launch differs
int t2v_optical_flow_u8(t2v_ctx* ctx, void* stream, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs, int H,
                        int W, int levels, int iters, int radius, float lambda, float* workspace, float* flow_out) {
    T2V_REQUIRE(ctx && cur && prev && workspace && flow_out, "optical_flow_u8: null pointer");
    T2V_REQUIRE(H >= 8 && W >= 8, "optical_flow_u8: H, W must be >= 8 (got %d x %d)", H, W);
    T2V_REQUIRE(optical_flow_shape_ok(H, W, levels), "optical_flow_u8: unsupported size %d x %d or level count %d", H, W, levels);
    T2V_REQUIRE(radius >= 1 && radius <= 7, "optical_flow_u8: radius must be in 1..7 (got %d)", radius);
    T2V_REQUIRE(iters >= 1, "optical_flow_u8: iters must be >= 1 (got %d)", iters);
    T2V_REQUIRE(lambda > 0.f, "optical_flow_u8: lambda must be > 0");
    T2V_REQUIRE((cur_cs == 3 || cur_cs == 4) && (prev_cs == 3 || prev_cs == 4),
                "optical_flow_u8: channel strides must be 3 or 4 (got %d and %d)", cur_cs, prev_cs);
    return launch_optical_flow_u8((hipStream_t)stream, cur, cur_cs, prev, prev_cs, H, W, levels, iters, radius, lambda, workspace,
                                  flow_out);
}

// ---- image resampling for the training loader (ABI 21) ----
int t2v_resample_crop_normalize_u8(t2v_ctx* ctx, void* stream, const uint8_t* src, int T, int h, int w,
                                   const int32_t* x_first, const int32_t* x_count, const int32_t* x_coef, int kx, int out_w,
                                   const int32_t* y_first, const int32_t* y_count, const int32_t* y_coef, int ky, int out_h,
                                   int crop_x, int crop_y, int crop_w, int crop_h, float* dst, int dst_cs, int dst_c0) {
    T2V_REQUIRE(ctx && src && x_first && x_count && x_coef && y_first && y_count && y_coef && dst,
                "resample_crop_normalize_u8: null pointer");
    T2V_REQUIRE(T >= 1 && T <= 65535, "resample_crop_normalize_u8: T must be in 1..65535 (got %d)", T);
    T2V_REQUIRE(h >= 1 && w >= 1 && out_w >= 1 && out_h >= 1, "resample_crop_normalize_u8: empty frame");
    T2V_REQUIRE(kx >= 1 && ky >= 1 && kx <= resample_max_taps() && ky <= resample_max_taps(),
                "resample_crop_normalize_u8: %d x %d taps, the limit is %d (resize on the CPU)", kx, ky, resample_max_taps());
    T2V_REQUIRE(crop_w >= 1 && crop_h >= 1 && crop_x >= 0 && crop_y >= 0 && crop_x <= out_w - crop_w && crop_y <= out_h - crop_h,
                "resample_crop_normalize_u8: crop %dx%d at (%d, %d) outside the %dx%d resized image", crop_w, crop_h, crop_x,
                crop_y, out_w, out_h);
    T2V_REQUIRE(dst_c0 >= 0 && dst_c0 + 3 <= dst_cs, "resample_crop_normalize_u8: channels [c0, c0+3) outside the channel stride");
    return launch_resample_crop_normalize_u8((hipStream_t)stream, src, T, h, w, x_first, x_count, x_coef, kx, y_first, y_count,
                                             y_coef, ky, crop_x, crop_y, crop_w, crop_h, dst, dst_cs, dst_c0);
}

// ---- picture-quality sums: PSNR / SSIM of two uint8 images (additive to ABI 22) ----
static bool image_metrics_shape_ok(int H, int W, int nbox) {
    return H >= 1 && W >= 1 && H <= T2V_METRICS_MAX_SIDE && W <= T2V_METRICS_MAX_SIDE && nbox >= 0 && nbox <= T2V_METRICS_MAX_BOXES;
}
size_t t2v_image_metrics_scratch_doubles(int H, int W, int nbox) {
    return image_metrics_shape_ok(H, W, nbox) ? image_metrics_scratch_doubles(H, W, nbox) : 0;
}
int t2v_image_metrics_u8(t2v_ctx* ctx, void* stream, const uint8_t* a, int a_cs, const uint8_t* b, int b_cs, int H, int W,
                         const int32_t* boxes, int nbox, double* scratch, double* out) {
    T2V_REQUIRE(ctx && a && b && scratch && out, "image_metrics_u8: null pointer");
    T2V_REQUIRE((a_cs == 3 || a_cs == 4) && (b_cs == 3 || b_cs == 4),
                "image_metrics_u8: channel strides must be 3 or 4 (got %d and %d)", a_cs, b_cs);
    T2V_REQUIRE(H >= 1 && W >= 1 && H <= T2V_METRICS_MAX_SIDE && W <= T2V_METRICS_MAX_SIDE,
                "image_metrics_u8: H, W must be in 1..%d (got %d x %d)", T2V_METRICS_MAX_SIDE, H, W);
    T2V_REQUIRE(nbox >= 0 && nbox <= T2V_METRICS_MAX_BOXES, "image_metrics_u8: nbox must be in 0..%d (got %d)",
                T2V_METRICS_MAX_BOXES, nbox);
    T2V_REQUIRE(nbox == 0 || boxes, "image_metrics_u8: %d boxes and a null box pointer", nbox);
    for (int i = 0; i < nbox; ++i) {
        const int32_t* q = boxes + 4 * i;
        T2V_REQUIRE(q[0] >= 0 && q[0] < q[1] && q[1] <= H && q[2] >= 0 && q[2] < q[3] && q[3] <= W,
                    "image_metrics_u8: box %d = rows [%d, %d) x columns [%d, %d) is empty or outside the %d x %d frame", i, q[0],
                    q[1], q[2], q[3], H, W);
    }
    return launch_image_metrics_u8((hipStream_t)stream, a, a_cs, b, b_cs, H, W, boxes, nbox, scratch, out);
}

// ---- temporal-consistency sums of a generated pair against the real pair (additive to ABI 22) ----
size_t t2v_temporal_metrics_scratch_doubles(int H, int W, int nbox) {
    return image_metrics_shape_ok(H, W, nbox) ? temporal_metrics_scratch_doubles(H, W, nbox) : 0;
}
int t2v_temporal_metrics_u8(t2v_ctx* ctx, void* stream, const uint8_t* a_cur, int a_cur_cs, const uint8_t* a_prev, int a_prev_cs,
                            const uint8_t* b_cur, int b_cur_cs, const uint8_t* b_prev, int b_prev_cs, const float* flow_fwd,
                            const float* flow_bwd, const float* flow_a, int H, int W, const int32_t* boxes, int nbox,
                            double* scratch, double* out) {
    T2V_REQUIRE(ctx && a_cur && a_prev && b_cur && b_prev && flow_fwd && flow_bwd && scratch && out,
                "temporal_metrics_u8: null pointer");
    const int cs[4] = {a_cur_cs, a_prev_cs, b_cur_cs, b_prev_cs};
    for (int i = 0; i < 4; ++i)
        T2V_REQUIRE(cs[i] == 3 || cs[i] == 4, "temporal_metrics_u8: channel strides must be 3 or 4 (got %d, %d, %d, %d)", cs[0],
                    cs[1], cs[2], cs[3]);
    T2V_REQUIRE(H >= 1 && W >= 1 && H <= T2V_METRICS_MAX_SIDE && W <= T2V_METRICS_MAX_SIDE,
                "temporal_metrics_u8: H, W must be in 1..%d (got %d x %d)", T2V_METRICS_MAX_SIDE, H, W);
    T2V_REQUIRE(nbox >= 0 && nbox <= T2V_METRICS_MAX_BOXES, "temporal_metrics_u8: nbox must be in 0..%d (got %d)",
                T2V_METRICS_MAX_BOXES, nbox);
    T2V_REQUIRE(nbox == 0 || boxes, "temporal_metrics_u8: %d boxes and a null box pointer", nbox);
    for (int i = 0; i < nbox; ++i) {
        const int32_t* q = boxes + 4 * i;
        T2V_REQUIRE(q[0] >= 0 && q[0] < q[1] && q[1] <= H && q[2] >= 0 && q[2] < q[3] && q[3] <= W,
                    "temporal_metrics_u8: box %d = rows [%d, %d) x columns [%d, %d) is empty or outside the %d x %d frame", i,
                    q[0], q[1], q[2], q[3], H, W);
    }
    return launch_temporal_metrics_u8((hipStream_t)stream, a_cur, a_cur_cs, a_prev, a_prev_cs, b_cur, b_cur_cs, b_prev, b_prev_cs,
                                      flow_fwd, flow_bwd, flow_a, H, W, boxes, nbox, scratch, out);
}

// ---- training visuals: image / unit-map / flow panels of one frame as uint8 RGB (additive to ABI 22) ----
static bool train_visuals_shape_ok(int H, int W, int npanels) {
    return H >= 1 && W >= 1 && H <= T2V_METRICS_MAX_SIDE && W <= T2V_METRICS_MAX_SIDE && npanels >= 1 &&
           npanels <= T2V_VISUALS_MAX_PANELS;
}
size_t t2v_train_visuals_scratch_doubles(int H, int W, int npanels) {
    return train_visuals_shape_ok(H, W, npanels) ? train_visuals_scratch_doubles(H, W, npanels) : 0;
}
int t2v_train_visuals_u8(t2v_ctx* ctx, void* stream, const float* const* panel_ptrs, const int32_t* panel_ints, int npanels,
                         int H, int W, int scale, double* scratch, size_t scratch_doubles, uint8_t* out) {
    T2V_REQUIRE(ctx && panel_ptrs && panel_ints && scratch && out, "train_visuals_u8: null pointer");
    T2V_REQUIRE(npanels >= 1 && npanels <= T2V_VISUALS_MAX_PANELS, "train_visuals_u8: npanels must be in 1..%d (got %d)",
                T2V_VISUALS_MAX_PANELS, npanels);
    T2V_REQUIRE(H >= 1 && W >= 1 && H <= T2V_METRICS_MAX_SIDE && W <= T2V_METRICS_MAX_SIDE,
                "train_visuals_u8: H, W must be in 1..%d (got %d x %d)", T2V_METRICS_MAX_SIDE, H, W);
    T2V_REQUIRE(scale == 1 || scale == 2 || scale == 4, "train_visuals_u8: scale must be 1, 2 or 4 (got %d)", scale);
    T2V_REQUIRE(H % scale == 0 && W % scale == 0, "train_visuals_u8: scale %d does not divide %d x %d", scale, H, W);
    for (int i = 0; i < npanels; ++i) {
        const int kind = panel_ints[3 * i], c0 = panel_ints[3 * i + 1], cs = panel_ints[3 * i + 2];
        T2V_REQUIRE(panel_ptrs[i], "train_visuals_u8: panel %d is a null pointer", i);
        T2V_REQUIRE(kind == T2V_VISUALS_IMAGE || kind == T2V_VISUALS_UNIT || kind == T2V_VISUALS_FLOW,
                    "train_visuals_u8: panel %d has the unknown kind %d", i, kind);
        const int nc = kind == T2V_VISUALS_IMAGE ? 3 : (kind == T2V_VISUALS_FLOW ? 2 : 1);
        T2V_REQUIRE(c0 >= 0 && cs >= 1 && c0 <= cs - nc, "train_visuals_u8: panel %d reads channels [%d, %d) of %d", i, c0,
                    c0 + nc, cs);
    }
    T2V_REQUIRE((uintptr_t)out % 4 == 0, "train_visuals_u8: out must be 4-byte aligned");
    T2V_REQUIRE(scratch_doubles >= train_visuals_scratch_doubles(H, W, npanels),
                "train_visuals_u8: scratch holds %zu doubles, %d panels of %d x %d need %zu", scratch_doubles, npanels, H, W,
                train_visuals_scratch_doubles(H, W, npanels));
    return launch_train_visuals_u8((hipStream_t)stream, panel_ptrs, panel_ints, npanels, H, W, scale, scratch, out);
}

// ---- host plumbing (ABI 14): buffers, copies, streams, events for a host without a HIP binding of its own ----
int t2v_device_malloc(t2v_ctx* ctx, size_t bytes, void** out) {
    T2V_REQUIRE(ctx && out, "device_malloc: null pointer");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    *out = nullptr;
    if (bytes == 0) return T2V_OK;
    T2V_HIP_CHECK(hipMalloc(out, bytes));
    return T2V_OK;
}
int t2v_device_free(t2v_ctx* ctx, void* ptr) {
    T2V_REQUIRE(ctx, "device_free: null context");
    if (!ptr) return T2V_OK;
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    T2V_HIP_CHECK(hipFree(ptr));
    return T2V_OK;
}
int t2v_host_malloc(t2v_ctx* ctx, size_t bytes, void** out) {
    T2V_REQUIRE(ctx && out && bytes > 0, "host_malloc: bad arguments");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    T2V_HIP_CHECK(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return T2V_OK;
}
int t2v_host_free(t2v_ctx* ctx, void* ptr) {
    T2V_REQUIRE(ctx, "host_free: null context");
    if (!ptr) return T2V_OK;
    T2V_HIP_CHECK(hipHostFree(ptr));
    return T2V_OK;
}
int t2v_memcpy(t2v_ctx* ctx, void* stream, void* dst, const void* src, size_t bytes, int kind) {
    T2V_REQUIRE(ctx && (bytes == 0 || (dst && src)), "memcpy: null pointer");
    T2V_REQUIRE(kind == T2V_COPY_H2D || kind == T2V_COPY_D2H || kind == T2V_COPY_D2D, "memcpy: kind %d", kind);
    if (bytes == 0) return T2V_OK;
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipMemcpyKind k = kind == T2V_COPY_H2D ? hipMemcpyHostToDevice
                      : (kind == T2V_COPY_D2H ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice);
    T2V_HIP_CHECK(hipMemcpyAsync(dst, src, bytes, k, (hipStream_t)stream));
    return T2V_OK;
}
int t2v_stream_create(t2v_ctx* ctx, void** out) {
    T2V_REQUIRE(ctx && out, "stream_create: null pointer");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipStream_t s = nullptr;
    T2V_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return T2V_OK;
}
int t2v_stream_destroy(t2v_ctx* ctx, void* stream) {
    T2V_REQUIRE(ctx, "stream_destroy: null context");
    if (stream) T2V_HIP_CHECK(hipStreamDestroy((hipStream_t)stream));
    return T2V_OK;
}
int t2v_stream_synchronize(t2v_ctx* ctx, void* stream) {
    T2V_REQUIRE(ctx, "stream_synchronize: null context");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    T2V_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return T2V_OK;
}
int t2v_event_create(t2v_ctx* ctx, void** out) {
    T2V_REQUIRE(ctx && out, "event_create: null pointer");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    hipEvent_t e = nullptr;
    T2V_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    *out = e;
    return T2V_OK;
}
int t2v_event_record(t2v_ctx* ctx, void* event, void* stream) {
    T2V_REQUIRE(ctx && event, "event_record: null pointer");
    T2V_HIP_CHECK(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
    return T2V_OK;
}
int t2v_event_synchronize(t2v_ctx* ctx, void* event) {
    T2V_REQUIRE(ctx && event, "event_synchronize: null pointer");
    T2V_HIP_CHECK(hipEventSynchronize((hipEvent_t)event));
    return T2V_OK;
}
int t2v_event_destroy(t2v_ctx* ctx, void* event) {
    T2V_REQUIRE(ctx, "event_destroy: null context");
    if (event) T2V_HIP_CHECK(hipEventDestroy((hipEvent_t)event));
    return T2V_OK;
}
int t2v_device_synchronize(t2v_ctx* ctx) {
    T2V_REQUIRE(ctx, "device_synchronize: null context");
    T2V_HIP_CHECK(hipSetDevice(ctx->device));
    T2V_HIP_CHECK(hipDeviceSynchronize());
    return T2V_OK;
}

}  // extern "C"
