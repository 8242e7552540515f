// generator.hip -- whole-frame orchestration of the vid2vid generators on one HIP stream.
//
// Replaces CompositeGenerator.forward / CompositeLocalGenerator.forward (SURVEY.md App. A.1/A.2;
// section 8a rows a4, a13).  Pure launch sequencing: every tensor lives in the caller's
// workspace (bump-allocated here, identically by t2v_generator_workspace_bytes), nothing
// synchronises, so a frame is ~150 back-to-back launches on the caller's stream.
//
// Norms applied by their consumers: a producer that next_takes_raw() allows (and a lazy ResnetBlock chain) leaves its conv
// output raw and returns a Pending value -- the layer whose gamma / beta apply, the scratch set holding its (mean, rstd), relu,
// a residual.  The next conv_norm / head / export_feat / the encoder join takes that value; lazy_norm() and join_side() turn it
// into what the kernels read, discharge() runs the apply pass where no consumer does.
#include <algorithm>
#include <vector>

#include "conv_plan.h"

namespace t2v {
namespace {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct Arena {
    char* base;
    size_t cap;
    size_t off = 0;
    bool overflow = false;
    float* alloc(size_t floats) {
        const size_t bytes = (floats * sizeof(float) + 255) / 256 * 256;
        float* p = reinterpret_cast<float*>(base + off);
        off += bytes;
        if (base && off > cap) overflow = true;
        return p;
    }
};

t2v_conv_desc mk_conv(int H, int W, int Cin, int Cout, int k, int stride, int pad, int pad_mode, int transposed,
                      int act = T2V_ACT_NONE, float act_scale = 1.f) {
    t2v_conv_desc d;
    d.H = H; d.W = W; d.Cin = Cin; d.Cout = Cout; d.kH = k; d.kW = k; d.stride = stride; d.pad = pad;
    d.pad_mode = pad_mode; d.transposed = transposed; d.act = act; d.act_scale = act_scale;
    d.output_padding = transposed ? 1 : 0;
    d.algo = T2V_ALGO_DIRECT;
    return d;
}

struct LayerSpec {
    t2v_conv_desc cd;
    int x_cs;
    bool has_norm;
    long out_px() const {      // pixels of the output map (the transposed layers: k3, s2, p1, output_padding 1)
        if (cd.transposed) return 4L * cd.H * cd.W;
        return (long)((cd.H + 2 * cd.pad - cd.kH) / cd.stride + 1) * ((cd.W + 2 * cd.pad - cd.kW) / cd.stride + 1);
    }
};

// conv_algo 3 | 4 | 5: the selection of 0 in the opt-in split-bf16 arithmetic, 3 on the trunk, 4 on the polyphase stride-2 layers
// as well, 5 also on the stride-2 layers that stay direct
inline bool split_mode(const t2v_gen_desc& g) { return g.conv_algo >= 3 && g.conv_algo <= 5; }
// a stride-2 / transposed 3x3 layer: polyphase F(4,2) where that is the faster form, with conv_algo 4 in split-bf16 arithmetic
// where that form takes the layer.  Every class polyphase_pays selects measured faster split than fp32 as a whole conv, ranges
// apart (scripts/measure_split_bf16_stride2.py, MI355X, profiles/split_bf16_stride2_times.txt): 256->512 @256x256 251.6 -> 192.8 us
// (the shortest ring run, K = 256), 512->1024 @128x128 221.0 -> 136.9, 1024->512 (transposed) @64x64 214.4 -> 133.2, 512->256
// (transposed) @128x128 250.2 -> 198.1; 512<->1024 at 512x320 148.9 -> 115.2 / 141.3 -> 111.8, at 512x680 290.1 -> 177.1 /
// 292.3 -> 185.5: no class is excluded
// conv_algo 5: a layer that stays direct (polyphase_pays says no) runs as T2V_ALGO_DIRECT_BF16X2 where that form takes it AND
// its class was measured: both channel counts >= 128, i.e. the 128 <-> 256 layers of the ngf-128 generators (and the same
// class reached from ngf 64 one level down).  Narrower layers that the predicate accepts (64 -> 128: 288 one-per-CU tiles with
// K = 576 at 384x384, where the fp32 plan takes 64x64 tiles) were not measured and stay fp32.  Every measured class is faster as apply pass + whole conv, ranges apart (scripts/measure_split_bf16_outer.py, MI355X,
// profiles/split_bf16_outer_times.txt; fp32 -> split, us): 128->256 @512x512 330.5 -> 168.6, 256->128 (transposed) @256x256
// 317.3 -> 176.8; at 512x320 212.1 -> 113.3 / 211.3 -> 109.2, at 512x680 482.7 -> 240.4 / 438.5 -> 230.9, at 1024x1024
// 1339.7 -> 693.5 / 1255.0 -> 706.8 (the same layers forced to T2V_ALGO_POLYPHASE_BF16X2: 307.1 / 317.4 @512x512): no measured
// class is excluded.
// pairs_ok: the layer's input is a map only this layer reads, so the norm apply pass in front of it may store the pair layout
// of T2V_ALGO_DIRECT_BF16X2 in place (encoder maps and decoder maps between two layers; a decoder's first layer only behind a
// ResnetBlock chain, whose output is the branch's own -- without one it reads the encoder sum both branches share)
int stride2_algo(const t2v_gen_desc& g, const t2v_conv_desc& cd, int x_cs, bool pairs_ok) {
    if (!(g.conv_algo == 0 || split_mode(g))) return T2V_ALGO_DIRECT;
    if (!polyphase_pays(&cd, x_cs))
        return g.conv_algo == 5 && pairs_ok && cd.Cin >= 128 && cd.Cout >= 128 && direct_split_supported(&cd, x_cs) ? T2V_ALGO_DIRECT_BF16X2
                                                                                                                 : T2V_ALGO_DIRECT;
    return g.conv_algo >= 4 && polyphase_split_supported(&cd, x_cs) ? T2V_ALGO_POLYPHASE_BF16X2 : T2V_ALGO_POLYPHASE;
}

// canonical layer list (the order documented in t2v.h)
void enumerate_layers(const t2v_gen_desc& g, std::vector<LayerSpec>& out) {
    const int G = g.ngf, n = g.is_local ? 1 : g.n_downsample;
    const int H = g.H, W = g.W;
    auto enc = [&](int in_nc) {
        out.push_back({mk_conv(H, W, in_nc, G, 7, 1, 3, T2V_PAD_REFLECT, 0), round_up(in_nc, 4), true});
        for (int i = 0; i < n; ++i) {
            t2v_conv_desc cd = mk_conv(H >> i, W >> i, G << i, G << (i + 1), 3, 2, 1, T2V_PAD_ZERO, 0);
            // the deep stride-2 layers as polyphase Winograd F(4,2) (polyphase.hip) where that is the faster form
            cd.algo = stride2_algo(g, cd, G << i, true);
            out.push_back({cd, G << i, true});
        }
    };
    auto rbs = [&](int count) {
        const int C = G << n;
        t2v_conv_desc cd = mk_conv(H >> n, W >> n, C, C, 3, 1, 1, T2V_PAD_REFLECT, 0);
        // the ResnetBlock convs (84 % of the FLOPs) run as Winograd F(2x2,3x3) wherever the geometry allows
        // conv_algo 3 | 4: the selection of 0, its F(4x4,3x3) layers in split-bf16 arithmetic where that form takes them
        cd.algo = best_conv_algo(&cd, C, split_mode(g) ? 0 : g.conv_algo);
        if (split_mode(g) && cd.algo == T2V_ALGO_WINOGRAD_F4 && winograd_supported(&cd, C, T2V_ALGO_WINOGRAD_F4_BF16X2))
            cd.algo = T2V_ALGO_WINOGRAD_F4_BF16X2;
        for (int i = 0; i < 2 * count; ++i) out.push_back({cd, C, true});
    };
    const int nb_enc = g.is_local ? 0 : g.n_blocks - g.n_blocks / 2;
    const int nb_res = g.is_local ? g.n_blocks : g.n_blocks / 2;
    auto ups = [&]() {
        for (int i = 0; i < n; ++i) {
            const int l = n - i;
            t2v_conv_desc cd = mk_conv(H >> l, W >> l, G << l, G << (l - 1), 3, 2, 1, T2V_PAD_ZERO, 1);
            cd.algo = stride2_algo(g, cd, G << l, i > 0 || nb_res > 0);
            out.push_back({cd, G << l, true});
        }
    };
    enc(g.input_nc); rbs(nb_enc);
    enc(g.prev_nc);  rbs(nb_enc);
    rbs(nb_res); ups();
    out.push_back({mk_conv(H, W, G, g.output_nc, 7, 1, 3, T2V_PAD_REFLECT, 0, T2V_ACT_TANH), G, false});
    if (!g.no_flow) {
        rbs(nb_res); ups();
        out.push_back({mk_conv(H, W, G, 3, 7, 1, 3, T2V_PAD_REFLECT, 0, T2V_ACT_FLOW_W, g.flow_multiplier), G, false});
    }
}

int check_desc(const t2v_gen_desc* g) {
    T2V_REQUIRE(g, "null generator descriptor");
    const int n = g->is_local ? 1 : g->n_downsample;
    T2V_REQUIRE(g->ngf > 0 && g->ngf % 4 == 0, "ngf=%d must be a positive multiple of 4", g->ngf);
    T2V_REQUIRE(n >= 1 && n <= 6, "n_downsample=%d out of range", n);
    T2V_REQUIRE(g->H > 0 && g->W > 0 && g->H % (1 << n) == 0 && g->W % (1 << n) == 0,
                "H=%d W=%d must be positive multiples of %d", g->H, g->W, 1 << n);
    T2V_REQUIRE((g->H >> n) >= 2 && (g->W >> n) >= 2, "bottleneck %dx%d too small for reflection pad 1", g->H >> n,
                g->W >> n);
    T2V_REQUIRE(g->output_nc == 3, "output_nc=%d: only RGB output is on the path", g->output_nc);
    T2V_REQUIRE(g->input_nc > 0 && g->prev_nc >= 3, "bad input_nc/prev_nc");
    T2V_REQUIRE(g->n_blocks >= 0, "bad n_blocks");
    return T2V_OK;
}

constexpr int kMaxBatch = T2V_MAX_BATCH;

// Every buffer holds the `nimg` images of a batch back to back (image stride = the single-image size), so the
// batched kernels of the ResnetBlock chains address image i at base + i*stride and the per-image launches of the
// other layers do the same.
struct Buffers {
    float *encA[8], *encB[8];  // encoder activations per level (A: pose/seg, B: prev-image)
    float* bt[4];              // bottleneck temporaries (resnet chains)
    float* bt2[4];             // ... of the branch that runs on the side stream
    float* d;                  // encoder sum
    float* vshare;             // flow frames of the global generator: the F(4x4) input transform V of d, made once for both branches
    float *dimg, *dflow;       // local generator: d + coarse features
    float *decI[8], *decF[8];  // decoder activations per level
    float *raw, *fw;
    size_t lvl[8];             // floats of one image at level l
    size_t bott;               // = lvl[n]
    // per-stream scratch [0]: caller's stream, [1]: side stream; one slot per image
    float* stats[2];
    float* mean_rstd[2];
    float* wino[2];   // Winograd scratch: transformed input V + transformed output M of the whole batch
    double* fin[2];   // norm finalize scratch (pooled moments per group of partials)
    size_t stats_stride, mr_stride, fin_stride;   // floats (doubles for fin) between the images' slots
};

void plan_buffers(const t2v_gen_desc& g, const std::vector<LayerSpec>& layers, int nimg, Arena& a, Buffers& b) {
    const int G = g.ngf, n = g.is_local ? 1 : g.n_downsample;
    auto lvl = [&](int l) { return (size_t)(g.H >> l) * (g.W >> l) * (G << l); };
    const size_t N = (size_t)nimg;
    for (int l = 0; l <= n; ++l) {
        b.lvl[l] = lvl(l);
        b.encA[l] = a.alloc(N * lvl(l));
        b.encB[l] = a.alloc(N * lvl(l));
    }
    b.bott = lvl(n);
    for (int i = 0; i < 4; ++i) b.bt[i] = a.alloc(N * lvl(n));
    for (int i = 0; i < 4; ++i) b.bt2[i] = a.alloc(N * lvl(n));
    b.d = a.alloc(N * lvl(n));
    {   // the first conv of the image branch and of the flow branch read the same map d: one V, kept until both GEMMs are done
        // (a slot of its own: the streams' own workspaces are overwritten by the branches' next convs)
        const bool flow_global = !g.no_flow && !g.is_local && g.n_blocks / 2 > 0;
        b.vshare = nullptr;
        if (flow_global) {
            const LayerSpec& L = layers[2 * (1 + n + 2 * (g.n_blocks - g.n_blocks / 2))];      // the branches' first conv
            if (is_f4(L.cd.algo))
                b.vshare = a.alloc((size_t)wino_pos(L.cd.algo) * wino_rows_batch(&L.cd, L.cd.algo, nimg) * L.cd.Cin);
        }
    }
    b.dimg = a.alloc(N * lvl(n));
    b.dflow = a.alloc(N * lvl(n));
    for (int l = 0; l < n; ++l) {
        b.decI[l] = a.alloc(N * lvl(l));
        b.decF[l] = g.no_flow ? nullptr : a.alloc(N * lvl(l));
    }
    b.raw = a.alloc(N * g.H * g.W * 4);
    b.fw = a.alloc(N * g.H * g.W * 4);
    size_t max_stats = 0;
    int max_c = 4;
    for (const LayerSpec& L : layers) {
        if (L.has_norm) max_stats = std::max(max_stats, norm_partial_floats(&L.cd, L.x_cs));
        if (L.cd.Cout > max_c) max_c = L.cd.Cout;
    }
    b.stats_stride = (max_stats + 63) / 64 * 64;
    b.mr_stride = (size_t)max_c * 2;
    b.fin_stride = (size_t)kFinalizeMaxGroups * max_c * 4;
    for (int k = 0; k < 2; ++k) {
        b.stats[k] = a.alloc(N * b.stats_stride);
        b.mean_rstd[k] = a.alloc(N * b.mr_stride);
        b.fin[k] = reinterpret_cast<double*>(a.alloc(N * b.fin_stride * 2));
    }
    size_t max_wino = 0;
    for (const LayerSpec& L : layers)
        if (is_winograd(L.cd.algo)) {
            const size_t w = winograd_workspace_floats(&L.cd, is_f4(L.cd.algo) ? nimg : 1);
            if (w > max_wino) max_wino = w;
        } else if (is_poly(L.cd.algo)) {
            const size_t w = polyphase_workspace_floats(&L.cd);
            if (w > max_wino) max_wino = w;
        }
    for (int k = 0; k < 2; ++k) b.wino[k] = max_wino ? a.alloc(max_wino) : nullptr;
}

// the images of a batch as pointers (maps that are not laid out back to back: the caller's inputs and outputs)
struct Ptrs {
    const float* p[kMaxBatch];
};
struct MutPtrs {
    float* p[kMaxBatch];
    operator Ptrs() const {
        Ptrs q;
        for (int i = 0; i < kMaxBatch; ++i) q.p[i] = p[i];
        return q;
    }
};

// A raw conv output whose norm is still owed: the consumer (or discharge()) applies y = [relu](norm(x)) + res.  Nothing is
// owed while layer < 0.  One value per batch: the images' (mean, rstd) tables sit mr_stride apart in scratch set `sc` until
// that set's next finalize replaces them, a residual is the batch's bottleneck maps back to back.
struct Pending {
    int layer = -1;              // the layer whose statistics and gamma / beta apply
    int sc = 0;                  // scratch set of the (mean, rstd) tables
    int relu = 0;
    const float* res = nullptr;
    explicit operator bool() const { return layer >= 0; }
};
// what applies a pending norm: the forms that may carry one, and the rest
enum class Takes { Applied, Polyphase, Head7x7, ChainF4 };

struct Runner {
    t2v_ctx* ctx;
    hipStream_t s;
    const t2v_gen_desc& g;
    const std::vector<LayerSpec>& specs;
    const t2v_layer* layers;
    Buffers& b;
    int nimg;
    int li = 0;
    int sc = 0;   // which per-stream scratch set this runner uses

    Ptrs at(const float* base, size_t stride) const {
        Ptrs q{};
        for (int i = 0; i < nimg; ++i) q.p[i] = base ? base + (size_t)i * stride : nullptr;
        return q;
    }
    MutPtrs at(float* base, size_t stride) const {
        MutPtrs q{};
        for (int i = 0; i < nimg; ++i) q.p[i] = base ? base + (size_t)i * stride : nullptr;
        return q;
    }
    float* stats_of(int im) const { return b.stats[sc] + (size_t)im * b.stats_stride; }
    float* mr_of(int im) const { return b.mean_rstd[sc] + (size_t)im * b.mr_stride; }
    double* fin_of(int im) const { return b.fin[sc] + (size_t)im * b.fin_stride; }

    // the norm `p` owes the maps y, from image `im` on, as the join kernel takes it
    NormJoinSide join_side(const Pending& p, int im, const float* y) const {
        const t2v_layer& w = layers[p.layer];
        return {y, b.mean_rstd[p.sc] + (size_t)im * b.mr_stride, g.norm_affine ? w.gamma : nullptr,
                g.norm_affine ? w.beta : nullptr, p.res ? p.res + (size_t)im * b.bott : nullptr};
    }
    // ... and as the input side of a consumer of form `by` takes it (xout: LazyNorm's side output, the chain only)
    int lazy_norm(const Pending& p, int im, Takes by, float* xout, LazyNorm* out) const {
        T2V_REQUIRE(by != Takes::Applied,
                    "internal: only the polyphase input transform, the halo-tile head and a chain's F(4x4) input transform apply a pending norm");
        if (by == Takes::ChainF4) {
            T2V_REQUIRE(b.mr_stride == (size_t)2 * specs[p.layer].cd.Cout, "internal: chain scratch layout");
            T2V_REQUIRE((p.relu == 0 || p.relu == 1) && (p.res != nullptr) == (xout != nullptr) && !(p.res && p.relu),
                        "internal: a chain's pending norm is norm + ReLU, or norm + residual with the sum written on the side");
        } else {
            T2V_REQUIRE(p.relu == 1 && !p.res && !xout, "internal: a lazy output carries a plain norm + ReLU");
        }
        const NormJoinSide n = join_side(p, im, nullptr);
        *out = LazyNorm{n.mean_rstd, n.gamma, n.beta, p.relu, n.res, xout};
        return T2V_OK;
    }
    // the apply pass that nobody took over: dst = [relu](norm(src)) + res for `count` images from image `im` on
    // pairs: dst receives the pair layout a T2V_ALGO_DIRECT_BF16X2 layer reads (the split store of the same pass)
    int discharge(const Pending& p, int im, int count, const float* src, float* dst, bool pairs = false) const {
        const LayerSpec& L = specs[p.layer];
        T2V_REQUIRE(count == 1 || b.mr_stride == (size_t)2 * L.cd.Cout, "internal: chain scratch layout");
        const NormJoinSide n = join_side(p, im, src);
        if (pairs) return launch_inorm_apply_split(s, n.y, n.mean_rstd, n.gamma, n.beta, n.res, dst, L.out_px(), L.cd.Cout, p.relu, count);
        return launch_inorm_apply(s, n.y, n.mean_rstd, n.gamma, n.beta, n.res, nullptr, dst, L.out_px(), L.cd.Cout, p.relu, count);
    }
    // layer l runs as T2V_ALGO_DIRECT_BF16X2: the pass that writes its input stores the pair layout
    bool reads_pairs(int l) const { return l < (int)specs.size() && is_direct_split(specs[l].cd.algo); }

    // conv (+ fused stats) -> finalize of layer `own.layer` for ONE image; y receives the conv output.  `in`: the norm x still
    // owes -- this (polyphase) layer's input transform applies it.  defer: leave y raw and `own` to the next layer (no apply
    // pass: a read and a write of the map less), else y is normalised in place.  Same arithmetic in the same order: the frames
    // are bit-identical to the apply form (T2V_CHAIN_LAZY=0).
    // x_pairs: x is in the pair layout (this layer is T2V_ALGO_DIRECT_BF16X2); y_pairs: the apply pass stores y in it
    int conv_norm_one(int im, const float* x, const Pending& in, float* y, const Pending& own, bool defer, bool x_pairs, bool y_pairs) {
        const LayerSpec& L = specs[own.layer];
        const t2v_layer& w = layers[own.layer];
        float* stats = stats_of(im);
        if (g.norm_affine) T2V_REQUIRE(w.gamma && w.beta, "layer %d: norm_affine=1 but gamma/beta missing", own.layer);
        const bool poly = is_poly(L.cd.algo);
        T2V_REQUIRE(x_pairs == is_direct_split(L.cd.algo) && !(defer && y_pairs),
                    "internal: layer %d: the pair layout goes to the split-bf16 direct layers, from an apply pass", own.layer);
        LazyNorm ln;
        if (in) T2V_TRY(lazy_norm(in, im, poly ? Takes::Polyphase : Takes::Applied, nullptr, &ln));
        ConvPlan pl;
        const ConvPlan* plan = nullptr;
        if (is_winograd(L.cd.algo)) {
            T2V_REQUIRE(!defer, "internal: a Winograd layer outside a chain leaves an applied norm");
            T2V_TRY(winograd_forward(ctx, s, &L.cd, x, w.w, w.bias, y, stats, b.wino[sc], 7));
        } else if (poly) {
            T2V_TRY(polyphase_forward(ctx, s, &L.cd, x, w.w, w.bias, y, stats, b.wino[sc], 7, in ? &ln : nullptr));
        } else if (is_direct_split(L.cd.algo)) {
            T2V_TRY(direct_split_forward(s, &L.cd, x, w.w, w.bias, y, stats));
        } else {
            T2V_TRY(build_conv_plan(&L.cd, L.x_cs, true, &pl));
            T2V_TRY(run_conv(ctx, s, pl, x, w.w, w.bias, y, L.cd.Cout, stats));
            plan = &pl;
        }
        T2V_TRY(finalize_norm(s, &L.cd, L.x_cs, stats, 1, g.eps, mr_of(im), fin_of(im), nullptr, plan));
        return defer ? T2V_OK : discharge(own, im, 1, y, y, y_pairs);
    }
    // the next layer for every image of the batch (one launch sequence per image): y = [relu](norm(conv(x))) + res, or with
    // `defer` the raw conv output and that norm in *owed.  (The images of a lock-step batch as
    // blockIdx.y of ONE launch of the stride-2 / transposed convs -- run_conv_batch, what the train step's discriminators
    // use -- was measured here and dropped: 142.1 / 141.9 vs 142.1 / 141.7 fps for two 512x320 sequences, 67.0 / 66.7 vs
    // 66.8 / 66.7 at 512x680, 92.0 / 92.0 vs 91.8 / 91.7 at 512x512, alternating runs: inside two-stream frames the other
    // stream already fills what a 2.5-blocks-per-CU launch leaves idle.)
    int conv_norm(const Ptrs& x, Pending in, const MutPtrs& y, int relu, const float* res, bool defer = false,
                  Pending* owed = nullptr, bool x_pairs = false, bool y_pairs = false) {
        const Pending own{li, sc, relu, res};
        for (int im = 0; im < nimg; ++im) T2V_TRY(conv_norm_one(im, x.p[im], in, y.p[im], own, defer, x_pairs, y_pairs));
        ++li;
        if (owed) *owed = defer ? own : Pending{};
        return T2V_OK;
    }
    // the layer after the current one consumes this one's output, nothing else does, and it applies a pending norm itself:
    // a polyphase layer (in its input transform), or a 7x7 head on the halo-tile kernel (on its halo planes in LDS)
    bool next_takes_raw() const {
        if (!options().chain_lazy) return false;
        const LayerSpec& nx = specs[li + 1];
        if (is_poly(nx.cd.algo)) return true;
        ConvPlan pl;
        return !nx.has_norm && build_conv_plan(&nx.cd, nx.x_cs, false, &pl) == T2V_OK && conv_plan_is_head7x7(pl);
    }

    // in: the norm the last decoder layer left to the head
    int head(const Ptrs& x, const Pending& in, const MutPtrs& y) {
        const LayerSpec& L = specs[li];
        const t2v_layer& w = layers[li];
        ++li;
        ConvPlan pl;
        T2V_TRY(build_conv_plan(&L.cd, L.x_cs, false, &pl));
        for (int im = 0; im < nimg; ++im) {
            if (in) {
                LazyNorm ln;
                T2V_TRY(lazy_norm(in, im, Takes::Head7x7, nullptr, &ln));
                T2V_TRY(run_head7x7(s, pl, x.p[im], w.w, w.bias, y.p[im], 4, &ln));
            } else {
                T2V_TRY(run_conv(ctx, s, pl, x.p[im], w.w, w.bias, y.p[im], 4, nullptr));
            }
        }
        return T2V_OK;
    }
    // The feature map a caller asked for (the two-scale path's img_feat / flow_feat; `stride` floats each): a copy of the
    // decoder output, or, where the decoder left its norm to the head, the apply pass the decoder skipped, written into the
    // caller's buffer (the same traffic as the copy).
    int export_feat(const float* feat, size_t stride, const Pending& in, float* const* dst) {
        for (int im = 0; im < nimg; ++im) {
            if (!dst[im]) continue;
            if (in)
                T2V_TRY(discharge(in, im, 1, feat + im * stride, dst[im]));
            else
                T2V_HIP_CHECK(hipMemcpyAsync(dst[im], feat + im * stride, stride * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        return T2V_OK;
    }

    // x + [pad1,conv3,N,ReLU,pad1,conv3,N](x), image by image
    int resblock(const float* x, float* t, float* y, bool y_pairs) {
        T2V_TRY(conv_norm(at(x, b.bott), Pending{}, at(t, b.bott), 1, nullptr));
        return conv_norm(at(t, b.bott), Pending{}, at(y, b.bott), 0, x, false, nullptr, false, y_pairs);
    }

    // One F(4x4) Winograd conv of a chain over the whole batch (maps `bott` floats apart), up to and including the
    // finalize of its norm statistics; the norm itself, [relu](norm(y_raw)) + res, is left to the consumer as *owed.
    // `in` is the norm the INPUT still owes: the previous conv's, whose (mean, rstd) tables are in mean_rstd[sc] until this
    // conv's finalize replaces them; xout as in LazyNorm.
    // v_in (nothing owed only): the V of x that share_v() made; the input transform is left out
    int wino4_conv_stats(const float* x, const Pending& in, float* xout, float* y_raw, int relu, const float* res, Pending* owed,
                         const float* v_in = nullptr) {
        const LayerSpec& L = specs[li];
        const t2v_layer& w = layers[li];
        *owed = Pending{li, sc, relu, res};
        ++li;
        const t2v_conv_desc& cd = L.cd;
        if (g.norm_affine) T2V_REQUIRE(w.gamma && w.beta, "layer %d: norm_affine=1 but gamma/beta missing", owed->layer);
        LazyNorm ln;
        if (in) T2V_TRY(lazy_norm(in, 0, Takes::ChainF4, xout, &ln));
        WinoBatch wb;
        wb.nimg = nimg;
        wb.img_stride_x = (long)b.bott;
        wb.lazy = in ? &ln : nullptr;
        wb.v_in = in ? nullptr : v_in;
        // the images' partials are packed back to back by the batched output transform
        T2V_TRY(winograd_forward(ctx, s, &cd, x, w.w, w.bias, y_raw, b.stats[sc], b.wino[sc], wb.v_in ? 6 : 7, &wb));
        const size_t per_img = norm_partial_floats(&cd, L.x_cs);
        for (int im = 0; im < nimg; ++im)
            T2V_TRY(finalize_norm(s, &cd, L.x_cs, b.stats[sc] + im * per_img, 1, g.eps, mr_of(im), fin_of(im)));
        return T2V_OK;
    }

    // The same chain with every norm applied by its consumer: the next conv's input transform normalises (and adds
    // the residual) on the fly, and writes the block output the following block needs as ITS residual on the side.
    // Only the last norm of the chain runs as an apply pass.  Per block: 8 launches instead of 10 for the WHOLE batch, and one read + one write of the map less
    // per conv.  tmp: raw conv1 / conv2 outputs, block outputs (alternating); all hold the batch back to back.
    // defer: the last norm is left to the caller as well (the encoder join applies both encoders' in one pass);
    // v0: V of x, made by share_v()
    int res_chain_lazy(const float* x, int count, float* tmp[4], const float** out, bool defer, Pending* owed, const float* v0,
                       bool out_pairs) {
        const float* cur = x;
        Pending end;      // what the conv output waiting in tmp[1] owes: its norm + the block input `cur`
        for (int i = 0; i < count; ++i) {
            float* xi = i ? tmp[2 + (i & 1)] : nullptr;      // block i's input, written on the side by its first transform
            Pending mid;
            T2V_TRY(wino4_conv_stats(i ? tmp[1] : x, end, xi, tmp[0], 1, nullptr, &mid, i ? nullptr : v0));
            if (i) cur = xi;
            T2V_TRY(wino4_conv_stats(tmp[0], mid, nullptr, tmp[1], 0, cur, &end));
        }
        *out = tmp[1];
        *owed = defer ? end : Pending{};
        return defer ? T2V_OK : discharge(end, 0, nimg, tmp[1], tmp[1], out_pairs);
    }

    // a chain of `count` blocks starting at layer l takes the lazy form
    bool chain_is_lazy(int l, int count) const {
        return options().chain_lazy && count > 0 && is_f4(specs[l].cd.algo) && b.mr_stride == (size_t)2 * specs[l].cd.Cout;
    }
    // V of the map the chain at layer l starts from (the batch back to back), into the shared slot
    int share_v(int l, const float* x) {
        const t2v_conv_desc& cd = specs[l].cd;
        return launch_winograd4_input(s, x, b.vshare, cd.H, cd.W, cd.Cin, cd.pad, cd.pad_mode == T2V_PAD_REFLECT, nimg, 0, nimg,
                                      (long)b.bott, nullptr, is_split(cd.algo));
    }
    // chain of `count` resblocks starting from x (never written; the batch back to back, `bott` floats apart); result
    // pointer in *out, the norm it still owes (with `defer`, the lazy chain only) in *owed.  tmp: 4 distinct buffers != x.
    // out_pairs: the chain's output (count > 0: a buffer of tmp, read by the decoder's first layer alone) in the pair layout
    int res_chain(const float* x, int count, float* tmp[4], const float** out, bool defer, Pending* owed, const float* v0 = nullptr,
                  bool out_pairs = false) {
        T2V_REQUIRE(!out_pairs || (count > 0 && !defer), "internal: the pair layout is stored by a chain's own closing apply pass");
        if (chain_is_lazy(li, count)) return res_chain_lazy(x, count, tmp, out, defer, owed, v0, out_pairs);
        T2V_REQUIRE(!defer && !v0, "internal: only the lazy chain leaves its last norm pending / borrows a V");
        const float* cur = x;
        for (int i = 0; i < count; ++i) {
            float* y = (cur == tmp[1]) ? tmp[2] : tmp[1];
            T2V_TRY(resblock(cur, tmp[0], y, out_pairs && i + 1 == count));
            cur = y;
        }
        *out = cur;
        *owed = Pending{};
        return T2V_OK;
    }

    // c7,N,R, (d,N,R) x n, RB x nb; defer: as res_chain
    int encoder(const Ptrs& x, float** act, int nb, float* tmp[4], const float** out, bool defer, Pending* owed) {
        const int n = g.is_local ? 1 : g.n_downsample;
        // (the stem's output feeds the first stride-2 layer only, act[i] the layer after it only: where that layer is
        // T2V_ALGO_DIRECT_BF16X2 the apply pass stores the pair layout in place; act[n] goes on in fp32)
        bool pairs = n > 0 && reads_pairs(li + 1);
        T2V_TRY(conv_norm(x, Pending{}, at(act[0], b.lvl[0]), 1, nullptr, n > 0 && next_takes_raw(), owed, false, pairs));
        for (int i = 0; i < n; ++i) {
            const bool x_pairs = pairs;
            pairs = i + 1 < n && reads_pairs(li + 1);
            T2V_TRY(conv_norm(at(act[i], b.lvl[i]), *owed, at(act[i + 1], b.lvl[i + 1]), 1, nullptr,
                              i + 1 < n && next_takes_raw(), owed, x_pairs, pairs));
        }
        if (nb == 0) {
            T2V_REQUIRE(!defer, "internal: an encoder without blocks ends in an applied norm");
            *out = act[n];
            return T2V_OK;
        }
        return res_chain(act[n], nb, tmp, out, defer, owed);
    }

    // *owed: the norm the last layer left to the head
    // x_pairs: x is in the pair layout (decoder_reads_pairs(): the caller's chain stored it so); dec[l], l > 0, is read by the
    // next layer alone and takes the layout where that layer asks for it; dec[0] goes to the head and export_feat in fp32
    int decoder(const float* x, float** dec, const float** out, Pending* owed, bool x_pairs) {
        const int n = g.is_local ? 1 : g.n_downsample;
        const float* cur = x;
        size_t cur_stride = b.bott;
        *owed = Pending{};
        for (int i = 0; i < n; ++i) {
            const int l = n - 1 - i;
            float* y = dec[l];
            // (the direct 128 <-> 256 layers load by LDS-DMA with hardware zero padding and take no pending norm: has_norm
            // layers other than polyphase never answer next_takes_raw)
            const bool y_pairs = i + 1 < n && reads_pairs(li + 1);
            T2V_TRY(conv_norm(at(cur, cur_stride), *owed, at(y, b.lvl[l]), 1, nullptr, next_takes_raw(), owed, x_pairs, y_pairs));
            x_pairs = y_pairs;
            cur = y;
            cur_stride = b.lvl[l];
        }
        *out = cur;
        return T2V_OK;
    }
};

}  // namespace
}  // namespace t2v

using namespace t2v;

extern "C" {

int t2v_generator_num_layers(const t2v_gen_desc* d) {
    if (check_desc(d) != T2V_OK) return -1;
    std::vector<LayerSpec> L;
    enumerate_layers(*d, L);
    return (int)L.size();
}

int t2v_generator_layer_desc(const t2v_gen_desc* d, int i, t2v_conv_desc* out, int* x_cs) {
    T2V_TRY(check_desc(d));
    std::vector<LayerSpec> L;
    enumerate_layers(*d, L);
    T2V_REQUIRE(i >= 0 && i < (int)L.size() && out, "layer index %d out of range", i);
    *out = L[i].cd;
    if (x_cs) *x_cs = L[i].x_cs;
    return T2V_OK;
}

size_t t2v_generator_workspace_bytes_batch(const t2v_gen_desc* d, int batch) {
    if (check_desc(d) != T2V_OK || batch < 1 || batch > kMaxBatch) return 0;
    std::vector<LayerSpec> L;
    enumerate_layers(*d, L);
    Arena a{nullptr, 0};
    Buffers b;
    plan_buffers(*d, L, batch, a, b);
    return a.off;
}
size_t t2v_generator_workspace_bytes(const t2v_gen_desc* d) { return t2v_generator_workspace_bytes_batch(d, 1); }

int t2v_generator_forward_batch(t2v_ctx* ctx, void* stream, const t2v_gen_desc* d, const t2v_layer* layers, int n_layers,
                                const t2v_gen_io* ios, int batch, void* workspace, size_t ws_bytes) {
    T2V_REQUIRE(ctx && layers && ios && workspace, "generator_forward: null pointer");
    T2V_REQUIRE(batch >= 1 && batch <= kMaxBatch, "generator_forward: batch %d out of range [1,%d]", batch, kMaxBatch);
    T2V_TRY(check_desc(d));
    T2V_TRY(check_async_errors());      // a hand-over that timed out in an earlier frame is reported here
    std::vector<LayerSpec> specs;
    enumerate_layers(*d, specs);
    T2V_REQUIRE(n_layers == (int)specs.size(), "generator_forward: expected %d layers, got %d", (int)specs.size(),
                n_layers);
    T2V_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
    for (int im = 0; im < batch; ++im) {
        const t2v_gen_io* io = ios + im;
        T2V_REQUIRE(io->pose && io->prev && io->out, "generator_forward: pose/prev/out must be set (image %d)", im);
        if (d->is_local) {
            T2V_REQUIRE(io->coarse_img_feat, "local generator needs coarse_img_feat");
            T2V_REQUIRE(d->no_flow || io->coarse_flow_feat, "local generator with flow needs coarse_flow_feat");
        }
    }
    for (int i = 0; i < n_layers; ++i)
        T2V_REQUIRE(layers[i].w && layers[i].bias, "layer %d: weight/bias pointer missing", i);
    Arena a{reinterpret_cast<char*>(workspace), ws_bytes};
    Buffers b;
    plan_buffers(*d, specs, batch, a, b);
    if (a.overflow) {
        set_error("generator_forward: workspace %zu bytes < required %zu", ws_bytes, a.off);
        return T2V_ERR_WORKSPACE;
    }
    hipStream_t s = (hipStream_t)stream;
    // Two streams: the pose encoder and the previous-frame encoder are independent until their sum, and so
    // are the image and flow branches after it.  Each branch is a chain of ~50-100 kernels, a third of them
    // small (norm finalize / apply, Winograd transforms: 5-13 us, launch- and tail-bound); run side by side
    // the other branch's GEMM blocks fill those gaps.  T2V_STREAMS=1 runs everything on the caller's stream.
    // Not where every kernel fills the chip by itself: a single-scale 1024x1024 frame (128x128 bottleneck, 1024 Winograd
    // tiles per position; whole-chip launches of 0.5-1.1 ms) is 1.6-2.2 % FASTER on one stream (41.5 vs 42.2 ms, no flow
    // 31.8 vs 32.5), 768x768 and everything below it 1-5 % slower -- so the default (T2V_STREAMS unset / 0) decides by size.
    const int bott_tiles = ((d->H >> d->n_downsample) + 3) / 4 * (((d->W >> d->n_downsample) + 3) / 4);
    const bool two_streams = options().streams == 2 || (options().streams == 0 && (d->is_local || bott_tiles < 1024));
    const OverlapScope overlap(two_streams);     // (kernels that leave the other stream wave slots, where they exist)
    hipStream_t s2 = two_streams ? ctx->side : s;
    auto fork = [&]() -> int {
        if (!two_streams) return T2V_OK;
        T2V_HIP_CHECK(hipEventRecord(ctx->ev_fork, s));
        T2V_HIP_CHECK(hipStreamWaitEvent(s2, ctx->ev_fork, 0));
        return T2V_OK;
    };
    auto join = [&]() -> int {
        if (!two_streams) return T2V_OK;
        T2V_HIP_CHECK(hipEventRecord(ctx->ev_join, s2));
        T2V_HIP_CHECK(hipStreamWaitEvent(s, ctx->ev_join, 0));
        return T2V_OK;
    };
    const int n = d->is_local ? 1 : d->n_downsample;
    const int G = d->ngf;
    const size_t bott = b.bott;
    const int nb_enc = d->is_local ? 0 : d->n_blocks - d->n_blocks / 2;
    const int nb_res = d->is_local ? d->n_blocks : d->n_blocks / 2;
    const int enc_layers = 1 + n + 2 * nb_enc;                 // layers of one encoder
    const int branch_layers = 2 * nb_res + n + 1;              // res trunk + decoder + head of one branch
    Runner r{ctx, s, *d, specs, layers, b, batch};
    Runner r2{ctx, s2, *d, specs, layers, b, batch};
    r2.sc = 1;      // (a scratch set of its own on one stream as well: the join reads both encoders' (mean, rstd) tables)

    Ptrs pose{}, prevp{};
    for (int im = 0; im < batch; ++im) {
        pose.p[im] = ios[im].pose;
        prevp.p[im] = ios[im].prev;
    }
    // d = model_down_seg(x) + model_down_img(prev)
    float* tmpA[4] = {b.bt[0], b.bt[1], b.bt[2], b.bt[3]};
    float* tmpB[4] = {b.bt2[0], b.bt2[1], b.bt2[2], b.bt2[3]};
    const float *segout, *imgout;
    T2V_TRY(fork());
    r2.li = enc_layers;
    // Both chains lazy (they have the same layers): their closing norms + residuals and the sum of the two run as ONE pass
    // after the join instead of two apply passes and an add
    const bool fused_join = r.chain_is_lazy(1 + n, nb_enc);
    Pending owedA, owedB;
    T2V_TRY(r2.encoder(prevp, b.encB, nb_enc, tmpB, &imgout, fused_join, &owedB));
    T2V_TRY(r.encoder(pose, b.encA, nb_enc, tmpA, &segout, fused_join, &owedA));
    T2V_TRY(join());
    // (norm + x) + seg: the order the fused form summed in
    if (fused_join) {
        T2V_TRY(launch_inorm_join(s, r2.join_side(owedB, 0, imgout), r.join_side(owedA, 0, segout), b.d,
                                  (long)(d->H >> n) * (d->W >> n), G << n, batch));
    } else {
        T2V_TRY(launch_add(s, imgout, segout, b.d, (long)(batch * bott)));
    }
    const float* dsum = b.d;
    r.li = 2 * enc_layers;

    const float* img_in = dsum;
    const float* flow_in = dsum;
    if (d->is_local) {
        for (int im = 0; im < batch; ++im) {
            T2V_TRY(launch_add(s, dsum + im * bott, ios[im].coarse_img_feat, b.dimg + im * bott, (long)bott));
            if (!d->no_flow)
                T2V_TRY(launch_add(s, dsum + im * bott, ios[im].coarse_flow_feat, b.dflow + im * bott, (long)bott));
        }
        img_in = b.dimg;
        if (!d->no_flow) flow_in = b.dflow;
    }
    const size_t px4 = (size_t)d->H * d->W * 4, feat = (size_t)d->H * d->W * G;
    MutPtrs raw{}, fw{};
    bool blend[kMaxBatch];
    for (int im = 0; im < batch; ++im) {
        blend[im] = !(d->no_flow || ios[im].use_raw_only);
        raw.p[im] = ios[im].raw ? ios[im].raw : (blend[im] ? b.raw + im * px4 : ios[im].out);
        fw.p[im] = ios[im].flow_w ? ios[im].flow_w : b.fw + im * px4;
    }
    float *want_img_feat[kMaxBatch], *want_flow_feat[kMaxBatch];
    for (int im = 0; im < batch; ++im) {
        want_img_feat[im] = ios[im].img_feat;
        want_flow_feat[im] = ios[im].flow_feat;
    }
    // Both branches of the global generator start from the same map d: where their chains are F(4x4) lazy chains, the input
    // transform of d runs once, before the fork, and both first GEMMs read that V
    const float* v0 = nullptr;
    if (b.vshare && img_in == flow_in && r.chain_is_lazy(2 * enc_layers, nb_res)) {
        T2V_TRY(r.share_v(2 * enc_layers, dsum));
        v0 = b.vshare;
    }
    Pending owed_img, owed_flow;      // one per branch: the branches run on two streams and share nothing
    if (!d->no_flow) {
        // flow branch on the side stream (temporaries bt2: the encoders are done with them)
        T2V_TRY(fork());
        r2.li = 2 * enc_layers + branch_layers;
        const float *res_flow, *flow_feat;
        const bool pairs = r2.reads_pairs(r2.li + 2 * nb_res);      // the decoder's first layer (enumerate_layers: nb_res > 0 then)
        T2V_TRY(r2.res_chain(flow_in, nb_res, tmpB, &res_flow, false, &owed_flow, v0, pairs));
        T2V_TRY(r2.decoder(res_flow, b.decF, &flow_feat, &owed_flow, pairs));
        T2V_TRY(r2.head(r2.at(flow_feat, feat), owed_flow, fw));
        T2V_TRY(r2.export_feat(flow_feat, feat, owed_flow, want_flow_feat));
    }
    const float *res_img, *img_feat;
    const bool img_pairs = r.reads_pairs(r.li + 2 * nb_res);
    T2V_TRY(r.res_chain(img_in, nb_res, tmpA, &res_img, false, &owed_img, v0, img_pairs));
    T2V_TRY(r.decoder(res_img, b.decI, &img_feat, &owed_img, img_pairs));
    T2V_TRY(r.head(r.at(img_feat, feat), owed_img, raw));
    T2V_TRY(r.export_feat(img_feat, feat, owed_img, want_img_feat));
    if (!d->no_flow) {
        T2V_TRY(join());
        r.li += branch_layers;
        T2V_REQUIRE(r2.li == n_layers, "internal: flow branch consumed up to layer %d of %d", r2.li, n_layers);
        const int prev_cs = round_up(d->prev_nc, 4);
        for (int im = 0; im < batch; ++im)
            if (blend[im])
                T2V_TRY(launch_warp_composite(s, raw.p[im], fw.p[im], ios[im].prev, prev_cs, d->prev_nc - 3, ios[im].out,
                                              nullptr, d->H, d->W));
    }
    for (int im = 0; im < batch; ++im)
        if (!blend[im] && raw.p[im] != ios[im].out)
            T2V_HIP_CHECK(hipMemcpyAsync(ios[im].out, raw.p[im], px4 * sizeof(float), hipMemcpyDeviceToDevice, s));
    T2V_REQUIRE(r.li == n_layers, "internal: consumed %d of %d layers", r.li, n_layers);
    return T2V_OK;
}

int t2v_generator_forward(t2v_ctx* ctx, void* stream, const t2v_gen_desc* d, const t2v_layer* layers, int n_layers,
                          const t2v_gen_io* io, void* workspace, size_t ws_bytes) {
    return t2v_generator_forward_batch(ctx, stream, d, layers, n_layers, io, 1, workspace, ws_bytes);
}

}  // extern "C"
