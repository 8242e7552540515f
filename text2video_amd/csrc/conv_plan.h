// conv_plan.h -- host-side planning of one convolution launch (shared by capi.hip/generator.hip).
#pragma once
#include "t2v_internal.h"

namespace t2v {

struct ConvPlan {
    ConvKParams kp;   // everything except the pointers / Cout_s
    int tile;         // ConvTile
    int BM, BN;
    int Hout, Wout;
    int Cout_p;       // Cout rounded up to the N tile (rows of the packed weight)
    int Cin;          // real input channels (<= kp.Cin_s)
    int nparts;       // instance-norm partial-statistics rows (= nphases * mtiles)
    size_t wfloats;   // packed weight size
};

int build_conv_plan(const t2v_conv_desc* d, int x_cs, bool need_stats, ConvPlan* out);
// F(4x4,3x3) in either arithmetic: the split-bf16 form shares every geometry, layout size and the output transform
inline bool is_split(int algo) { return algo == T2V_ALGO_WINOGRAD_F4_BF16X2; }
inline bool is_f4(int algo) { return algo == T2V_ALGO_WINOGRAD_F4 || is_split(algo); }
inline bool is_winograd(int algo) { return algo == T2V_ALGO_WINOGRAD || is_f4(algo); }
inline int wino_m(int algo) { return is_f4(algo) ? 4 : 2; }          // output tile edge
inline int wino_pos(int algo) { return (wino_m(algo) + 2) * (wino_m(algo) + 2); }    // transform positions: 16 | 36
inline int wino_out_h(const t2v_conv_desc* d) { return d->H + 2 * d->pad - 2; }   // 3x3, stride 1
inline int wino_out_w(const t2v_conv_desc* d) { return d->W + 2 * d->pad - 2; }
// tiles of the ceil(H/m) x ceil(W/m) grid, real and padded to whole GEMM tiles per transform position
inline TileGrid wino_tile_grid(const t2v_conv_desc* d, int algo) { return tile_grid(wino_out_h(d), wino_out_w(d), wino_m(algo)); }
inline int wino_tiles_padded(const t2v_conv_desc* d, int algo) { return wino_tile_grid(d, algo).Tp; }
inline int wino_tiles_real(const t2v_conv_desc* d, int algo) { return wino_tile_grid(d, algo).T; }
// GEMM rows per transform position for a batch of nimg images: F(4x4) packs the images' tiles and pads the total
inline int wino_rows_batch(const t2v_conv_desc* d, int algo, int nimg) {
    return (nimg > 1 && is_f4(algo)) ? wino_pad_tiles(nimg * wino_tiles_real(d, algo)) : wino_tiles_padded(d, algo);
}
inline size_t winograd_vm_floats(const t2v_conv_desc* d, int nimg = 1) {             // V + M of `nimg` images
    return (size_t)wino_pos(d->algo) * wino_rows_batch(d, d->algo, nimg) * ((size_t)d->Cin + d->Cout);
}
// ... followed, for F(4x4,3x3), by the hand-over scratch of the fixed-grid GEMM (conv_igemm.hip: wino_gemm_sk_kernel; the
// split-bf16 form keeps the size and leaves the scratch alone)
inline size_t winograd_workspace_floats(const t2v_conv_desc* d, int nimg = 1) {
    return winograd_vm_floats(d, nimg) + (is_f4(d->algo) ? wino_gemm_sk_scratch_floats() : 0);
}
// GEMM rows of the whole conv (all positions): what the algorithm choice compares
inline long wino_gemm_rows(const t2v_conv_desc* d, int algo) { return (long)wino_pos(algo) * wino_tiles_padded(d, algo); }
bool winograd_supported(const t2v_conv_desc* d, int x_cs, int algo);
// ---- polyphase Winograd F(4,2) of the stride-2 / transposed 3x3 layers (polyphase.hip): 81 positions, tiles of 4x4 outputs
// (down) | 4x4 inputs = 8x8 outputs (up)
bool polyphase_supported(const t2v_conv_desc* d, int x_cs);
bool polyphase_pays(const t2v_conv_desc* d, int x_cs);      // ... and is the faster form (the generator's selection rule)
// either arithmetic: the split-bf16 form shares every geometry, layout size and the output transforms
inline bool is_poly_split(int algo) { return algo == T2V_ALGO_POLYPHASE_BF16X2; }
inline bool is_poly(int algo) { return algo == T2V_ALGO_POLYPHASE || is_poly_split(algo); }
// the direct stride-2 / transposed conv in split-bf16 arithmetic (conv_igemm_split.hip): the plan, the packed-weight size and
// the statistics partials are those of the direct form on 128 x 128 tiles
inline bool is_direct_split(int algo) { return algo == T2V_ALGO_DIRECT_BF16X2; }
bool direct_split_supported(const t2v_conv_desc* d, int x_cs);
// x: the input in the pair layout (an inorm_apply_split pass or launch_split_pairs made it), w_packed: pack_weight's
int direct_split_forward(hipStream_t s, const t2v_conv_desc* d, const float* x_pairs, const float* w_packed, const float* bias,
                         float* y, float* stats_partial);
inline bool is_bf16x2(int algo) { return is_split(algo) || is_poly_split(algo) || is_direct_split(algo); }      // the forward-only forms
// ... the split-bf16 form (81 GEMMs on wino_split_gemm_kernel) takes the layer
bool polyphase_split_supported(const t2v_conv_desc* d, int x_cs);
inline TileGrid poly_tile_grid(const t2v_conv_desc* d) {
    return d->transposed ? tile_grid(d->H, d->W, 4) : tile_grid(d->H / 2, d->W / 2, 4);
}
inline int poly_tiles_real(const t2v_conv_desc* d) { return poly_tile_grid(d).T; }
inline int poly_tiles_padded(const t2v_conv_desc* d) { return poly_tile_grid(d).Tp; }
inline int poly_out_h(const t2v_conv_desc* d) { return d->transposed ? 2 * d->H : d->H / 2; }
inline int poly_out_w(const t2v_conv_desc* d) { return d->transposed ? 2 * d->W : d->W / 2; }
inline int poly_m(const t2v_conv_desc* d) { return d->transposed ? 8 : 4; }       // output tile edge (statistics partial geometry)
// (the split-bf16 form keeps the size and leaves the scratch alone)
inline size_t polyphase_workspace_floats(const t2v_conv_desc* d) {                // V + M + the fixed-grid GEMM's hand-over scratch
    return (size_t)81 * poly_tiles_padded(d) * ((size_t)d->Cin + d->Cout) + wino_gemm_sk_scratch_floats();
}
// lazy != null: x is the previous layer's raw conv output; its norm (+ ReLU) is applied inside the input transform
int polyphase_forward(t2v_ctx* ctx, hipStream_t s, const t2v_conv_desc* d, const float* x, const float* w_packed,
                      const float* bias, float* y, float* stats_partial, float* workspace, int stages,
                      const LazyNorm* lazy = nullptr);
int best_conv_algo(const t2v_conv_desc* d, int x_cs, int cap);
// A batch of images through one Winograd conv (F(4x4,3x3) only when nimg > 1): the images' maps x / y are
// `img_stride_x` / H*W*Cout floats apart, V and M hold nimg*Tp tile rows per transform position (one GEMM with
// M = nimg*Tp rows per position), the statistics partials follow each other image by image.
struct WinoBatch {
    int nimg = 1;
    long img_stride_x = 0;     // floats between the input maps
    // keep_v != null (nimg == 1): V goes into slot `keep_slot` of a batch-wide tile list [36][keep_total * Tp][Cin] -- the
    // Winograd-domain weight gradient's workspace -- instead of the call's own workspace, and the GEMM reads it from there
    float* keep_v = nullptr;
    int keep_total = 1, keep_slot = 0;
    // v_in != null: the GEMM reads a V that another call made of the same input (same geometry and batch) instead of the
    // workspace's own; `stages` then leaves the input transform out
    const float* v_in = nullptr;
    // lazy != null (F(4x4,3x3), own V): x is a raw conv output whose norm the input transform applies (stage bit 1)
    const LazyNorm* lazy = nullptr;
};
int winograd_forward(t2v_ctx* ctx, hipStream_t s, const t2v_conv_desc* d, const float* x, const float* w_packed,
                     const float* bias, float* y, float* stats_partial, float* workspace, int stages,
                     const WinoBatch* batch = nullptr);
// statistics partials one image of `d`'s output leaves for its norm (floats); 0 where the layer has no plan
size_t norm_partial_floats(const t2v_conv_desc* d, int x_cs);
// partials -> (mean, rstd) with the launcher that matches the producer's partial geometry; `pooled_images` images' partials
// (back to back) pool into one table.  plan: the producer's direct-conv plan where the caller has built it already
int finalize_norm(hipStream_t s, const t2v_conv_desc* producer, int x_cs, const float* stats, int pooled_images, float eps,
                  float* mean_rstd, double* scratch = nullptr, const RunningUpdate* ru = nullptr, const ConvPlan* plan = nullptr);
int run_conv(t2v_ctx* ctx, hipStream_t s, const ConvPlan& pl, const float* x, const float* w, const float* bias,
             float* y, int y_cs, float* stats);
// the plan is one the dedicated 7x7 head kernel takes (conv_head.hip) ...
bool conv_plan_is_head7x7(const ConvPlan& pl);
// ... and that launch; lazy != null: x is the previous layer's raw conv output, normalised inside the kernel
int run_head7x7(hipStream_t s, const ConvPlan& pl, const float* x, const float* w, const float* bias, float* y, int y_cs,
                const LazyNorm* lazy);
// `batch` images a constant stride apart in one implicit-GEMM launch (blockIdx.y); strides in floats
int run_conv_batch(t2v_ctx* ctx, hipStream_t s, const ConvPlan& pl, int batch, const float* x, long x_stride, const float* w,
                   const float* bias, float* y, int y_cs, long y_stride, float* stats, long stats_stride);

}  // namespace t2v
