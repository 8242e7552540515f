/*
 * t2v.h -- C ABI of libt2v_hip.so: the MI355X (gfx950) frame-synthesis hot path of Text2Video.
 *
 * This is the drop-in boundary "B2" of SURVEY.md section 8(b).  The reference reaches its device
 * kernels through torch-0.4.1's THCUNN C ABI; each entry point below names the reference
 * interface it replaces ($SP = /root/reference/venv_vid2vid/lib/python3.7/site-packages).
 *
 * Conventions
 *   - plain C: pointers + sizes, no torch types.  All tensor pointers are DEVICE pointers to
 *     fp32 NHWC data (channels innermost) unless stated otherwise.  "cs" arguments are the
 *     channel *storage* stride (a multiple of 4 >= the logical channel count; extra channels
 *     must hold finite values and are ignored / written as zero).
 *   - ownership: the caller allocates every device buffer (tensors, packed weights, workspace)
 *     and keeps it alive until the stream has drained.  The compute entry points never allocate device memory; a
 *     host that has no device allocator of its own gets buffers, streams and events from the "host plumbing" section
 *     at the end (ABI 14).
 *   - asynchronous: work is enqueued on the hipStream_t passed as `void* stream`
 *     (torch.cuda.current_stream().cuda_stream on the Python side); nothing synchronises.
 *   - errors: every call returns T2V_OK (0) or a negative t2v_status; t2v_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI.  (THCUNN raised THError -> Python
 *     RuntimeError; the Python binding re-raises RuntimeError from the status code.)
 *   - threading: a t2v_ctx is bound to one device; use one ctx per host thread.
 */
#ifndef T2V_H_
#define T2V_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* (T2V_ALGO_POLYPHASE_BF16X2, t2v_conv_polyphase_bf16x2_supported and t2v_gen_desc.conv_algo 4 came after 22 and left it
 * alone: they add a symbol and values, no existing entry, struct or value changed.  So did T2V_ALGO_DIRECT_BF16X2 and
 * t2v_gen_desc.conv_algo 5; the two entry points of that form are declared in t2v_bf16x2.h.) */
#define T2V_ABI_VERSION 22

typedef enum {
    T2V_OK = 0,
    T2V_ERR_INVALID = -1,   /* bad argument / unsupported shape */
    T2V_ERR_HIP = -2,       /* a HIP runtime call failed */
    T2V_ERR_WORKSPACE = -3, /* workspace too small */
    T2V_ERR_HANDOVER = -4   /* a fixed-grid kernel's accumulator hand-over timed out in an EARLIER launch: that launch's
                             * output holds NaNs; reported once, the process then runs one block per tile */
} t2v_status;

enum { T2V_PAD_ZERO = 0, T2V_PAD_REFLECT = 1 };
/* epilogue activations fused into the conv (Tanh_updateOutput THCUNN.h:1177,
 * Sigmoid_updateOutput :1098, flow x20 [SURVEY App. A.1]) */
enum { T2V_ACT_NONE = 0, T2V_ACT_TANH = 1, T2V_ACT_FLOW_W = 2 /* ch0,1: x*20 ; ch2: sigmoid */,
       T2V_ACT_LRELU = 3 /* x>0 ? x : act_scale*x  (LeakyReLU_updateOutput THCUNN.h:220) */ };

/* Convolution algorithm, all fp32.  WINOGRAD = F(2x2,3x3): input transform -> 16 batched GEMMs on the
 * implicit-GEMM kernel -> output transform fused with bias and the norm statistics (2.25x fewer MFMA
 * FLOPs than the direct conv).  WINOGRAD_F4 = F(4x4,3x3), 36 batched GEMMs, 4x fewer MFMA FLOPs,
 * interpolation points {0, +-3/4, +-3/2, inf} (rounding error ~4x the direct kernel's, 1.5e-6 of the
 * output's std per conv).  Only where t2v_conv_winograd_supported() says so; packed weights differ
 * per algorithm.
 * POLYPHASE (ABI 15) = the stride-2 3x3 convs (zero pad 1) and ConvTranspose2d(3, stride 2, pad 1, output_padding 1) as
 * polyphase Winograd F(4,2): per dimension the 2-tap sub-correlation on one sub-pixel phase as F(4,2) (5 products per 4
 * outputs), the 1-tap one as it is -- 81 batched GEMMs [tiles x Cin] x [Cin x Cout] per 4x4 (8x8) output tile instead of
 * 144 multiply-adds per channel pair: 0.5625x the MFMA FLOPs of SpatialConvolutionMM / SpatialFullDilatedConvolution
 * (THCUNN.h:664,794), points {0, +-3/4, 3/2, inf}.  Only where t2v_conv_polyphase_supported() says so; it goes through
 * the *_winograd entry points (pack_weight, workspace_floats, forward_winograd), its statistics partials through the
 * finalize entries like any producer's.
 * WINOGRAD_F4_BF16X2 (ABI 22) = WINOGRAD_F4 with its 36 GEMMs on the bf16 matrix cores, the one form that is NOT fp32
 * throughout: every fp32 operand v of the GEMM stage is split into hi = bf16(v) and lo = bf16(v - hi) (round to nearest
 * even) and the contraction is sum_k (ah*bh + ah*bl + al*bh), accumulated in fp32; al*bl is dropped.  About 16 mantissa
 * bits per product -- of the Winograd-domain operands V and U, which are an order larger than the output they cancel to,
 * so the split error is amplified: measured (profiles/split_bf16_accuracy.txt) 2.2e-5 of the output's
 * rms per 64 -> 128 conv against 1.8e-7 for WINOGRAD_F4 (about 120x), and max |frame - float64| 1.8e-4 against 2.7e-5 (6.9x)
 * on a 160 x 160 two-block generator, below the 1e-3 parity bar.  (The reduced-precision trade
 * upstream's --fp16 offered; SpatialConvolutionMM_updateOutput, THCUNN.h:664, as THCUNN's half instantiation ran it.)  The
 * transforms, bias and statistics are WINOGRAD_F4's fp32 arithmetic.  V and U hold two bf16 planes in the bytes of the fp32
 * tensors: every size is WINOGRAD_F4's.  Forward only, where t2v_conv_winograd_bf16x2_supported() says so; never chosen by
 * t2v_conv_best_algo -- a caller opts in (t2v_gen_desc.conv_algo 3).
 * POLYPHASE_BF16X2 = POLYPHASE with its 81 GEMMs in the same split-bf16 arithmetic on the same kernel (SpatialConvolutionMM /
 * SpatialFullDilatedConvolution, THCUNN.h:664,794, as THCUNN's half instantiations ran them).  Transforms, bias and statistics
 * are POLYPHASE's fp32 arithmetic; V and U hold two bf16 planes in the bytes of the fp32 tensors, so every size is POLYPHASE's.
 * The F(4,2) operands are milder than F(4x4,3x3)'s: the float64 emulation of the form gives 1.7e-5 of the output's rms per
 * conv.  Forward only, where t2v_conv_polyphase_bf16x2_supported() says so; never chosen by t2v_conv_best_algo -- a caller
 * opts in (t2v_gen_desc.conv_algo 4).
 * DIRECT_BF16X2 = DIRECT for the 3x3 stride-2 conv and the transposed conv, its contraction in the same split-bf16 arithmetic
 * (SpatialConvolutionMM / SpatialFullDilatedConvolution, THCUNN.h:664,794, as THCUNN's half instantiations ran them).  The input
 * map and the packed weight hold, in place of every fp32 channel pair, the dwords {hi.x, hi.y | lo.x, lo.y}: every size is
 * DIRECT's.  Bias and statistics partials are DIRECT's fp32 epilogue on 128 x 128 tiles.  It runs through the
 * t2v_conv2d_forward_winograd* entries, whose workspace (t2v_conv_winograd_workspace_floats: H*W*Cin floats) receives the split
 * of x.  Forward only, where t2v_conv_direct_bf16x2_supported of t2v_bf16x2.h says so; never chosen by t2v_conv_best_algo -- a caller opts
 * in (t2v_gen_desc.conv_algo 5). */
enum { T2V_ALGO_DIRECT = 0, T2V_ALGO_WINOGRAD = 1, T2V_ALGO_WINOGRAD_F4 = 2, T2V_ALGO_POLYPHASE = 3,
       T2V_ALGO_WINOGRAD_F4_BF16X2 = 4, T2V_ALGO_POLYPHASE_BF16X2 = 5, T2V_ALGO_DIRECT_BF16X2 = 6 };

typedef struct t2v_ctx t2v_ctx;

int t2v_abi_version(void);
const char* t2v_last_error(void);
int t2v_create(t2v_ctx** out, int device);
int t2v_destroy(t2v_ctx* ctx);
/* The T2V_* environment switches are read once, at the first t2v_create; this reads them again.
 * (THCUNN's counterpart are process-global flags such as torch.backends.cudnn.benchmark,
 * $SP/torch/backends/cudnn/__init__.py:454-455.) */
void t2v_reload_env(void);
/* Errors a kernel can only report after the fact (THCUNN: THError out of a later synchronising call).  T2V_OK, or
 * T2V_ERR_HANDOVER once after a fixed-grid hand-over timed out; every entry point that can launch such a kernel makes the
 * same check first.  Callers run it after they synchronise a stream. */
int t2v_check_async_errors(void);
/* 1 while the fixed-grid ("stream-K") forms of the Winograd GEMM stage / weight-gradient reduction may be used: the
 * dispatch-order self-test of t2v_create passed and no hand-over has timed out; 0: one block per tile everywhere. */
int t2v_fixed_grid_enabled(void);
/* Overlap hint (ABI 13): on != 0 tells the library that the caller runs a SECOND stream beside the one it passes in, so that
 * kernels which leave wave slots to that stream are preferred where they exist (today: the 512x512 ResnetBlock GEMM stage on
 * 256x128 tiles with one block per CU instead of 128x128 with two -- slower alone, faster in a two-stream frame).  Per calling
 * thread; returns the previous value.  t2v_generator_forward[_batch] sets it for its own launches; a caller that overlaps
 * single-op calls itself (or wants t2v_conv_winograd_gemm_form to answer for the generator's frames) sets it explicitly.
 * on == 2 (ABI 18): the second stream carries fixed-grid GEMMs of its OWN (the train step's weight gradients beside its data
 * gradients): the whole-tile fixed-grid GEMM and the Winograd-domain weight gradient then launch ONE 128x128 block per CU
 * (half a CU's LDS and registers each) instead of two, so that the two streams' launches -- and the bandwidth-bound kernels
 * between two GEMMs -- are resident side by side instead of queueing behind a grid that keeps every CU full until its last
 * block leaves.  The tile forms chosen are those of on == 0; the results carry the same bits.  T2V_SK_BLOCKS_PER_CU=1 / 2
 * forces one / two per CU whatever the hint.
 * (THCUNN has no counterpart: its ops run on the one current stream of THCState.) */
int t2v_set_overlap_hint(int on);
/* Test hook: raise != 0 sets the sticky error word exactly as a timed-out consumer wave would; raise == 0 clears it and
 * switches the fixed-grid kernels back on. */
void t2v_debug_async_error(int raise);

/* ------------------------------------------------------------------------------------------
 * Convolution.  Replaces SpatialReflectionPadding_updateOutput (THCUNN.h:952) +
 * SpatialConvolutionMM_updateOutput (THCUNN.h:664) [Conv2d.forward $SP/torch/nn/modules/conv.py:
 * 299-300] and SpatialFullDilatedConvolution_updateOutput (THCUNN.h:794) [ConvTranspose2d.forward
 * conv.py:687-691].  Reflection padding is resolved inside the kernel's tile loader.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int H, W;        /* input spatial size */
    int Cin, Cout;   /* logical channels */
    int kH, kW;      /* kernel */
    int stride;      /* 1 or 2 */
    int pad;         /* padding on each side (reflect: the ReflectionPad2d amount) */
    int pad_mode;    /* T2V_PAD_ZERO | T2V_PAD_REFLECT */
    int transposed;  /* 1: ConvTranspose2d(k in {3,4}, stride=2, padding, output_padding) */
    int act;         /* T2V_ACT_* applied after bias */
    float act_scale; /* T2V_ACT_FLOW_W: flow multiplier (20 * 2^scale); T2V_ACT_LRELU: negative slope */
    int output_padding; /* transposed only (0 or 1); the generator's up-convs use 1 */
    int algo;           /* T2V_ALGO_DIRECT | T2V_ALGO_WINOGRAD (3x3 stride-1 reflect-pad-1 convs only) */
} t2v_conv_desc;

/* output spatial size */
int t2v_conv_out_dims(const t2v_conv_desc* d, int* Hout, int* Wout);
/* number of floats of the packed weight buffer (includes all zero padding) */
size_t t2v_conv_packed_weight_floats(const t2v_conv_desc* d, int x_cs);
/* repack a torch-layout weight ([Cout,Cin,kH,kW], or [Cin,Cout,3,3] when transposed -- conv.py:
 * 28-33) that already lives on the device into the kernel's K-contiguous layout. */
int t2v_conv_pack_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs,
                         const float* w_torch_dev, float* packed_dev);
/* The same for the DATA-GRADIENT conv `d` of a stride-1 forward layer, given that layer's own torch weight
 * [Cout_f = d->Cin][Cin_f = d->Cout][k][k]: the 180-degree flip and the in/out transpose of updateGradInput's filter are
 * folded into the gather (no flipped / transposed copy of the weight is ever made). */
int t2v_conv_pack_weight_adjoint(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs,
                                 const float* w_forward_torch_dev, float* packed_dev);
/* number of floats of the per-tile instance-norm partial-statistics buffer for this conv */
size_t t2v_conv_stats_floats(const t2v_conv_desc* d);
/* y = act(conv(x) + bias).  If stats_partial != NULL the epilogue also emits per-(tile,channel)
 * (mean, M2) partials over the block's pixels for the fused instance norm. */
int t2v_conv2d_forward(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                       const float* w_packed, const float* bias, float* y, int y_cs,
                       float* stats_partial);
/* The same for `batch` images in ONE launch (ABI 14; direct algorithm): x = [batch][H][W][x_cs], y = [batch][Hout][Wout][y_cs],
 * image b's statistics partials at stats_partial + b * t2v_conv_stats_floats(d).  Every image's result is the single-image
 * call's, bit for bit.  (SpatialConvolutionMM_updateOutput loops over the batch with one GEMM per image, THCUNN.h:664; here the
 * images share a launch because the discriminators' layers of the train step fill a fraction of the chip each.) */
int t2v_conv2d_forward_batch(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x, int x_cs,
                             const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial);
/* A 7x7 generator head on the RAW output of the conv before it (ABI 19): x has not gone through its norm layer yet, and the
 * head's halo-tile kernel applies [relu]((x - mean) * rstd [* gamma + beta]) to every halo plane it stages, with the
 * arithmetic of t2v_instance_norm_apply -- y carries the bits of t2v_instance_norm_apply followed by t2v_conv2d_forward, without
 * the pass over the map in between (what t2v_generator_forward* does with the last decoder layer's output unless
 * T2V_CHAIN_LAZY=0).  d: 7x7, stride 1, ReflectionPad 3, Cout <= 3, x_cs % 16 == 0, H, W >= 4 (the shapes the halo-tile kernel
 * takes; anything else is T2V_ERR_INVALID); mean_rstd [x_cs][2] as t2v_*_norm_finalize writes it -- one row per channel of the conv
 * that produced x, so x_cs == Cin and x has no storage lane; gamma, beta both or neither;
 * relu must be 1 (the norm in front of a head is always followed by its ReLU). */
int t2v_conv2d_forward_head_norm(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                 const float* w_packed, const float* bias, float* y, int y_cs, const float* mean_rstd,
                                 const float* gamma, const float* beta, int relu);

/* Bit mask of the Winograd variants `d` (algo ignored) can run as: 1 = F(2x2,3x3), 2 = F(4x4,3x3).
 * Needs 3x3, stride 1, ReflectionPad 1 or zero padding 0..2 (pad 2: the data gradient of the pad-1 conv),
 * Cin % 32 == 0 == x_cs, Cout % 4 == 0, no activation.  Any H, W >= 2:
 * the ceil(H/m) x ceil(W/m) tile grid (m = 2 | 4) is ragged at the bottom / right edge and padded with
 * empty tiles to a multiple of 128 (extra GEMM rows, masked in the output transform). */
int t2v_conv_winograd_supported(const t2v_conv_desc* d, int x_cs);
/* 1 where `d` (algo ignored) can run as T2V_ALGO_WINOGRAD_F4_BF16X2 (ABI 22): the conditions of F(4x4,3x3) above plus
 * Cin % 32 == 0 and Cout % 128 == 0 (the split GEMM's K stage and tile width).  (THCUNN's counterpart is the type
 * dispatch that picked SpatialConvolutionMM's half instantiation, THCUNN.h:664 under THC_GENERIC_FILE.)  Every backward,
 * weight-gradient and data-gradient entry and query refuses a descriptor whose algo is T2V_ALGO_WINOGRAD_F4_BF16X2. */
int t2v_conv_winograd_bf16x2_supported(const t2v_conv_desc* d, int x_cs);
/* bit 0: T2V_ALGO_POLYPHASE applies to `d` (d->algo ignored); bit 1: ... and is the form the library itself selects (both
 * channel counts >= 256, >= 128 tiles: where it measured faster than the implicit-GEMM kernel).  Applies to: 3x3, stride 2; a conv with zero padding 1 and even H, W, or a
 * transposed conv with pad 1 / output_padding 1; x_cs == Cin, Cin % 32 == 0, Cout % 128 == 0, no activation.  The tile grid
 * (4x4 outputs | 4x4 inputs) is ragged at the bottom / right edge and padded with empty tiles, as for the Winograd forms.  t2v_generator_layer_desc() selects it where it measured faster. */
int t2v_conv_polyphase_supported(const t2v_conv_desc* d, int x_cs);
/* 1 where `d` (algo ignored) can run as T2V_ALGO_POLYPHASE_BF16X2: bit 0 of t2v_conv_polyphase_supported (which asks
 * x_cs == Cin, Cin % 32 == 0 and Cout % 128 == 0, the split GEMM's K stage and tile width) and V and U within the GEMM's
 * 32-bit byte offsets (81 * rows * Cin * 4 bytes each, rows = the padded tile count | Cout).  Every backward, weight-gradient
 * and data-gradient entry and query refuses a descriptor whose algo is T2V_ALGO_POLYPHASE_BF16X2. */
int t2v_conv_polyphase_bf16x2_supported(const t2v_conv_desc* d, int x_cs);
/* The algorithm the library itself would pick for `d` (d->algo ignored): the one with the fewest GEMM rows among
 * direct (9 per output pixel), F(2x2,3x3) and F(4x4,3x3) (16 | 36 per tile, tile count padded to 128).
 * cap: 0 = any, 1 = direct only, 2 = at most F(2x2,3x3).  Returns a T2V_ALGO_* value. */
int t2v_conv_best_algo(const t2v_conv_desc* d, int x_cs, int cap);
/* floats of scratch a Winograd forward needs: transformed input V + transformed output M, and for F(4x4,3x3) the
 * hand-over area of the fixed-grid GEMM stage (blocks that share a 128x128 tile pass accumulators through it; any
 * content on entry, one workspace per conv in flight) */
size_t t2v_conv_winograd_workspace_floats(const t2v_conv_desc* d, int x_cs);
/* ... of t2v_conv2d_forward_winograd_batch_stages for `nimg` packed images (F(4x4,3x3); nimg 1 for the other forms):
 * V and M of pad(nimg * T) rows per position, then the hand-over area; 0 where the form does not take the shape */
size_t t2v_conv_winograd_batch_workspace_floats(const t2v_conv_desc* d, int x_cs, int nimg);
/* GEMM rows one image contributes per F(4x4,3x3) transform position: its ceil(H/4) x ceil(W/4) tiles padded to the
 * 64 / 128-row granule (the slot pitch of the batch-wide tile lists in the weight-gradient workspace) */
int t2v_conv_winograd_tile_rows(const t2v_conv_desc* d);
/* Which form the batched GEMM stage of an F(4x4,3x3) conv over `nimg` images takes under the current switches (reporting
 * only: bench.py's roofline label): one block per tile, or a fixed grid of resident blocks that hand accumulators over where
 * a tile is cut -- on 128x128 tiles, 192x64 tiles, 160x128 tiles with one block per CU (129..160 tile rows: the reference's
 * 512x320 frames), or ragged M tiles of 4,..,4,r 32-row fragments; T2V_ALGO_WINOGRAD_F4_BF16X2 has the one split-bf16 form.
 * -1: not an F(4x4,3x3) conv. */
enum { T2V_GEMM_TILE_PER_BLOCK_64x64 = 0, T2V_GEMM_TILE_PER_BLOCK_128x128 = 1, T2V_GEMM_FIXED_GRID_128x128 = 2,
       T2V_GEMM_FIXED_GRID_192x64 = 3, T2V_GEMM_FIXED_GRID_160x128 = 4, T2V_GEMM_FIXED_GRID_RAGGED = 5,
       T2V_GEMM_FIXED_GRID_256x128 = 6 /* one block per CU, like 160x128 */,
       T2V_GEMM_FIXED_GRID_RAGGED_TALL = 7 /* ragged, balanced tiles of 3..6 fragments, one block per CU */,
       T2V_GEMM_SPLIT_BF16_128x128 = 8 /* T2V_ALGO_WINOGRAD_F4_BF16X2: one block per tile on the bf16 matrix cores (ABI 22;
                                        * SpatialConvolutionMM's GEMM, THCUNN.h:664, in split-bf16 arithmetic) */ };
int t2v_conv_winograd_gemm_form(const t2v_conv_desc* d, int nimg);
/* forward with d->algo == T2V_ALGO_WINOGRAD | T2V_ALGO_WINOGRAD_F4 | T2V_ALGO_WINOGRAD_F4_BF16X2; same contract as
 * t2v_conv2d_forward plus the workspace.  Every form that runs through the *_winograd entries asks "y_cs == Cout" as well as
 * x_cs == Cin (anything else is T2V_ERR_INVALID): these entries meet no storage lane on either side. */
int t2v_conv2d_forward_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial,
                                float* workspace);
/* the same, one stage at a time (measurement and tests): `stages` is a bit mask of
 * 1 = input transform x -> V, 2 = the 16 | 36 batched GEMMs V,U -> M, 4 = output transform M -> y (+bias, stats). */
int t2v_conv2d_forward_winograd_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                       const float* w_packed, const float* bias, float* y, int y_cs,
                                       float* stats_partial, float* workspace, int stages);
/* ... of the generator's forms (tests): `nimg` F(4x4,3x3) images `img_stride` floats apart, packed into one tile list
 * (image i owns GEMM rows [i*T, (i+1)*T), the last one also the padding rows; y and the statistics partials image after
 * image), and with mean_rstd ([nimg][Cin][2]) the previous layer's instance norm applied inside the input transform:
 * F(4x4): relu 1 gives d = relu((x - mean) * rstd [* gamma + beta]); relu 0 with res and xout (pad 1) gives
 * d = norm(x) + res, written to xout as well.  A polyphase desc takes one image, relu 0 | 1 and no res / xout. */
int t2v_conv2d_forward_winograd_batch_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int nimg, const float* x,
                                             int x_cs, long img_stride, const float* w_packed, const float* bias, float* y,
                                             int y_cs, float* stats_partial, float* workspace, int stages,
                                             const float* mean_rstd, const float* gamma, const float* beta, int relu,
                                             const float* res, float* xout);

/* ------------------------------------------------------------------------------------------
 * Instance norm (+affine) + ReLU + residual.  Replaces BatchNormalization_updateOutput(train)
 * (THCUNN.h:33) as reached from F.instance_norm ($SP/torch/nn/functional.py:1258-1301) and
 * Threshold_updateOutput (THCUNN.h:1328).  Biased variance, eps inside the sqrt.
 *   finalize: combines the conv epilogue's partials (Chan et al.) -> mean_rstd[C][2]
 *   apply:    y = act((x-mean)*rstd*gamma+beta) + res1 + res2   (gamma/beta/res* nullable,
 *             y may alias x); relu: 0 none, 1 ReLU, 2 LeakyReLU(0.2) (the discriminators)
 *   Batch statistics (BatchNorm2d in train mode over a batch of B images, the discriminators):
 *   run the conv per image with stats_partial + b*t2v_conv_stats_floats(d), then finalize_batch.
 * ------------------------------------------------------------------------------------------ */
int t2v_instance_norm_finalize(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer,
                               const float* stats_partial, float eps, float* mean_rstd);
int t2v_batch_norm_finalize(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                            const float* stats_partial, float eps, float* mean_rstd);
/* BatchNorm2d's running statistics (training mode; $SP/torch/nn/modules/batchnorm.py:27-29,57-64; the momentum
 * argument of BatchNormalization_updateOutput, THCUNN.h:33-45): running_mean / running_var [C] are updated in place
 * from the (mean, rstd) table a finalize call produced over n values per channel:
 *   running_mean = (1-momentum)*running_mean + momentum*mean
 *   running_var  = (1-momentum)*running_var  + momentum*var*n/(n-1)      (unbiased; var = 1/rstd^2 - eps) */
int t2v_batch_norm_update_running(t2v_ctx* ctx, void* stream, const float* mean_rstd, float* running_mean,
                                  float* running_var, long n, int C, float momentum, float eps);
/* t2v_batch_norm_finalize + `times` running-statistics updates (n = batch * output pixels of `producer`) in the same
 * launch; batch = 1: an instance norm standing for BatchNorm2d(train) on a batch of one */
int t2v_batch_norm_finalize_running(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                                    const float* stats_partial, float eps, float* mean_rstd, float* running_mean,
                                    float* running_var, float momentum, int times);
/* The same finalize with a scratch buffer (additive to ABI 22): t2v_batch_norm_finalize, the running-statistics arguments of
 * t2v_batch_norm_finalize_running (running_mean and running_var both NULL: no update, momentum and times ignored), and
 * `scratch`, scratch_doubles doubles of device memory.  With a scratch buffer a launch that pools 2048 partials or more
 * spreads them over several groups of blocks, which leave their sums in the buffer, and a second kernel merges the groups
 * (and moves the running statistics); the tables are the same sums added in another order.  scratch == NULL: exactly the
 * call without it.  A scratch buffer shorter than t2v_norm_finalize_scratch_doubles(producer) is refused (T2V_ERR_INVALID)
 * before anything is launched.  batch = 1: an instance norm. */
size_t t2v_norm_finalize_scratch_doubles(const t2v_conv_desc* producer);
int t2v_batch_norm_finalize_scratch(t2v_ctx* ctx, void* stream, const t2v_conv_desc* producer, int batch,
                                    const float* stats_partial, float eps, float* mean_rstd, float* running_mean,
                                    float* running_var, float momentum, int times, double* scratch, size_t scratch_doubles);
int t2v_instance_norm_apply(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd,
                            const float* gamma, const float* beta, const float* res1,
                            const float* res2, float* y, long npix, int C, int relu);
/* Three more entries to the norm-apply kernels (additive to ABI 22): the launches a generator frame makes, on their own.
 * Each refuses on the host, before anything is launched (T2V_ERR_INVALID): a NULL required pointer, C % 4 != 0 (n % 4 != 0),
 * npix < 1, nimg < 1, gamma without beta or beta without gamma.
 *
 * t2v_instance_norm_apply_batch: t2v_instance_norm_apply on nimg images in one launch.  x, res1, res2 (nullable) and y hold
 * the images back to back, npix*C floats apart; mean_rstd holds nimg tables [C][2], 2*C floats apart; gamma and beta [C]
 * are shared by the images.  y == x is allowed.  Image i carries the bits of t2v_instance_norm_apply on its own operands.
 *
 * t2v_instance_norm_join: y = (norm_a(a_y) + a_res) + (norm_b(b_y) + b_res) in one pass, the encoder join: the bits of
 * two t2v_instance_norm_apply calls (relu 0, res1 = the side's res) followed by t2v_add.  Per side: y and res (both
 * required) nimg maps of npix*C floats, mean_rstd nimg tables of 2*C floats, gamma / beta [C] (both or neither).
 *
 * t2v_add: y[i] = a[i] + b[i], n floats, n % 4 == 0, 16-byte aligned pointers. */
int t2v_instance_norm_apply_batch(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd,
                                  const float* gamma, const float* beta, const float* res1,
                                  const float* res2, float* y, long npix, int C, int relu, int nimg);
int t2v_instance_norm_join(t2v_ctx* ctx, void* stream, const float* a_y, const float* a_mean_rstd, const float* a_gamma,
                           const float* a_beta, const float* a_res, const float* b_y, const float* b_mean_rstd,
                           const float* b_gamma, const float* b_beta, const float* b_res, float* y, long npix, int C,
                           int nimg);
int t2v_add(t2v_ctx* ctx, void* stream, const float* a, const float* b, float* y, long n);

/* ------------------------------------------------------------------------------------------
 * Flow-warp compositor.  Replaces SpatialGridSamplerBilinear_updateOutput (THCUNN.h:1048; F.
 * grid_sample functional.py:2046-2093, corner aligned, border padding) plus the blend
 * out = raw*w + warp(prev, flow)*(1-w) [SURVEY App. A.1].  fw = [H,W,3] (flow_x, flow_y in
 * pixels, weight).  prev: NHWC with storage stride prev_cs, the 3 channels starting at prev_c0.
 * warp_out (nullable) receives the warped image.  raw == NULL: plain `resample(prev, flow)` (the
 * train step's warp losses); the warped image goes to warp_out and, if given, out.
 *
 * _backward replaces SpatialGridSamplerBilinear_updateGradInput (THCUNN.h:1055: gradInput AND
 * gradGrid) fused with the blend's adjoint.  d_out: gradient of `out`, d_warp: gradient of
 * `warp_out` (either may be NULL, not both; d_out needs raw).  Writes d_raw [H,W,4] (nullable) =
 * d_out*w, d_fw [H,W,4] = (d flow_x, d flow_y, d weight, 0), and -- only if d_prev != NULL --
 * ACCUMULATES the image gradient into d_prev (same layout / channels as prev; the caller zero-fills;
 * atomic adds, so its summation order is not fixed).  Border rule as torch 0.4.1's kernel: bilinear
 * weights from the unclipped position, corner indices clipped into the image => the gradient with
 * respect to a coordinate is zero outside the image and exactly on its last row / column.
 * ------------------------------------------------------------------------------------------ */
int t2v_flow_warp_composite(t2v_ctx* ctx, void* stream, const float* raw, const float* fw,
                            const float* prev, int prev_cs, int prev_c0, float* out, float* warp_out,
                            int H, int W);
int t2v_flow_warp_composite_backward(t2v_ctx* ctx, void* stream, const float* d_out, const float* d_warp,
                                     const float* raw, const float* fw, const float* prev, int prev_cs,
                                     int prev_c0, float* d_raw, float* d_fw, float* d_prev, int H, int W);

/* AvgPool2d(3, stride 2, padding 1, count_include_pad=False) -- SpatialAveragePooling_
 * updateOutput (THCUNN.h:579; pooling.py:536-543).  NHWC, C % 4 == 0 not required. */
int t2v_avgpool3x3s2(t2v_ctx* ctx, void* stream, const float* x, float* y, int H, int W, int C);

/* ------------------------------------------------------------------------------------------
 * Convolution backward (accGradParameters of SpatialConvolutionMM / SpatialFullDilatedConvolution,
 * THCUNN.h:664,794).  `d` is the FORWARD conv descriptor.
 *   backward_weight: dW (packed layout, same as the packed forward weight) = sum over the batch and
 *       all pixels of dy (x) x through every filter tap; accumulate != 0 adds to dw_packed.
 *       Narrow high-resolution layers cut the pixel reduction into ranges (deterministic partials in
 *       `workspace`, summed in a fixed order: up to 4 partials by the last-arriving block of each (tap, n, c)
 *       tile inside the launch -- arrival tickets, write-through partials -- more by a reduce pass; the same
 *       bits either way).
 *       x: [batch][H][W][x_cs], dy: [batch][Hout][Wout][dy_cs].
 *   unpack_weight:   packed -> torch layout (inverse of t2v_conv_pack_weight).
 *   channel_sum:     out[c] = sum over pixels of x[.][c]  (bias gradient).
 * The data gradient needs no entry point of its own: it is a forward convolution with the adjoint
 * geometry (stride-2 conv <-> ConvTranspose with the same torch-layout weight; stride-1: flipped /
 * transposed weight, padding k-1-p) -- text2video_amd/backward.py builds those descriptors.
 * ------------------------------------------------------------------------------------------ */
size_t t2v_conv_backward_weight_workspace_floats(const t2v_conv_desc* d, int x_cs, int batch);
int t2v_conv2d_backward_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                               int x_cs, const float* dy, int dy_cs, float* dw_packed, int accumulate,
                               float* workspace /* NULL when ..._workspace_floats() == 0 */);
/* The same with the images of the batch `x_img_stride` / `dy_img_stride` floats apart instead of contiguous (ABI 14): the two
 * frames of a training clip live in buffers of their own, and one launch over both runs its blocks twice as long as two
 * launches (the kernel's fixed cost per block is ~8 of a 512<->1024 layer's 36 stage times per frame: 0.64 -> 0.73 of peak).
 * Any non-zero multiple of 4 bytes, negative included.  Only where t2v_conv_backward_weight_strided_supported() says so
 * (zero padding, no folded taps, GEMM rows that are whole 16-pixel stages: the stride-2 and transposed layers); workspace as
 * for t2v_conv2d_backward_weight at the same batch.  The result is that call's on the contiguous batch, bit for bit. */
int t2v_conv_backward_weight_strided_supported(const t2v_conv_desc* d, int x_cs, int dy_cs);
int t2v_conv2d_backward_weight_strided(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                                       int x_cs, long x_img_stride, const float* dy, int dy_cs, long dy_img_stride,
                                       float* dw_packed, int accumulate, float* workspace);
/* Weight gradient of a 3x3 stride-1 conv in the Winograd domain, F(4x4,3x3): dU[xi] = sum over tiles of
 * (A dy A^T)[xi] x (B^T x B)[xi] -- 36 pixel-reduction GEMMs of a quarter of the direct gradient's FLOPs -- then
 * dW = G^T dU G, written in TORCH layout [Cout][Cin][3][3] (accumulate: += ).  Where
 * t2v_conv_backward_weight_winograd_supported() says so (the forward conditions of F(4x4,3x3) plus dy_cs == Cout). */
int t2v_conv_backward_weight_winograd_supported(const t2v_conv_desc* d, int x_cs, int dy_cs);
size_t t2v_conv_backward_weight_winograd_workspace_floats(const t2v_conv_desc* d, int x_cs, int batch);
int t2v_conv2d_backward_weight_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, const float* x,
                                        int x_cs, const float* dy, int dy_cs, float* dw_torch, int accumulate,
                                        float* workspace);
/* The same in two stages, for callers that meet the images of one reduction at different times (the frames of a
 * training clip run through the same layer one after the other, and so do their backward passes): stages & 1
 * transforms images [b0, b0+nb) (x, dy point at image b0) into their slots of a workspace sized for `batch`
 * images; stages & 2 reduces over all `batch` slots and writes dW.  One reduction over K = batch * tiles instead
 * of `batch` short ones: the per-block fixed work of the 36 GEMMs and the filter transform are paid once. */
int t2v_conv2d_backward_weight_winograd_stages(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int b0,
                                               int nb, const float* x, int x_cs, const float* dy, int dy_cs,
                                               float* dw_torch, int accumulate, float* workspace, int stages);
/* The forward pass of such a layer in a train step (ABI 16): t2v_conv2d_forward_winograd (algo T2V_ALGO_WINOGRAD_F4, one image)
 * with V = B^T d B written into slot `slot` of the weight gradient's batch-wide workspace (`wgrad_workspace` sized by
 * t2v_conv_backward_weight_winograd_workspace_floats(d, x_cs, batch)) and read by the forward GEMM from there.  The backward
 * pass then calls _stages(stages & 1) with x == NULL for that image: only A dy A^T is transformed, the input transform of the
 * forward pass is not repeated (updateOutput and accGradParameters of THCUNN.h:664 share their im2col-equivalent). */
/* A dy A^T of one image into slot `slot`, for a layer followed by a norm (+ ReLU): `dy` is the gradient BEHIND the norm,
 * `conv_out` the layer's raw output, `sums` the (sum g, sum g*xhat) of t2v_instance_norm_backward[_affine] called with
 * dx == NULL.  The gradient in front of the norm (BatchNormalization_backward's gradInput, THCUNN.h:47) is formed per
 * loaded element -- inorm backward's arithmetic in its order, bit for bit -- and never stored: where the data gradient reads
 * A dy A^T from this workspace (t2v_conv2d_backward_data_winograd) nothing else needs it. */
int t2v_conv2d_backward_weight_winograd_dy_norm(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                                int x_cs, const float* conv_out, const float* dy, const float* mean_rstd,
                                                const float* gamma, const float* beta, int relu, const float* sums,
                                                float* workspace);
int t2v_conv2d_forward_winograd_keep_v(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, const float* x, int x_cs,
                                       const float* w_packed, const float* bias, float* y, int y_cs, float* stats_partial,
                                       float* workspace, float* wgrad_workspace, int batch, int slot);

/* Data gradient of a 3x3 stride-1 ReflectionPad(1) conv by the TRANSPOSED Winograd algorithm (updateGradInput of
 * SpatialConvolutionMM + SpatialReflectionPadding_updateGradInput, THCUNN.h:664,952): forward is V = B^T d B, M = U V,
 * Y = A^T M A; its transpose is dM = A dy A^T -- the tensor the Winograd-domain weight gradient builds anyway, read here
 * out of ITS workspace (slot `slot` of `batch`, after t2v_conv2d_backward_weight_winograd_stages(stages & 1)) -- then
 * dV = U^T dM (36 GEMMs over the layer's own T tiles, against (H+2)(W+2)/16 for the full-correlation form), the 6x6 patches
 * B dV B^T overlap-added into the padded gradient and folded by the reflect-pad adjoint.  `d` is the FORWARD descriptor;
 * H, W multiples of 4; ut_packed from t2v_conv_pack_weight_transposed (the forward weight's transform, transposed, no flip). */
int t2v_conv_backward_data_winograd_supported(const t2v_conv_desc* d, int x_cs, int dy_cs);
size_t t2v_conv_backward_data_winograd_weight_floats(const t2v_conv_desc* d, int x_cs);
size_t t2v_conv_backward_data_winograd_scratch_floats(const t2v_conv_desc* d, int x_cs);
int t2v_conv_pack_weight_transposed(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* w_forward_dev,
                                    float* packed_dev);
int t2v_conv2d_backward_data_winograd(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                      const float* wgrad_workspace, int x_cs, const float* ut_packed, float* scratch, float* dx);
/* The same with the FORWARD layer's own packed weights (t2v_conv_pack_weight of `d` with algo T2V_ALGO_WINOGRAD_F4 at the
 * same x_cs): U [36][Cout][x_cs] is the [K][N] operand of dV = dM U as it lies; the fixed-grid GEMM reads it in place (two
 * k rows of 128 columns per LDS-DMA instruction, ds_read_b64 per k), the same MFMA chains as with the transposed copy and so
 * the same bits -- no t2v_conv_pack_weight_transposed per optimiser step and no second copy of the transformed weights.
 * _takes_forward_weights: 1 where that form exists (whole 128 x 128 tiles on the fixed grid, Cout % 128 == 0, x_cs % 128 == 0). */
int t2v_conv_backward_data_winograd_takes_forward_weights(const t2v_conv_desc* d, int x_cs, int dy_cs);
int t2v_conv2d_backward_data_winograd_fw(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int batch, int slot,
                                         const float* wgrad_workspace, int x_cs, const float* u_forward_packed, float* scratch,
                                         float* dx);

int t2v_conv_unpack_weight(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* packed_dev,
                           float* w_torch_dev);
/* unpack_weight with a destination that may already hold a gradient: accumulate != 0 adds (w_torch += unpacked).  The
 * backward nodes of a layer used several times per step deliver straight into the parameter's slice of a flat
 * exchange bucket: the first writes, the later ones add -- what autograd's AccumulateGrad would do with an extra pass. */
int t2v_conv_unpack_weight_into(t2v_ctx* ctx, void* stream, const t2v_conv_desc* d, int x_cs, const float* packed_dev,
                                float* w_torch_dev, int accumulate);
/* dst = src (overwrite != 0) or dst += src; x *= s; zero-fill: the small-tensor ends of the gradient path (bias / affine
 * gradients into their bucket slice, averaging a summed bucket where the collective cannot, clearing the slice of a
 * parameter no backward node reached).  Replace ATen's add / mul / fill on the product path. */
int t2v_accumulate(t2v_ctx* ctx, void* stream, float* dst, const float* src, long n, int overwrite);
int t2v_scale(t2v_ctx* ctx, void* stream, float* x, long n, float s);
int t2v_zero(t2v_ctx* ctx, void* stream, void* ptr, size_t bytes);
/* src [C][2] (t2v_instance_norm_backward's dbeta_dgamma) -> dst0[c] (+)= src[c][0], dst1[c] (+)= src[c][1] */
int t2v_unzip2(t2v_ctx* ctx, void* stream, const float* src, float* dst0, float* dst1, int C, int overwrite);
int t2v_channel_sum(t2v_ctx* ctx, void* stream, const float* x, long npix, int C, int cs,
                    float* scratch /* >= 256*C floats */, float* out);
/* adjoint of ReflectionPad2d(pad): dxp [H+2pad][W+2pad][C] -> dx [H][W][C]  (SpatialReflectionPadding_updateGradInput) */
int t2v_reflect_pad_backward(t2v_ctx* ctx, void* stream, const float* dxp, float* dx, int H, int W, int C, int pad);
/* BatchNormalization_backward(train) / instance norm backward fused with the activation derivative:
 *   g = dy * act'(gamma*xhat+beta); dx = rstd*gamma*(g - mean(g) - xhat*mean(g*xhat)); dbeta_dgamma[c] = (sum g, sum g*xhat)
 * x = the conv output that was normalised, npix = pixels in the statistics (all images of a batch-norm batch),
 * relu as in t2v_instance_norm_apply, C % 4 == 0, scratch >= 128*C*2 floats.  dx may be NULL (ABI 16): the sums only. */
int t2v_instance_norm_backward(t2v_ctx* ctx, void* stream, const float* x, const float* dy, const float* mean_rstd,
                               const float* gamma, const float* beta, int relu, long npix, int C, float* scratch,
                               float* dx, float* dbeta_dgamma);
/* ... the same, with the two sums also delivered into the affine parameters' gradient tensors: d_beta[c] (+)= sum g,
 * d_gamma[c] (+)= sum g*xhat (overwrite != 0: written; else added) -- BatchNormalization_backward's gradBias / gradWeight
 * accumulation (THCUNN.h:47-62) without a pass of its own */
int t2v_instance_norm_backward_affine(t2v_ctx* ctx, void* stream, const float* x, const float* dy, const float* mean_rstd,
                                      const float* gamma, const float* beta, int relu, long npix, int C, float* scratch,
                                      float* dx, float* dbeta_dgamma, float* d_beta, float* d_gamma, int overwrite);
/* dpre = dy * act'(.) from the activation OUTPUT y; act: T2V_ACT_TANH, 2 = sigmoid, T2V_ACT_LRELU (slope), 0 = scale by slope,
 * 4 = the fused flow / weight head (T2V_ACT_FLOW_W) on [.,4] storage: ch 0,1 scale by slope, ch 2 sigmoid, ch 3 zero */
int t2v_act_backward(t2v_ctx* ctx, void* stream, const float* dy, const float* y, int act, float slope, long n,
                     float* dpre);
int t2v_avgpool3x3s2_backward(t2v_ctx* ctx, void* stream, const float* dy, float* dx, int H, int W, int C);
/* MaxPool2d(2,2), floor mode (torchvision vgg19 `features`, $SP/torchvision/models/vgg.py:82 cfg 'E' -- the VGG
 * perceptual loss): x [H][W][C] -> y [H/2][W/2][C]; backward routes dy to the first maximum of
 * each window in row-major order and writes zeros elsewhere. */
int t2v_maxpool2x2(t2v_ctx* ctx, void* stream, const float* x, float* y, int H, int W, int C);
int t2v_maxpool2x2_backward(t2v_ctx* ctx, void* stream, const float* x, const float* dy, float* dx, int H, int W, int C);
/* gradients of scale*sum((x-c)^2) and scale*sum|a-b| (wrt x / a) */
int t2v_sum_sq_diff_const_backward(t2v_ctx* ctx, void* stream, const float* x, float c, float scale, long n, float* dx);
int t2v_sum_abs_diff_backward(t2v_ctx* ctx, void* stream, const float* a, const float* b, float scale, long n, float* da);

/* ------------------------------------------------------------------------------------------
 * Train-step scalars.
 *   sum_sq_diff_const : sum (x - c)^2      -> out[0]   (MSECriterion_updateOutput THCUNN.h:356,
 *                       LSGAN target 1/0; the caller divides by n for 'elementwise_mean')
 *   sum_abs_diff      : sum |a - b|        -> out[0]   (AbsCriterion_updateOutput THCUNN.h:18)
 *   adam_step         : torch.optim.Adam.step ($SP/torch/optim/adam.py:48-98), one fused pass:
 *                       m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g*g ;
 *                       p -= lr*sqrt(1-b2^t)/(1-b1^t) * m / (sqrt(v) + eps)
 * `scratch` must hold >= 2048 floats.  Deterministic two-level reductions (no atomics).
 * ------------------------------------------------------------------------------------------ */
int t2v_sum_sq_diff_const(t2v_ctx* ctx, void* stream, const float* x, float c, long n, float* scratch, float* out);
int t2v_sum_abs_diff(t2v_ctx* ctx, void* stream, const float* a, const float* b, long n, float* scratch, float* out);
/* sum over pixels and the channels [c0, c0+C) of mask[pix] * |a - b| on [npix][cs] tensors (b NULL: zero target; mask
 * NULL: all ones) -- the numerator of vid2vid's MaskedL1Loss (flow, warp and weight losses; AbsCriterion THCUNN.h:18
 * on the masked operands); _backward: da = scale * mask * sign(a - b), zero in all other channels. */
int t2v_sum_abs_diff_masked(t2v_ctx* ctx, void* stream, const float* a, const float* b, const float* mask, long npix,
                            int c0, int C, int cs, float* scratch, float* out);
int t2v_sum_abs_diff_masked_backward(t2v_ctx* ctx, void* stream, const float* a, const float* b, const float* mask,
                                     float scale, long npix, int c0, int C, int cs, float* da);
/* All scalar loss terms of a train step in one launch (MSECriterion / AbsCriterion _updateOutput AND _updateGradInput,
 * THCUNN.h:356,365,18,27, for every term at once).  Term t is described by three device tables:
 *   term_ptrs[4t..]   = a, b, seed (device addresses; b / seed may be 0), n (op 0: pixels; op 1, 2: floats)
 *   term_ints[2t..]   = op, cs     op 0: sum (a[i*cs] - c)^2 over the pixels, seed[i*cs] = 2 s (a - c), pad channels 0
 *                                  op 1: sum |a - b|, seed = s sign(a - b);   op 2: no value, seed = 0
 *   term_floats[3t..] = c, s (seed scale), v (value scale: out[t] = v * sum)
 * Block b of the first kernel reduces `chunk` (a multiple of 4) elements of term chunk_term[b] starting at chunk_off[b] into
 * partials[b]; the chunks of a term are consecutive, term_chunk0[t] .. term_chunk0[t+1].  Deterministic (no atomics). */
int t2v_loss_terms(t2v_ctx* ctx, void* stream, const int64_t* term_ptrs, const int32_t* term_ints, const float* term_floats,
                   const int32_t* chunk_term, const int64_t* chunk_off, const int32_t* term_chunk0, int nterms, int nchunks,
                   int chunk, float* partials, float* out);
/* lr, betas and eps are doubles, as adam.py holds them: 1-beta, the bias corrections and the step size are evaluated
 * in double and rounded to fp32 once (adam.py:86-96 does the same through Python floats). */
int t2v_adam_step(t2v_ctx* ctx, void* stream, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                  long n, double lr, double beta1, double beta2, double eps, int step);

/* The same update for many tensors in ONE launch (all tables are DEVICE arrays): ptrs[t] = {param, grad, exp_avg,
 * exp_avg_sq} addresses of tensor t (grad 0: the tensor is skipped, as Adam skips parameters without gradient),
 * nelem[t] its length, step_size[t] = lr*sqrt(1-beta2^k)/(1-beta1^k) with that tensor's own step count k; the work is
 * cut into `nchunks` chunks of `chunk` elements: chunk c covers [chunk_off[c], chunk_off[c]+chunk) of tensor chunk_tensor[c]. */
int t2v_adam_step_multi(t2v_ctx* ctx, void* stream, const int64_t* ptrs, const int64_t* nelem, const float* step_size,
                        const int32_t* chunk_tensor, const int64_t* chunk_off, int nchunks, int chunk, double beta1,
                        double beta2, double eps);

/* layout / dtype plumbing on the device.  nchw_to_nhwc: channels [C, dst_cs) of dst are written as zero.  nhwc_to_nchw:
 * channels [C, src_cs) of src are ignored. */
int t2v_nchw_to_nhwc(t2v_ctx* ctx, void* stream, const float* src, float* dst, int C, int H, int W, int dst_cs);
int t2v_nhwc_to_nchw(t2v_ctx* ctx, void* stream, const float* src, float* dst, int C, int H, int W, int src_cs);
/* ToTensor + Normalize(.5,.5) ($SP/torchvision/transforms/functional.py:38-60,206-208) of a
 * uint8 HWC(3) pose map into channels [c0,c0+3) of an NHWC fp32 buffer; the other channels of dst are not touched */
int t2v_pose_u8_to_f32(t2v_ctx* ctx, void* stream, const uint8_t* src_hwc3, float* dst, long npix, int dst_cs, int c0);
/* util.tensor2im [SURVEY 3.2]: uint8((x+1)/2*255 clipped), same layout */
int t2v_tensor2im_u8(t2v_ctx* ctx, void* stream, const float* x, uint8_t* y, long n);
/* dst[pix][dst_c0 + c] = src[pix][src_c0 + c] for c < nc; every other channel of src is ignored, of dst not touched */
int t2v_copy_channels(t2v_ctx* ctx, void* stream, const float* src, int src_cs, int src_c0, float* dst,
                      int dst_cs, int dst_c0, int nc, long npix);

/* ------------------------------------------------------------------------------------------
 * Whole-frame generator.  Replaces CompositeGenerator.forward / CompositeLocalGenerator.forward
 * [SURVEY App. A.1/A.2] as called by Vid2VidModelG.generate_frame_infer.
 *
 * Layer order of `layers` (conv layers only; gamma/beta are the affine params of the norm that
 * follows the conv, NULL for InstanceNorm(affine=False) and for the heads):
 *   global (is_local=0):
 *     down_seg: c7, d x n_downsample, RB x (n_blocks - n_blocks/2) [2 convs each]
 *     down_img: same
 *     res_img : RB x (n_blocks/2)        up_img: u x n_downsample       final_img: c7
 *     if !no_flow: res_flow RB x (n_blocks/2), up_flow u x n_downsample,
 *                  final_flow_w: ONE c7 with 3 outputs = cat(model_final_flow, model_final_w)
 *   local (is_local=1, ngf = ngf of this scale):
 *     down_seg: c7, d      down_img: c7, d
 *     up_img: RB x n_blocks, u         final_img: c7
 *     if !no_flow: up_flow: RB x n_blocks, u ; final_flow_w
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    int H, W;           /* multiples of 2^n_downsample */
    int input_nc;       /* pose channels x n_frames_G (9)   -> storage round_up4 (12) */
    int prev_nc;        /* (n_frames_G-1) x output_nc (6)   -> storage round_up4 (8)  */
    int output_nc;      /* 3 */
    int ngf;
    int n_downsample;
    int n_blocks;
    int no_flow;
    int norm_affine;    /* 1: BatchNorm2d(affine) in train mode, N=1  ==  IN + gamma/beta */
    int is_local;       /* 0: CompositeGenerator, 1: CompositeLocalGenerator */
    float flow_multiplier; /* 20 * 2^scale */
    float eps;          /* 1e-5 */
    int conv_algo;      /* ResnetBlock convs: 0 = best supported of F(4x4,3x3) > F(2x2,3x3) > direct;
                         * 1 = direct only; 2 = F(2x2,3x3) or direct; 3 (ABI 22) = as 0, with every ResnetBlock conv that 0
                         * runs as F(4x4,3x3) and t2v_conv_winograd_bf16x2_supported() accepts as
                         * T2V_ALGO_WINOGRAD_F4_BF16X2 (the reduced-precision mode; workspace sizes are those of 0);
                         * 4 = as 3, and every stride-2 / transposed layer that 0 runs as T2V_ALGO_POLYPHASE and
                         * t2v_conv_polyphase_bf16x2_supported() accepts as T2V_ALGO_POLYPHASE_BF16X2 (same sizes);
                         * 5 = as 4, and the stride-2 / transposed layers that 4 leaves T2V_ALGO_DIRECT, where
                         * t2v_conv_direct_bf16x2_supported of t2v_bf16x2.h accepts them and the class measured faster (both
                         * channel counts >= 128: the 128 <-> 256 layers), as
                         * T2V_ALGO_DIRECT_BF16X2 (no size grows; such a layer leaves one statistics partial per 128 pixels) */
} t2v_gen_desc;

typedef struct {
    const float* w;      /* packed by t2v_conv_pack_weight */
    const float* bias;   /* [Cout] */
    const float* gamma;  /* [Cout] or NULL */
    const float* beta;   /* [Cout] or NULL */
} t2v_layer;

typedef struct {
    const float* pose;              /* [H,W,round_up4(input_nc)] */
    const float* prev;              /* [H,W,round_up4(prev_nc)]  */
    const float* coarse_img_feat;   /* local only: [H/2,W/2,2*ngf] */
    const float* coarse_flow_feat;  /* local only, !no_flow */
    int use_raw_only;
    float* out;        /* [H,W,4] final frame, channels 0..2 (channel 3 = 0) */
    float* raw;        /* nullable [H,W,4] img_raw */
    float* flow_w;     /* nullable [H,W,4] flow_x, flow_y, weight */
    float* img_feat;   /* nullable [H,W,ngf] */
    float* flow_feat;  /* nullable [H,W,ngf] */
} t2v_gen_io;

int t2v_generator_num_layers(const t2v_gen_desc* d);
/* conv descriptor of layer i (what to pack weights with -- its `algo` depends on d->H, d->W and
 * d->conv_algo) and its input storage stride */
int t2v_generator_layer_desc(const t2v_gen_desc* d, int i, t2v_conv_desc* out, int* x_cs);
size_t t2v_generator_workspace_bytes(const t2v_gen_desc* d);
int t2v_generator_forward(t2v_ctx* ctx, void* stream, const t2v_gen_desc* d, const t2v_layer* layers,
                          int n_layers, const t2v_gen_io* io, void* workspace, size_t ws_bytes);

/* `batch` INDEPENDENT recurrences advanced in lock-step on one GPU: the frames of `batch` sequences (the reference
 * always generates two per utterance -- tmp and tmp_smooth, text2video_audio.sh:24-31 -- and BASELINE configs[2] has
 * more chunks than GPUs on 1-4 GPUs) through ONE pass of the layer list.  ios[i] is image i's io block (every image
 * its own pose window, previous frames, use_raw_only and outputs).  The ResnetBlock chains (Winograd F(4x4,3x3)) run
 * batched: the transforms carry the image index in their grid, and the 36 GEMMs see batch x T tile rows per weight
 * matrix instead of T -- the skinny M = 256 of one 64x64 bottleneck becomes 512 at batch 2; norm statistics stay
 * per image (instance norm), so each image's frame is the frame t2v_generator_forward computes for it.  The
 * remaining layers are launched image by image.  Workspace from ..._workspace_bytes_batch(d, batch). */
#define T2V_MAX_BATCH 8
size_t t2v_generator_workspace_bytes_batch(const t2v_gen_desc* d, int batch);
int t2v_generator_forward_batch(t2v_ctx* ctx, void* stream, const t2v_gen_desc* d, const t2v_layer* layers,
                                int n_layers, const t2v_gen_io* ios, int batch, void* workspace, size_t ws_bytes);

/* ------------------------------------------------------------------------------------------
 * Dense optical flow (ABI 20): stands in for upstream's `flowNet(real_B, real_B_prev)` -- FlowNet2, whose code and weights
 * are not in the reference tree -- as the producer of the train step's reference flow.  It is NOT FlowNet2: a classical
 * coarse-to-fine iterative Lucas-Kanade estimate on the grey images, fully local (no global solve, no atomics: two calls
 * give the same bits).  The flow lives on cur's grid and points into prev, cur(x, y) ~ prev(x + u, y + v), in pixels: what
 * t2v_flow_warp_composite / upstream's resample take.
 *   grey = (R + G + B) / 3 of the three channels from c0 of an NHWC fp32 tensor with channel stride cs;
 *   pyramid: level l+1 = AvgPool2d(3, 2, 1, count_include_pad=False) of level l.  levels == 0: the default rule, start at 1
 *     and halve while levels < 6 and min(ceil(h/2), ceil(w/2)) >= 16 (512x512: 6, 64x96: 3, 48x40: 2);
 *   per level, coarsest first: the flow starts at zero (coarsest) or at 2 * bilinear(coarser flow; x/2, y/2); gx, gy =
 *     central differences of cur (replicate border); with n = (2r+1)^2 and box = window SUM (zeros outside the image)
 *     Sxx = box(gx^2) + lambda n, Syy = box(gy^2) + lambda n, Sxy = box(gx gy), det = Sxx Syy - Sxy^2 (>= (lambda n)^2);
 *   per iteration: it = prev(x + u, y + v) - cur (bilinear, position clamped into the image); bx = -box(gx it),
 *     by = -box(gy it); du = (Syy bx - Sxy by) / det, dv = (Sxx by - Sxy bx) / det; the step is cut to length 1
 *     (divide by max(1, |(du, dv)|)); then u and v are replaced by their 3x3 mean over the taps inside the image.
 * flow_out: [H][W][4] = (u, v, 0, 0).  workspace: t2v_optical_flow_workspace_floats(H, W, levels) floats (0 for a shape the
 * call refuses), 8-byte aligned, any content.  Refused, with nothing launched: H or W < 8, radius outside 1..7, iters < 1,
 * lambda <= 0, more than 8 levels.  No allocation, no host synchronisation and no atomics inside the call.  Every gather
 * coordinate is clamped (fminf / fmaxf) before it becomes an index: a non-finite input cannot address outside a plane.
 * Kernel launches per call, fixed by (levels, iters) alone:  levels * (iters + 1) + 1
 *   = levels (grey + pyramid of both images) + levels * iters (one per level and iteration) + 1 (output).
 * ------------------------------------------------------------------------------------------ */
size_t t2v_optical_flow_workspace_floats(int H, int W, int levels);
int t2v_optical_flow(t2v_ctx* ctx, void* stream, const float* cur, int cur_cs, int cur_c0, const float* prev, int prev_cs,
                     int prev_c0, int H, int W, int levels, int iters, int radius, float lambda, float* workspace,
                     float* flow_out);

/* The same flow on the delivered bytes (additive to ABI 22): cur, prev are uint8 HWC frames [H][W][cs] with cs in {3, 4}
 * chosen per image (a generated frame comes with stride 4, a decoded real frame with 3); channels 0..2 are read.
 *   grey = (x0 + x1 + x2) / 3.0f with x_c = (v_c / 255.0f - 0.5f) / 0.5f, the value t2v_pose_u8_to_f32 forms: the result is
 *   bit for bit t2v_optical_flow on the fp32 images that call makes of the same bytes.
 * Only the launch that forms the grey images differs: workspace size (t2v_optical_flow_workspace_floats), launch count,
 * refusals (plus a channel stride outside {3, 4}) and the clamped-gather guarantee are those of t2v_optical_flow.
 * uint8 input cannot be non-finite and det >= (lambda n)^2 > 0, so every flow this call returns is finite. */
int t2v_optical_flow_u8(t2v_ctx* ctx, void* stream, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs, int H,
                        int W, int levels, int iters, int radius, float lambda, float* workspace, float* flow_out);

/* t2v_optical_flow_refined / t2v_optical_flow_refined_u8 -- this estimate with a Horn-Schunck refinement at every pyramid
 * level, which fills textureless regions (additive to ABI 22) -- are declared and defined in t2v_flow_refine.h, the header
 * of libt2v_flow.so, a library of its own that links this one. */

/* ------------------------------------------------------------------------------------------
 * Image resampling for the training loader (ABI 21): PIL's `Image.resize` of a clip's frames, the crop and
 * torchvision's ToTensor + Normalize(.5, .5) in ONE launch, bit for bit what the CPU path computes.
 *   src: T uint8 frames [T][h][w][3] of one size (device memory).
 *   The resampler is separable and table-driven; the tables are device pointers the host built (the library knows no
 *   filter).  Per axis, for every coordinate i of the WHOLE resized image (out_w / out_h entries):
 *     first[i], count[i]: the taps are source indices first[i] .. first[i] + count[i] - 1 (count[i] <= k);
 *     coef[i][k] (int32): their weights, scaled by 2^22.
 *   Arithmetic, Pillow's 8-bit resampler (int32 throughout), in this order:
 *     horizontal:  b(x', y)  = clip8((2^21 + sum_j src(x_first[x'] + j, y) * x_coef[x'][j]) >> 22)
 *     vertical:    u(x', y') = clip8((2^21 + sum_j   b(x', y_first[y'] + j) * y_coef[y'][j]) >> 22)
 *   with an arithmetic shift and clip8 = saturation to [0, 255]: the vertical pass runs on the horizontal pass's BYTES.
 *   An axis that keeps its size takes the identity table (one tap of 2^22), as Pillow skips that pass.
 *   dst: fp32 [T][crop_h][crop_w][dst_cs]; pixel (x, y) of frame t receives u(crop_x + x, crop_y + y) in channels
 *   [dst_c0, dst_c0 + 3) as (u * (1.0f / 255.0f) - 0.5f) / 0.5f; the other channels are not touched.  That is train.py's
 *   (u8.float() / 255.0 - 0.5) / 0.5 as ATen evaluates it on the device (a division by a host scalar is a multiplication by
 *   its fp32 reciprocal there), i.e. the numbers the default loader trains on; t2v_pose_u8_to_f32 forms the true quotient
 *   u / 255.0f (torchvision's ToTensor on the CPU), which is one ulp away for some of the 256 bytes.
 * Only the columns and source rows the crop window needs are computed.  One launch; no allocation, no host
 * synchronisation, no atomics: two calls give the same bits.
 * Limits: kx, ky <= T2V_RESAMPLE_MAX_TAPS (Pillow's bicubic down to 1/8 of the source size per axis; 17 taps = 1/4), and
 * the taps of 8 consecutive output rows within 96 source rows, which every resampler table within the tap limit keeps.
 * Refused with T2V_ERR_INVALID and nothing launched: more taps, T outside 1..65535, an empty frame, a crop window outside
 * the resized image, dst_c0 + 3 > dst_cs -- the caller resizes on the CPU.  Table entries are clamped before they address
 * memory: wrong tables give wrong values, not a fault.
 * ------------------------------------------------------------------------------------------ */
#define T2V_RESAMPLE_MAX_TAPS 33
int t2v_resample_crop_normalize_u8(t2v_ctx* ctx, void* stream, const uint8_t* src, int T, int h, int w,
                                   const int32_t* x_first, const int32_t* x_count, const int32_t* x_coef, int kx, int out_w,
                                   const int32_t* y_first, const int32_t* y_count, const int32_t* y_coef, int ky, int out_h,
                                   int crop_x, int crop_y, int crop_w, int crop_h, float* dst, int dst_cs, int dst_c0);

/* ------------------------------------------------------------------------------------------
 * Picture-quality sums (additive to ABI 22): what PSNR, the mean absolute error and SSIM of two uint8 images are formed
 * from, over the whole frame and up to T2V_METRICS_MAX_BOXES boxes, in two launches (vid2vid/test.py --metrics,
 * python -m text2video_amd.evaluate).
 *   a, b: [H][W][cs] uint8 device images, cs in {3, 4} chosen per image (a generated frame comes with stride 4, a decoded
 *   real frame with 3); channels 0..2 are compared.
 *   boxes: HOST memory, [nbox][4] = y0, y1, x0, x1 (half-open rows / columns); read before the call returns.
 *   Region 0 is the whole frame, region r = 1..nbox is box r-1.  out (device, doubles) row r = {sse, sad, ssim_sum, ssim_n}:
 *     sse = sum (a - b)^2 and sad = sum |a - b| over the region's pixels and 3 channels: exact integers (< 2^53);
 *     ssim_sum = sum of the SSIM index s over the window positions whose WHOLE 11x11 window lies inside the region, and the
 *       3 channels -- so a box's SSIM is the SSIM of the cropped pair; ssim_n = 3 (h - 10)(w - 10) of them, 0 for a region
 *       narrower than 11 in either direction (ssim_sum is then 0).
 *   s (Wang, Bovik, Sheikh, Simoncelli 2004), per channel on the 8-bit values, in float64 throughout:
 *     window w = outer product of g[i] = exp(-(i - 5)^2 / 4.5), i = 0..10 (sigma 1.5), g normalised to sum 1;
 *     mx = sum w x, my = sum w y, vx = sum w x^2 - mx^2, vy = sum w y^2 - my^2, cxy = sum w x y - mx my;
 *     C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2;  s = (2 mx my + C1)(2 cxy + C2) / ((mx^2 + my^2 + C1)(vx + vy + C2)).
 *     The window sums run separably (rows, then columns) with fused multiply-adds; another float64 order of the same sums
 *     differs by ~1e-13 of s, a float32 evaluation by ~1e-5 on smooth images (the cancellation in vx, vy, cxy).
 *   scratch: t2v_image_metrics_scratch_doubles(H, W, nbox) doubles of device memory (one partial per 32x32 tile, region and
 *   sum; 0 for a shape the call refuses), any content; the caller vouches for its size.
 * Every tile's partial sums are added in a fixed order by the second launch: no atomics, two calls give the same bits, and
 * row 0 has the same bits whatever boxes are passed.  Rows of `out` past 1 + nbox are not touched.  No allocation, no host
 * synchronisation.  Refused with T2V_ERR_INVALID and nothing launched: a channel stride outside {3, 4}, H or W outside
 * 1..T2V_METRICS_MAX_SIDE, nbox outside 0..T2V_METRICS_MAX_BOXES, an empty box or one that leaves the frame.
 * ------------------------------------------------------------------------------------------ */
#define T2V_METRICS_MAX_BOXES 3
#define T2V_METRICS_MAX_SIDE 8192
size_t t2v_image_metrics_scratch_doubles(int H, int W, int nbox);
int t2v_image_metrics_u8(t2v_ctx* ctx, void* stream, const uint8_t* a, int a_cs, const uint8_t* b, int b_cs, int H, int W,
                         const int32_t* boxes /* HOST, [nbox][4] */, int nbox, double* scratch, double* out /* [1+nbox][4] */);

/* ------------------------------------------------------------------------------------------
 * Temporal-consistency sums (additive to ABI 22): how a generated pair of consecutive frames (a_cur, a_prev) moves, read
 * against the real pair (b_cur, b_prev) of the same two instants, over the whole frame and up to T2V_METRICS_MAX_BOXES
 * boxes, in two launches (vid2vid/test.py --metrics_temporal, python -m text2video_amd.evaluate --temporal).
 *   a_cur, a_prev, b_cur, b_prev: [H][W][cs] uint8 device images, cs in {3, 4} chosen per image; channels 0..2 are read.
 *   flow_fwd, flow_bwd, flow_a: fp32 [H][W][4] = (u, v, -, -) in pixels, the layout t2v_optical_flow writes:
 *     flow_fwd on b_cur's grid, pointing into b_prev; flow_bwd on b_prev's grid, pointing into b_cur; flow_a on a_cur's
 *     grid, pointing into a_prev -- flow_a may be NULL.
 *   boxes: HOST memory, [nbox][4] = y0, y1, x0, x1 (half-open); regions and their refusals are those of
 *   t2v_image_metrics_u8: region 0 is the whole frame, region r = 1..nbox is box r-1.
 *   out (device, doubles) row r = {n_valid, warp_sse_a, warp_sse_b, n_flow, epe_sum, tdiff_sse} of region r.
 * Everything in float64, evaluated from the fp32 / uint8 inputs.  For a pixel p = (x, y) of the region, f = flow_fwd(p):
 *   q = (x + f.u, y + f.v); p is INSIDE when f is finite and 0 <= q.x <= W-1 and 0 <= q.y <= H-1;
 *   bilinear(I; q) = (1-fy)((1-fx) I(x0,y0) + fx I(x1,y0)) + fy((1-fx) I(x0,y1) + fx I(x1,y1)), x0 = floor(q.x),
 *     x1 = min(x0+1, W-1), fx = q.x - x0, likewise in y;  bq = bilinear(flow_bwd; q);
 *   p is VALID when it is inside, bq is finite and |f + bq|^2 <= 0.01 (|f|^2 + |bq|^2) + 0.5 -- the forward-backward check
 *     of Sundaram, Brox, Keutzer 2010, the occlusion mask Ruder et al. 2016 and Lai et al. 2018 use for their warping error;
 *   n_valid = number of valid pixels;
 *   warp_sse_a = sum over valid p and the 3 channels of (a_cur_c(p) - bilinear(a_prev_c; q))^2;
 *   warp_sse_b = the same sum on b: the floor the flow's own error leaves on the real pair, what warp_sse_a is read against;
 *   n_flow, epe_sum: over ALL pixels of the region where f and ga = flow_a(p) are both finite, their number and
 *     sum sqrt((ga.u - f.u)^2 + (ga.v - f.v)^2) -- the tOF of Chu et al. 2020 (TecoGAN); both 0 when flow_a is NULL;
 *   tdiff_sse = sum over ALL pixels and the 3 channels of ((a_cur - a_prev) - (b_cur - b_prev))^2, an exact integer
 *     (< 2^53): the flicker term that depends on no flow.  n_valid and n_flow are exact integers too.
 *   scratch: t2v_temporal_metrics_scratch_doubles(H, W, nbox) doubles of device memory (one partial per 32x16 tile, region
 *   and quantity; 0 for a shape the call refuses), any content; the caller vouches for its size.
 * Every gather coordinate is clamped (fmin / fmax) before it becomes an index: a non-finite or huge flow value makes its
 * pixel invalid / not counted and can never address outside a plane.  Every tile's partial sums are added in a fixed order
 * by the second launch: no atomics, two calls give the same bits, and row 0 has the same bits whatever boxes are passed.
 * Rows of `out` past 1 + nbox are not touched.  No allocation, no host synchronisation.  Refused with T2V_ERR_INVALID and
 * nothing launched: a null image, flow_fwd, flow_bwd, scratch or out, a channel stride outside {3, 4}, H or W outside
 * 1..T2V_METRICS_MAX_SIDE, nbox outside 0..T2V_METRICS_MAX_BOXES, an empty box or one that leaves the frame.
 * ------------------------------------------------------------------------------------------ */
size_t t2v_temporal_metrics_scratch_doubles(int H, int W, int nbox);
int t2v_temporal_metrics_u8(t2v_ctx* ctx, void* stream, const uint8_t* a_cur, int a_cur_cs, const uint8_t* a_prev, int a_prev_cs,
                            const uint8_t* b_cur, int b_cur_cs, const uint8_t* b_prev, int b_prev_cs, const float* flow_fwd,
                            const float* flow_bwd, const float* flow_a /* may be NULL */, int H, int W,
                            const int32_t* boxes /* HOST, [nbox][4] */, int nbox, double* scratch, double* out /* [1+nbox][6] */);

/* ------------------------------------------------------------------------------------------
 * Training visuals (additive to ABI 22): the pictures a training run shows of one frame (vid2vid/train.py --display_web,
 * text2video_amd/train_display.py), up to T2V_VISUALS_MAX_PANELS panels rendered as uint8 RGB in two launches.
 *   panel_ptrs: HOST memory, npanels device pointers to fp32 NHWC tensors [H][W][cs]; panel_ints: HOST memory,
 *   [npanels][3] = kind, c0, cs: the panel reads channels from c0 on of a pixel of cs floats.  Both are read before the call
 *   returns.  out: [npanels][H/scale][W/scale][3] uint8 device memory, 4-byte aligned.
 *   T2V_VISUALS_IMAGE (channels c0..c0+2): the byte t2v_tensor2im_u8 writes, uint8((x+1)/2*255 clipped), fp32.
 *   T2V_VISUALS_UNIT (channel c0): uint8(x*255 clipped to [0,255]) in fp32, NaN -> 0, the byte repeated as R, G and B.
 *   T2V_VISUALS_FLOW (channels c0, c0+1 = u, v in pixels): HSV with saturation 1, hue = direction, value = magnitude
 *   normalised over the panel, in float64 from the fp32 inputs.  A pixel is finite when u and v are; m = sqrt(u^2 + v^2);
 *     lo, hi = min, max of m over the panel's finite pixels (every FLOW panel has its own);  V = (m - lo) / (hi - lo), and
 *     V = 0 for a non-finite pixel, for a panel without a finite pixel and for hi == lo;
 *     a = atan2(v, u), + 2 pi if negative;  h6 = 3 a / pi;  i = floor(h6) mod 6;  f = h6 - floor(h6);
 *     (r, g, b) = (1,f,0), (1-f,1,0), (0,1,f), (0,1-f,1), (f,0,1), (1,0,1-f) for i = 0..5;  byte = floor(255 V c + 0.5).
 *     (The colour wheel of upstream's util.tensor2flow as recalled; pinned to this definition, not to OpenCV's bytes.)
 *   scale in {1, 2, 4}: every output byte = (sum of the scale x scale full-resolution bytes above + scale^2 / 2) / scale^2 in
 *   integers; H and W must be multiples of scale.
 *   scratch: scratch_doubles >= t2v_train_visuals_scratch_doubles(H, W, npanels) doubles of device memory, any content
 *   (the per-slice min / max of the FLOW panels; 0 for a shape the call refuses).
 * Launch 1 writes every FLOW panel's per-block min / max (skipped without a FLOW panel), launch 2 reduces them per block
 * and renders: min and max do not depend on the order, so two calls give the same bytes.  No atomics, no allocation, no
 * host synchronisation.  Refused with T2V_ERR_INVALID, nothing launched and `out` untouched: a null pointer, npanels
 * outside 1..T2V_VISUALS_MAX_PANELS, H or W outside 1..T2V_METRICS_MAX_SIDE, scale outside {1, 2, 4} or not dividing H and
 * W, an unknown kind, c0 < 0 or c0 + the kind's channels > cs, an `out` that is not 4-byte aligned, a scratch that is too
 * small.
 * ------------------------------------------------------------------------------------------ */
#define T2V_VISUALS_MAX_PANELS 8
enum { T2V_VISUALS_IMAGE = 0, T2V_VISUALS_UNIT = 1, T2V_VISUALS_FLOW = 2 };
size_t t2v_train_visuals_scratch_doubles(int H, int W, int npanels);
int t2v_train_visuals_u8(t2v_ctx* ctx, void* stream, const float* const* panel_ptrs /* HOST, [npanels] */,
                         const int32_t* panel_ints /* HOST, [npanels][3] = kind, c0, cs */, int npanels, int H, int W, int scale,
                         double* scratch, size_t scratch_doubles, uint8_t* out /* [npanels][H/scale][W/scale][3] */);

/* ------------------------------------------------------------------------------------------
 * Host plumbing (ABI 14): device buffers, pinned host buffers, copies, streams and events for a host that has no HIP
 * binding of its own -- the reference's hosts got these from THC (THCudaMalloc / THCudaFree
 * $SP/torch/lib/include/THC/THCGeneral.h:143-144, THCudaHostAlloc :147, THCState_getCurrentStream :105,
 * THCCachingHostAllocator.h).  `vid2vid/test.py` runs its frame loop on these alone (text2video_amd/leantorch.py:
 * the one-shot command no longer pays for `import torch`); a host that does have an allocator (PyTorch in the tests,
 * the trainer and the resident server) passes its own pointers and never calls them.  All of them make ctx's device
 * current.  Nothing here caches: t2v_device_malloc is hipMalloc.
 * ------------------------------------------------------------------------------------------ */
int t2v_device_malloc(t2v_ctx* ctx, size_t bytes, void** out);
int t2v_device_free(t2v_ctx* ctx, void* ptr);
int t2v_host_malloc(t2v_ctx* ctx, size_t bytes, void** out);      /* page-locked, portable */
int t2v_host_free(t2v_ctx* ctx, void* ptr);
enum { T2V_COPY_H2D = 1, T2V_COPY_D2H = 2, T2V_COPY_D2D = 3 };
/* enqueued on `stream`; asynchronous to the host when the host side is page-locked (a pageable source is staged by the
 * runtime and the call returns when the host buffer may be reused) */
int t2v_memcpy(t2v_ctx* ctx, void* stream, void* dst, const void* src, size_t bytes, int kind);
int t2v_stream_create(t2v_ctx* ctx, void** out);                  /* non-blocking with respect to the null stream */
int t2v_stream_destroy(t2v_ctx* ctx, void* stream);
int t2v_stream_synchronize(t2v_ctx* ctx, void* stream);
int t2v_event_create(t2v_ctx* ctx, void** out);                   /* no timing */
int t2v_event_record(t2v_ctx* ctx, void* event, void* stream);
int t2v_event_synchronize(t2v_ctx* ctx, void* event);
int t2v_event_destroy(t2v_ctx* ctx, void* event);
int t2v_device_synchronize(t2v_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* T2V_H_ */
