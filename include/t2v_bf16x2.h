/* t2v_bf16x2.h -- the entry points of T2V_ALGO_DIRECT_BF16X2 (t2v.h), the direct 3x3 stride-2 / transposed convolution in
 * split-bf16 arithmetic.  A companion of t2v.h: same library (libt2v_hip.so), same ABI version, same conventions; the form
 * itself runs through t2v_conv2d_forward_winograd* and t2v_generator_forward* of t2v.h.  Its kernels are libt2v_split.so's, which
 * libt2v_hip.so loads as a dependency. */
#ifndef T2V_BF16X2_H_
#define T2V_BF16X2_H_

#include "t2v.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1 where `d` (algo ignored) can run as T2V_ALGO_DIRECT_BF16X2: 3x3, stride 2, zero padding 1, no activation; x_cs == Cin,
 * Cin % 32 == 0, Cout % 128 == 0; a conv on an even map or a transposed conv with output_padding 1 on any map (H, W >= 1); the
 * input map, the output map and the largest weight block (Cout * 9 * Cin floats, * 4 for a transposed conv) each below
 * 0x7fff0000 bytes, the out-of-range marker of the kernel's 32-bit byte offsets.  Every backward, weight-gradient and
 * data-gradient entry and query refuses a descriptor whose algo is T2V_ALGO_DIRECT_BF16X2. */
int t2v_conv_direct_bf16x2_supported(const t2v_conv_desc* d, int x_cs);
/* t2v_instance_norm_apply without residuals, storing what a T2V_ALGO_DIRECT_BF16X2 layer reads: for every channel pair of the
 * result the dwords {hi.x, hi.y | lo.x, lo.y} (hi = bf16_rne(v), lo = bf16_rne(v - hi)) in the 8 bytes of the pair -- bit for
 * bit the split of what t2v_instance_norm_apply stores.  y == x is allowed.  C % 4 == 0, gamma and beta both or neither. */
int t2v_instance_norm_apply_bf16x2(t2v_ctx* ctx, void* stream, const float* x, const float* mean_rstd, const float* gamma,
                                   const float* beta, float* y, long npix, int C, int relu);

#ifdef __cplusplus
}
#endif

#endif /* T2V_BF16X2_H_ */
