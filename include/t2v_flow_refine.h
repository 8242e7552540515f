/* t2v_flow_refine.h -- C ABI of libt2v_flow.so: t2v_optical_flow of t2v.h (dense coarse-to-fine Lucas-Kanade flow) with a
 * variational refinement of every level's estimate.  The library stands beside libt2v_hip.so, which it links: the context is
 * that library's t2v_ctx, a refusal returns T2V_ERR_INVALID (-1) and leaves its message where t2v_last_error() of t2v.h
 * reads it, a HIP error returns T2V_ERR_HIP (-2); 0 is success.  Its kernels are its own: the LK kernels compiled from
 * the text libt2v_hip.so compiles them from, and the refinement's. */
#ifndef T2V_FLOW_REFINE_H_
#define T2V_FLOW_REFINE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_FLOW_REFINE_ABI_VERSION 1

typedef struct t2v_ctx t2v_ctx;      /* t2v_create of t2v.h */

/* The LK estimate with a variational (Horn-Schunck) refinement at every pyramid level: a global
 * smoothness term fills the textureless regions that the local estimate leaves to its 3x3 smoothing.  Still NOT FlowNet2.
 * Grey images, pyramid, level rule, gx, gy, the LK iterations and the x2 bilinear hand-down are exactly those of
 * t2v_optical_flow.  After a level's LK iterations (smoothing included) have produced (u0, v0), the level goes on:
 *   It0 = prev_l(x + u0, y + v0) - cur_l (bilinear, position clamped into the image: the gather of the LK iteration);
 *   (u, v) = (u0, v0); then refine_iters Jacobi steps -- every pixel reads the previous iterate only:
 *     ub = (N + S + E + W) / 6 + (NE + NW + SE + SW) / 12 of u, neighbour indices clamped to the image (replicate; the centre
 *       has no weight), vb the same of v;
 *     t  = (gx (ub - u0) + gy (vb - v0) + It0) / (alpha^2 + gx^2 + gy^2);
 *     u  = ub - gx t,  v = vb - gy t;
 *   the refined (u, v) -- not smoothed again -- is what the next finer level starts from (2 * bilinear(.; x/2, y/2)) and,
 *   at level 0, what flow_out receives.  The kernels multiply by 1/6, 1/12 and by 1 / (alpha^2 + gx^2 + gy^2), formed once.
 * Grey values lie in [-1, 1]; alpha = 0.2 and refine_iters = 64 are the values the documents' figures were taken with.
 * refine_iters == 0: bit for bit t2v_optical_flow / t2v_optical_flow_u8 (the same launches).
 * iters_per_launch: Jacobi steps per kernel launch, 1..T2V_FLOW_REFINE_MAX_FUSED (the last launch of a level is shorter when
 *   it does not divide refine_iters); 0 = the library's choice.  The result does NOT depend on it, bit for bit: a launch
 *   of k steps stages its tile plus a ring of k cells in LDS and runs the one update expression k times on a shrinking
 *   region; cells outside the image are never cells, a neighbour beyond the frame is the clamped cell of the same iterate.
 * workspace: t2v_optical_flow_refined_workspace_floats(H, W, levels) floats (twice the LK workspace; 0 for a refused shape),
 * 8-byte aligned, any content.  Refused, with T2V_ERR_INVALID and nothing launched: everything t2v_optical_flow (_u8)
 * refuses; alpha not finite or <= 0 (or alpha^2 not a positive finite fp32 number); refine_iters outside 0..1024;
 * iters_per_launch outside 0..T2V_FLOW_REFINE_MAX_FUSED.  No allocation, no host synchronisation, no atomics; every gather
 * coordinate is clamped before it becomes an index; two calls give the same bits.  The u8 entry gives the bits of the fp32
 * entry on the images t2v_pose_u8_to_f32 makes of the same bytes, and its flows are finite (alpha^2 > 0).
 * Kernel launches per call, fixed by (levels, iters, refine_iters, iters_per_launch) alone, with k = iters_per_launch
 * (0: the library's choice, 8):
 *   refine_iters == 0:  levels * (iters + 1) + 1
 *   otherwise:          levels * (iters + 2 + ceil(refine_iters / k)) + 1
 *     = levels (grey + pyramid) + levels * iters (LK) + levels (It0 and the per-pixel constants)
 *       + levels * ceil(refine_iters / k) (Jacobi) + 1 (output). */
#define T2V_FLOW_REFINE_MAX_FUSED 8
/* T2V_FLOW_REFINE_ABI_VERSION of the library that was loaded. */
int t2v_flow_refine_abi_version(void);
size_t t2v_optical_flow_refined_workspace_floats(int H, int W, int levels);
int t2v_optical_flow_refined(t2v_ctx* ctx, void* stream, const float* cur, int cur_cs, int cur_c0, const float* prev,
                             int prev_cs, int prev_c0, int H, int W, int levels, int iters, int radius, float lambda,
                             float alpha, int refine_iters, int iters_per_launch, float* workspace, float* flow_out);
int t2v_optical_flow_refined_u8(t2v_ctx* ctx, void* stream, const uint8_t* cur, int cur_cs, const uint8_t* prev, int prev_cs,
                                int H, int W, int levels, int iters, int radius, float lambda, float alpha, int refine_iters,
                                int iters_per_launch, float* workspace, float* flow_out);

#ifdef __cplusplus
}
#endif

#endif /* T2V_FLOW_REFINE_H_ */
