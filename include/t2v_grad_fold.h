/* t2v_grad_fold.h -- C ABI of libt2v_gradfold.so: the fold of a flat gradient bucket into the accumulator of a train step that
 * walks several clips per rank before one optimiser step (--batchSize above the number of ranks).  The library stands beside
 * libt2v_hip.so, which it links: the context is that library's t2v_ctx, a refusal returns T2V_ERR_INVALID (-1) and leaves
 * its message where t2v_last_error() of t2v.h reads it, a HIP error returns T2V_ERR_HIP (-2); 0 is success. */
#ifndef T2V_GRAD_FOLD_H_
#define T2V_GRAD_FOLD_H_

#ifdef __cplusplus
extern "C" {
#endif

#define T2V_GRAD_FOLD_ABI_VERSION 1

typedef struct t2v_ctx t2v_ctx;      /* t2v_create of t2v.h */

/* mode of t2v_grad_fold, element by element over n floats:
 *   OPEN:  acc  = grad                  (the first clip of an optimiser step; grad is only read)
 *   ADD:   acc  = acc + grad            (a clip between the first and the last; grad is only read)
 *   CLOSE: grad = (acc + grad) * scale  (the last clip; acc is only read)
 * One fp32 addition, then one fp32 multiplication, never contracted: K clips folded OPEN, ADD, ..., CLOSE with
 * scale = (float)(1.0 / K) leave ((g_0 + g_1) + ... + g_{K-1}) * scale in grad, bit for bit what that expression gives in
 * IEEE fp32 arithmetic on the host. */
#define T2V_GRAD_FOLD_OPEN 0
#define T2V_GRAD_FOLD_ADD 1
#define T2V_GRAD_FOLD_CLOSE 2

/* T2V_GRAD_FOLD_ABI_VERSION of the library that was loaded. */
int t2v_grad_fold_abi_version(void);
/* One launch on `stream`, a grid sized from the device's compute units whatever n is.  grad and acc: n floats each on the
 * device, 4-byte aligned; where both have the same alignment modulo 16 the body moves 16 bytes per lane.  Refused, with
 * T2V_ERR_INVALID, before anything is launched or read: a null ctx, grad or acc; n <= 0; a mode that is none of the three; a
 * scale that is not finite and > 0 (it is read in CLOSE only, and checked in every mode); pointers that are not 4-byte
 * aligned; ranges [grad, grad + n) and [acc, acc + n) that overlap.  No allocation, no host synchronisation, no atomics. */
int t2v_grad_fold(t2v_ctx* ctx, void* stream, float* grad, float* acc, long n, int mode, float scale);

#ifdef __cplusplus
}
#endif

#endif /* T2V_GRAD_FOLD_H_ */
