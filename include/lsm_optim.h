/*
 * lsm_optim.h -- C ABI of the end of GR_MAPPO.ppo_update: the gradient norm, clip_grad_norm_'s coefficient and
 * torch.optim.Adam's step (single tensor, no amsgrad, L2 weight decay), on the packed weight blobs the other units
 * read (lsm_gnn.h, lsm_policy.h) and on the gradients their backward passes leave in the blobs' own layout
 * (lsm_backward.h, lsm_gnn_backward.h, lsm_gnn_embed_backward.h). The weights are updated in place: the next
 * forward call reads them where they are, with no trip through the host.
 *
 * One call steps up to LSM_OPT_MAX_GROUPS parameter groups. A group is what the reference gives one
 * torch.optim.Adam and one clip_grad_norm_ call (the actor: its encoder's blob and its head's blob; the critic
 * likewise): its own norm, coefficient, skip decision, step count and learning rate. A group is up to
 * LSM_OPT_MAX_SEGMENTS segments, each n consecutive floats of (weights, grads, exp_avg, exp_avg_sq). A segment may
 * start at any float offset of a blob: its pointers are 4-byte aligned only.
 *
 * THE ARITHMETIC (the contract). float32 unless stated; no fused multiply-add anywhere; division and square root
 * correctly rounded on both sides (the device code uses the plain operators, which the compiler expands to the
 * correctly rounded sequences; its __fsqrt_rn maps to the approximate instruction and is not used). b1f, b2f,
 * epsf, wdf, maxf are (float) of the group's beta1 .. max_grad_norm, omb1 = (float)(1.0 - beta1) and
 * omb2 = (float)(1.0 - beta2), formed in float64 and rounded once.
 *
 * Norm. S = the sum of (double)g * (double)g over the group's segments in this fixed order, which depends on
 * neither the grid nor the device and which the host entry point runs too:
 *   segments in table order; each segment cut into chunks of LSM_OPT_CHUNK consecutive floats (the last one
 *   shorter); within a chunk of len floats, lane j of LSM_OPT_LANES (256) adds its elements j, j + 256, j + 512, ...
 *   < len ascending into a float64 that starts at 0, each term the rounded float64 product; the 256 lane sums are
 *   then folded pairwise, q[j] += q[j + s] for s = 128, 64, .. 1 (all j < s), and q[0] is the chunk's partial;
 *   the group's partials are added ascending in float64 from 0.
 * grad_norm = (float)sqrt(S), the float64 square root rounded to float32 once. This is deliberately not torch's
 * norm of float32 per-tensor norms: a gradient whose float32 square sum overflows (an entry of 1e20) still gets a
 * finite norm here, and the result does not depend on how the parameters are cut into tensors.
 *
 * Coefficient. With use_max_grad_norm: c = maxf / (grad_norm + 1e-6f); clip_coef = c > 1.0f ? 1.0f : c (torch's
 * clamp: a NaN stays NaN). Without it clip_coef = 1 and grad_norm is still reported (the reference's
 * get_grad_norm). grads is const: the clipped gradient clip_coef * grad is used, not written back, unlike
 * clip_grad_norm_.
 *
 * Skip. With skip_nonfinite and a grad_norm that is not finite the group's weights, moments and state are left
 * bit for bit as they were and info's skipped = 1: what GradScaler.step does for the reference in float32 (its
 * scaling by powers of two is otherwise exact and is not reproduced). Without skip_nonfinite the NaN or inf
 * propagates exactly as the formulas say and the call finishes clean (where a NaN stands is part of the contract,
 * its sign bit and payload are not: they depend on how each side propagates a NaN operand and on the default
 * NaN it generates, and the host and the device were seen to differ in the sign).
 *
 * State, double[4] per group: {steps, p1 = beta1^steps, p2 = beta2^steps, reserved}; a fresh state is {0, 1, 1, 0}.
 * On an executed step, in float64: steps += 1, p1 *= beta1, p2 *= beta2 (running products instead of pow, so
 * that host and device agree to the bit), then
 *   step_size = (float)(lr / (1.0 - p1)),  s2 = (float)sqrt(1.0 - p2).
 *
 * Per element, on an executed step (g, m, v, w: the gradient, exp_avg, exp_avg_sq, the weight):
 *   g = clip_coef * grad;   if wdf != 0:  g = g + wdf * w
 *   m = m + omb1 * (g - m)
 *   v = v * b2f + (omb2 * g) * g
 *   w = w - step_size * (m / (sqrt(v) / s2 + epsf))
 *
 * info, float[4] per group, overwritten by every call: {grad_norm, clip_coef, skipped (0 or 1), reserved = 0}.
 *
 * LAUNCHES. All groups of a call go through the same three launches, whatever n_groups is:
 *   1. one workgroup per chunk: the chunk's float64 partial into the workspace;
 *   2. one workgroup per group: the partials ascending, then one thread writes grad_norm, clip_coef and the skip
 *      decision to info, advances state, and leaves clip_coef, step_size, s2 and the skip flag in the workspace;
 *   3. one workgroup per chunk: the elements. Where a segment's four pointers sit at the same offset from a 16-byte
 *      boundary the chunk's body goes through 16-byte vector accesses and the up to three floats before the
 *      boundary and after the last whole vector through scalar ones; otherwise every access is scalar.
 * A call with no chunk at all launches only the second. No atomics, no last-block-done counter, no host
 * synchronisation, no allocation; the segment table travels in the kernel arguments. The call is stream-ordered
 * and asynchronous, and bit-reproducible.
 *
 * Workspace: 8 * (4 * LSM_OPT_MAX_GROUPS + the number of chunks of all groups) bytes, 8-byte aligned; a chunk
 * count is ceil(n / LSM_OPT_CHUNK) per segment.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_optim_last_error() (thread-local, prefix "optim: "). Refused: a null table with n_groups > 0; n_groups
 * outside [0, LSM_OPT_MAX_GROUPS]; n_segments outside [0, LSM_OPT_MAX_SEGMENTS]; n < 0; a null pointer in a
 * segment with n > 0; a null state, info or (n_groups > 0) workspace; misaligned pointers (4 bytes; state and
 * workspace: 8); any overlap between two written ranges (weights, exp_avg, exp_avg_sq, state, info, workspace; of
 * one group or of two) or between a written range and a grads range; lr, eps, weight_decay or max_grad_norm
 * negative or not finite; a beta outside [0, 1). n_groups == 0, a group without segments and a segment with
 * n == 0 (whose pointers are not looked at) are legal.
 */
#ifndef LSM_OPTIM_H
#define LSM_OPTIM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_OPT_MAX_GROUPS 4
#define LSM_OPT_MAX_SEGMENTS 8
#define LSM_OPT_CHUNK 1024
#define LSM_OPT_LANES 256

typedef struct lsm_optim_segment {
  float* weights;      /* [n], updated in place */
  const float* grads;  /* [n], read only */
  float* exp_avg;      /* [n], updated in place */
  float* exp_avg_sq;   /* [n], updated in place */
  int64_t n;
} lsm_optim_segment;

typedef struct lsm_optim_group {
  lsm_optim_segment segments[LSM_OPT_MAX_SEGMENTS];
  int32_t n_segments;
  int32_t use_max_grad_norm; /* 0: clip_coef = 1, the norm is still reported */
  int32_t skip_nonfinite;    /* 1: a grad_norm that is not finite leaves the group untouched */
  int32_t reserved;          /* 0 */
  double lr;
  double beta1;
  double beta2;
  double eps;
  double weight_decay;
  double max_grad_norm;
  double* state; /* [4]: steps, beta1^steps, beta2^steps, reserved; read and written */
  float* info;   /* [4]: grad_norm, clip_coef, skipped, reserved; overwritten */
} lsm_optim_group;

/* Bytes of workspace for these groups; 0 for a table whose counts (n_groups, n_segments, n) the call refuses. */
size_t lsm_optim_workspace_bytes(const lsm_optim_group* groups, int32_t n_groups);

/* All pointers device pointers (the table itself is host memory, read during the call only). */
int lsm_optim_step(const lsm_optim_group* groups, int32_t n_groups, void* workspace, void* hip_stream);

/* The same routine on host memory (all pointers host pointers): the same text, the same order. */
int lsm_host_optim_step(const lsm_optim_group* groups, int32_t n_groups, void* workspace);

const char* lsm_optim_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
