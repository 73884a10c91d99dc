/*
 * lsm_backward.h -- C ABI of the backward pass through the actor and critic heads: from the gradient at a
 * head's output (lsm_loss.h's dlogits / dvalues) to the gradient of every packed head weight and the gradient
 * at the head's two input blocks (dx1 is the seed of the encoder's backward), on a time-major minibatch of C
 * chunks of T steps, as lsm_evaluate.h takes it. What the reference reaches with loss.backward() through
 * ACTLayer / v_out, RNNLayer (BPTT through the GRU) and MLPBase. The weight blob, lsm_head_config and its
 * limits are lsm_policy.h's. Discrete action spaces only. The encoder's backward is not here; the gradient norm,
 * the clipping and the optimiser are lsm_optim.h's, on dweights as this call leaves it.
 *
 * The call is self-contained: it recomputes the forward of lsm_evaluate.h's steps 1-3 (and the NaN rule of
 * step 4) from the same inputs with the same per-row arithmetic (csrc/lsm_head_tile.h), so the gradient is
 * that of the function lsm_head_evaluate computes. All arithmetic float32 unless stated. Per row m = l * C + b:
 *
 * - Output layer. delta_out = dlogits[m] (actor; an entry with available_actions[m][a] == 0 is read as 0
 *   whatever it holds: the reference's masking assignment cuts the graph there) or dvalues[m] (critic).
 *   dfeatures = W_out^T delta_out. A feature that the actor's NaN rule zeroed gets gradient 0.
 * - Every LayerNorm (the RNN's, each MLP layer's, the feature norm): with xhat = (p - mean) * rs of the
 *   forward (biased variance, eps 1e-5), g = dy * gamma: dp = rs * (g - mean(g) - xhat * mean(g * xhat));
 *   dgamma = sum_m dy * xhat, dbeta = sum_m dy.
 * - GRU, torch's cell, for l = T - 1 .. 0 per chunk, layers k = recurrent_N - 1 .. 0. With dh the gradient at
 *   h'_k (from the layer above, or the RNN norm, plus the state's gradient carried from step l + 1), h the
 *   masked previous state and hg = W_hn h + b_hn:
 *     dz = dh (h - n), dn = dh (1 - z), dn_pre = dn (1 - n^2), dr_pre = dn_pre hg r (1 - r),
 *     dz_pre = dz z (1 - z); delta_ih = [dr_pre, dz_pre, dn_pre], delta_hh = [dr_pre, dz_pre, dn_pre r];
 *     dx = W_ih^T delta_ih; dh_masked = dh z + W_hh^T delta_hh.
 *   h_k = h_k * masks[m] gives dh_prev = dh_masked * masks[m]: a zero mask cuts the chunk's history. With
 *   recurrent_N == 2 layer 1's dx is added to layer 0's dh of the same step. No seed enters at the final
 *   state (rnn_out is not differentiated) and the gradient at rnn_states is not an output (the buffer's rows
 *   are data). The state's gradient is carried in the workgroup, never through global memory between steps.
 * - ReLU passes the gradient where the activation is > 0 (0 at 0, as torch); Tanh multiplies by 1 - y^2.
 * - dx0 / dx1: the two column blocks of the gradient at the virtual cat([x0, x1]).
 * - Weights. For every matrix dW[j][i] = sum_m delta[m][j] * in[m][i], and the vectors (biases, gammas,
 *   betas) are column sums of the same kind. Rows are split into slabs of LSM_BWD_SLAB consecutive rows;
 *   within a slab every entry is accumulated in float32 with rows ascending, in three levels (an FMA chain
 *   over 16 rows, 16 such runs added in turn, those sums added in turn), so that the rounding grows with 16 +
 *   16 + 8 additions and not with 2048; a bias's column sum, whose terms may cancel to far below their size,
 *   also carries the rounding of each addition (two-sum) and adds it back at the end. The slabs' partials
 *   are added in ascending order in float64 and rounded once.
 * - Non-finite inputs give non-finite gradients, as in the reference. No address is ever formed from data.
 *
 * dweights [lsm_head_weights_floats(cfg)] is overwritten (not accumulated) with the gradient of every entry
 * of the blob in the blob's own order (lsm_policy.h); the feature-norm slots are written as 0 when
 * feature_norm == 0.
 *
 * lsm_head_backward is stream-ordered and asynchronous: no host synchronisation, no allocation, no atomics,
 * no last-block-done counter; every sum runs in a fixed order, so a call is bit-reproducible. Three stages,
 * each its own launch (the third: two):
 *   1. the forward with saves: lsm_evaluate.h's work split (a 256-thread workgroup owns 64 chunks, lane =
 *      chunk, four waves split the columns, l = 0 .. T - 1), writing what the other stages need to workspace.
 *      LDS per chunk: pad(max(in, Hd)) + 2 pad(Hd) + recurrent_N pad(Hd) floats, pad(w) = round_up(w, 4) + 4.
 *   2. the backward sweep, same ownership, l = T - 1 .. 0: writes dx0 / dx1 and every Linear's pre-activation
 *      gradient to workspace. LDS per chunk: pad(max(in, G)) + pad(max(in, Hd, A)) + pad(Hd) +
 *      recurrent_N pad(Hd) floats, G = 4 round_up(Hd, 4) with an RNN, else Hd.
 *   3. the weight gradients: one workgroup per (slab, 64 x 64 tile of a matrix and its bias column), then the
 *      float64 sum over the slabs.
 * A config whose 64-chunk tile needs more than the 163840 bytes of LDS a workgroup has in stage 1 or 2 is
 * refused by both entry points (hidden 64 fits up to in = 240 with recurrent_N 1 and up to in = 172 with
 * recurrent_N 2; hidden 128 with an RNN does not fit).
 *
 * Workspace, in float32 arrays of [T*C][n] each (n in brackets), all offsets int64:
 *   stage 1: the input of fc1 [in]; per MLP layer the activation [Hd] and its LayerNorm [Hd]; per GRU layer
 *   the masked state, r, z, n, hg and h' [6 Hd]; the features [Hd];
 *   stage 2: delta_out [A]; the RNN norm's (dy * xhat, dy) [2 Hd]; per GRU layer delta_ih and delta_hh [6 Hd];
 *   per MLP layer (dy * xhat, dy) and delta [3 Hd]; the feature norm's (dy * xhat, dy) [2 in];
 *   stage 3: ceil(T*C / LSM_BWD_SLAB) partials of lsm_head_weights_floats(cfg) floats.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_policy_last_error() (prefix "backward: "). Refused: the config's limits; a null io, weights, dweights
 * or workspace; with C > 0 a null x0 / x1 of nonzero width, the recurrent form without rnn_states or masks,
 * the actor without dlogits, the critic without dvalues; misaligned pointers (4 bytes; workspace: 8); T < 1,
 * C < 0, T * C > INT32_MAX; an output (dweights, dx0, dx1, workspace) overlapping an input or another
 * output; the LDS need above. C == 0 is legal and does nothing.
 */
#ifndef LSM_BACKWARD_H
#define LSM_BACKWARD_H

#include <stddef.h>
#include <stdint.h>

#include "lsm_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per slab of the weight-gradient reduction. */
#define LSM_BWD_SLAB 2048

/* One call's tensors: device pointers for lsm_head_backward, host pointers for lsm_host_head_backward. */
typedef struct lsm_bwd_io {
  const float* x0;                /* as lsm_eval_io: [T*C][in0], row l*C + b = step l of chunk b */
  const float* x1;                /* [T*C][in1] */
  const float* rnn_states;        /* [C][recurrent_N][hidden] */
  const float* masks;             /* [T*C] */
  const float* available_actions; /* actor: [T*C][A], nullable */
  const float* dlogits;           /* actor: [T*C][A], lsm_ppo_loss's */
  const float* dvalues;           /* critic: [T*C] */
  float* dweights;                /* [lsm_head_weights_floats(cfg)], the blob's own layout */
  float* dx0;                     /* [T*C][in0], nullable */
  float* dx1;                     /* [T*C][in1], nullable */
  void* workspace;                /* lsm_head_backward_workspace_bytes(cfg, C, T) bytes */
} lsm_bwd_io;

/* Bytes of workspace for a call with C chunks of T steps (at least 8); 0 for a config outside the limits,
 * C < 0, T < 1 or T * C > INT32_MAX. */
size_t lsm_head_backward_workspace_bytes(lsm_head_config cfg, int64_t C, int32_t T);

int lsm_head_backward(lsm_head_config cfg, const float* weights /* device blob */, const lsm_bwd_io* io, int64_t C,
                      int32_t T, void* hip_stream);

/* The same routine on host memory (all pointers host pointers), through the same per-row code with a tile
 * of one chunk and the same slab grouping. */
int lsm_host_head_backward(lsm_head_config cfg, const float* weights, const lsm_bwd_io* io, int64_t C, int32_t T);

#ifdef __cplusplus
}
#endif
#endif
