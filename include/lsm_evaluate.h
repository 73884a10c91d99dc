/*
 * lsm_evaluate.h -- C ABI of the sequence form of the actor and critic heads: what GR_Actor.evaluate_actions
 * and GR_Critic.forward (onpolicy/algorithms/graph_actor_critic.py) run after GNNBase.forward on a minibatch
 * of recurrent_generator or feed_forward_generator -- MLPBase, the T x N branch of RNNLayer.forward, and
 * ACTLayer.evaluate_actions' Categorical (the log-probability of the STORED action, the entropy) or v_out --
 * for C chunks of T steps in one launch (two with dist_entropy). Forward only: no backward pass. Discrete
 * action spaces only. The weight blob, lsm_head_config and its limits are lsm_policy.h's.
 *
 * The minibatch is time-major, as the generators yield it: row m = l * C + b is step l of chunk b. Per
 * chunk b, for l = 0 .. T - 1 in order, on row m (all arithmetic float32):
 * 1.-2. the feature norm and MLPLayer of lsm_policy.h, unchanged.
 * 3. RNNLayer, when recurrent_N > 0: h_k = h_k * masks[m] for every layer k (a product, as in the reference:
 *    a non-finite state under a zero mask stays non-finite), then the GRU cells of lsm_policy.h's step 3.
 *    h starts from rnn_states[b] and is carried to step l + 1; rnn_out[b][k] is h_k after the last step.
 *    This per-step product is the T x N branch of RNNLayer.forward: that branch runs the steps between two
 *    zero masks as one nn.GRU call and multiplies by masks[start] at each segment's start; every mask
 *    inside a segment is 1, and h * 1.0f is exact. features = LayerNorm(Hd)(h'_last). With
 *    recurrent_N == 0 every row is independent and rnn_states, masks and rnn_out are not read, written or
 *    checked; a feed_forward_generator minibatch is T = 1, C = its size.
 * 4. LSM_HEAD_ACTOR (ACTLayer.evaluate_actions, the Discrete branch): a NaN in features is read as 0 (the
 *    reference zeroes it in place; the features output holds the zeroed values). Logits, the availability
 *    mask, mx, e_a, s and log p_a as in lsm_policy.h's step 4. Then
 *      log_probs[m] = log p_(actions[m])
 *      entropy[m]   = -(sum over a ascending with e_a > 0 of (e_a / s) * log p_a)
 *    (a masked action has e_a == 0 and adds nothing, as under torch's clamp of the logits), and
 *      dist_entropy = sum_m entropy[m] * active_masks[m] / sum_m active_masks[m]   (0 / 0 stays NaN), or,
 *                     with active_masks == NULL, the mean of entropy over the T * C rows.
 *    dist_entropy is reduced in float64 in a fixed order that does not depend on launch timing: each chunk
 *    adds its rows' entropy * weight and weight (1 without active_masks) for l = 0 .. T - 1 in turn; each
 *    group of 64 consecutive chunks adds its chunks' two sums, b ascending, and writes them to
 *    scratch[2 g], scratch[2 g + 1]; a second launch of one thread adds the groups' sums, g ascending,
 *    divides and rounds once to float32. No atomics, no last-block-done counter.
 *    A row without any available action is uniform: log-probability -log A, entropy log A. (torch's
 *    Categorical rounds -FLT_MAX - logsumexp and reports 0 and -0 there; that is not imitated.) The
 *    log-probability of a stored action that is unavailable in a row with other actions available is about
 *    -FLT_MAX.
 *    Outputs, each nullable: log_probs [T*C], entropy [T*C], dist_entropy [1], logits [T*C][A] (after the
 *    availability mask; for tests), features [T*C][Hd], rnn_out [C][recurrent_N][Hd].
 * 5. LSM_HEAD_CRITIC: values[m] = Linear(Hd, 1)(features) as in lsm_policy.h's step 5. Outputs, each
 *    nullable: values [T*C], features, rnn_out. The actor's fields (actions .. logits, scratch) are ignored.
 *
 * Bad actions: actions[m] that is NaN, not integral, or outside [0, A) is clamped before any use -- NaN to
 * 0, otherwise to [0, A - 1] and then truncated toward zero (2.5 is 2, -1 is 0, A is A - 1) -- and sets
 * *bad = 1. *bad is only ever set: the caller clears it. No address is formed from an unclamped value.
 *
 * lsm_head_evaluate is stream-ordered and asynchronous: no host synchronisation, no allocation, no atomics;
 * a chunk's state never leaves its workgroup between steps; every sum runs in a fixed order, so a call is
 * bit-reproducible. A workgroup owns 64 chunks and keeps, per chunk, the input row, two activation rows and
 * recurrent_N state rows in LDS: 256 * (pad(max(in, Hd)) + 2 pad(max(Hd, A)) + recurrent_N pad(Hd)) bytes
 * with pad(w) = round_up(w, 4) + 4. A config that needs more than the 163840 bytes a workgroup has is
 * refused by both entry points (hidden 64 fits at every input width and recurrent_N; with recurrent_N 1
 * hidden 128 fits up to in = 240; with recurrent_N 2 hidden 124 is the largest that fits (up to in = 124)
 * and hidden 128 does not at any width, though lsm_head_forward takes it). lsm_head_plan (lsm_policy.h) answers for a config.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_policy_last_error() (prefix "evaluate: "). Refused: everything lsm_head_forward refuses for the config
 * and the pointers (a null io or weights; with C > 0 a null x0 / x1 of nonzero width or the recurrent form
 * without rnn_states or masks; misaligned pointers: 4 bytes, bad and scratch 8; the config's limits);
 * T < 1, C < 0, T * C > INT32_MAX; with C > 0 a null actions for the actor; dist_entropy without scratch;
 * rnn_out overlapping rnn_states; the actor with every output null; the LDS need above. C == 0 is legal and
 * does nothing.
 */
#ifndef LSM_EVALUATE_H
#define LSM_EVALUATE_H

#include <stddef.h>
#include <stdint.h>

#include "lsm_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One call's tensors: device pointers for lsm_head_evaluate, host pointers for lsm_host_head_evaluate. */
typedef struct lsm_eval_io {
  const float* x0;                /* [T*C][in0]; row l*C + b is step l of chunk b (the generators' order) */
  const float* x1;                /* [T*C][in1] */
  const float* rnn_states;        /* [C][recurrent_N][hidden]: each chunk's state at its first step */
  const float* masks;             /* [T*C] */
  const float* actions;           /* actor: [T*C] float32, the buffer's action rows */
  const float* available_actions; /* actor: [T*C][A], nullable */
  const float* active_masks;      /* actor: [T*C], nullable: the weights of dist_entropy */
  float* log_probs;               /* actor: [T*C], nullable */
  float* entropy;                 /* actor: [T*C] per row, nullable */
  float* dist_entropy;            /* actor: [1], nullable */
  float* logits;                  /* actor: [T*C][A], nullable (tests) */
  float* values;                  /* critic: [T*C], nullable */
  float* features;                /* [T*C][hidden], nullable */
  float* rnn_out;                 /* [C][recurrent_N][hidden]: the state after the last step, nullable */
  double* scratch;                /* lsm_head_evaluate_scratch_bytes(C, T) bytes; needed iff dist_entropy */
  int64_t* bad;                   /* [1], nullable */
} lsm_eval_io;

/* Bytes of scratch for a call with C chunks of T steps: two doubles per group of 64 chunks (at least 16);
 * 0 for C < 0 or T < 1. */
size_t lsm_head_evaluate_scratch_bytes(int64_t C, int32_t T);

int lsm_head_evaluate(lsm_head_config cfg, const float* weights /* device blob */, const lsm_eval_io* io,
                      int64_t C, int32_t T, void* hip_stream);

/* The same routine on host memory (all pointers host pointers), through the same per-row code. */
int lsm_host_head_evaluate(lsm_head_config cfg, const float* weights, const lsm_eval_io* io, int64_t C, int32_t T);

#ifdef __cplusplus
}
#endif
#endif
