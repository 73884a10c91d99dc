/*
 * lsm_policy.h -- C ABI of the fused actor and critic heads: what GR_Actor.forward and GR_Critic.forward
 * (onpolicy/algorithms/graph_actor_critic.py:162-172, 406-418) run after GNNBase.forward -- the
 * cat([obs, nbd_features]), MLPBase, the GRU RNNLayer, ACTLayer's Categorical (sample or mode, with the
 * log-probability) and the critic's v_out -- for M rows in one launch. Inference only (GMPERunner.collect
 * and evaluation, under torch.no_grad()): no backward pass; Discrete action spaces only. The sequence form
 * (evaluate_actions on a minibatch: the stored action's log-probability, the entropy) is lsm_evaluate.h.
 *
 * What is computed per row m (all arithmetic float32; Hd = hidden, in = in0 + in1). The row's input is
 * x = [x0[m][0 .. in0), x1[m][0 .. in1)]; the concatenation is never materialised in memory. in0 == 0 with a
 * null x0 is legal (the critic without use_cent_obs), and so is in1 == 0 with a null x1.
 *   actor:  x0 = obs, x1 = the encoder's output;  critic: x0 = cent_obs (or nothing), x1 = the encoder's.
 * 1. feature_norm: x = LayerNorm(in)(x). Every LayerNorm here: eps 1e-5, biased variance.
 * 2. MLPLayer: y = LayerNorm(Hd)(act(fc1 x)), then layer_N times y = LayerNorm(Hd)(act(fc2[i] y)), act
 *    ReLU or Tanh. These LayerNorms do not depend on feature_norm. The fc2[i] are separate weights; the
 *    state dict's base.mlp.fc_h.*, the template they were cloned from, is not used by forward and not packed.
 * 3. RNNLayer, when recurrent_N > 0 (the one-step branch; the T x N sequence branch is lsm_evaluate.h):
 *    h_l = rnn_states[m][l] * masks[m] (a product, as in the reference: a non-finite state under a zero mask
 *    stays non-finite). For l = 0 .. recurrent_N - 1, x_0 = y, x_l = h'_(l-1), torch's GRU cell, gates r, z, n:
 *      r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
 *      n = tanh(W_in x + b_in + r * (W_hn h + b_hn))   h' = (1 - z) * n + z * h
 *    rnn_out[m][l] = h'_l; features = LayerNorm(Hd)(h'_last). Without an RNN, features = y and no state is
 *    read or written.
 * 4. LSM_HEAD_ACTOR: l = Linear(Hd, A)(features); where available_actions[m][a] == 0, l_a = -FLT_MAX
 *    (torch.finfo(float32).min; available_actions == NULL: every action is available).
 *    mx = max l; e_a = exp(l_a - mx); s = sum of e_a, a ascending; log p_a = (l_a - mx) - log s.
 *    Mode (u == NULL): the first a attaining mx. Sample (u [M] float32 in [0, 1)): the first a whose
 *    running sum e_0 + .. + e_a exceeds u[m] * s; if rounding leaves none, the last a with e_a > 0.
 *    This is Categorical.sample as a distribution (the inverse CDF of the caller's uniforms), not torch's
 *    generator stream: the same seed does not give torch.multinomial's actions.
 *    Outputs, each nullable: actions_i32 [M] (what lsm_step takes as [n][N]), actions_f32 [M] (the replay
 *    buffer's row), log_probs [M] (of the chosen action), features [M][Hd] (GR_Actor.forward returns them),
 *    rnn_out [M][recurrent_N][Hd], logits [M][A] (after the availability mask; for tests).
 * 5. LSM_HEAD_CRITIC: values[m] = Linear(Hd, 1)(features), v_out. PopArt.forward is the same F.linear; its
 *    stddev, mean, mean_sq and debiasing_term are not packed. Outputs, each nullable: values [M], features,
 *    rnn_out. The actor's fields of lsm_head_io are ignored (not read, written or checked), as the
 *    critic's are for the actor; so are x0 / x1 of a zero width and the three state fields when
 *    recurrent_N == 0.
 *
 * The packed weight blob (float32, lsm_head_weights_floats(cfg) values, torch's [out][in] rows), in order:
 *   feature-norm gamma [in], beta [in]              (present, unread, when feature_norm == 0: 1 and 0)
 *   fc1 weight [Hd][in], bias [Hd], its LayerNorm gamma [Hd], beta [Hd]
 *   fc2[i], i = 0 .. layer_N - 1: weight [Hd][Hd], bias, LayerNorm gamma, beta
 *   GRU layer k = 0 .. recurrent_N - 1: weight_ih [3 Hd][Hd], weight_hh [3 Hd][Hd], bias_ih [3 Hd], bias_hh [3 Hd]
 *   the RNN's norm gamma [Hd], beta [Hd]             (only when recurrent_N > 0)
 *   the output Linear: weight [A][Hd] (actor) or [1][Hd] (critic), bias
 *
 * Bad inputs: a u[m] that is not finite or outside [0, 1) is clamped into [0, 1) (NaN and negatives
 * become 0, the rest the largest float below 1) and sets *bad = 1. *bad is only ever set: the caller clears
 * it. No address is formed from data: the chosen action is a loop index below num_actions.
 *
 * lsm_head_forward is stream-ordered and asynchronous: one kernel launch, no host synchronisation, no
 * allocation, no atomics; every row's sums run in one lane in a fixed order (four partial sums over the
 * inputs i mod 4, each ascending, added pairwise), so the output is bit-reproducible from call to call. Return value: 0 on success; nonzero on an argument error, before
 * any launch or write, with the text in lsm_policy_last_error() (thread-local, prefix "head: ").
 * Refused: a null io or weights; with M > 0 a null x0 with in0 > 0, a null x1 with in1 > 0, or the
 * recurrent form without rnn_states or masks; misaligned pointers (4 bytes; bad: 8); M < 0 or
 * M > INT32_MAX; in0 or in1 < 0; in0 + in1 outside [1, 256]; hidden outside [1, 128]; layer_N outside
 * [0, 4]; recurrent_N outside [0, 2]; an unknown kind; num_actions outside [1, 64] for the actor; rnn_out
 * overlapping rnn_states; the actor with neither actions_i32 nor actions_f32. M == 0 is legal and does
 * nothing.
 *
 * The declarations live apart from lsm_rollout.h (part of the rollout's build id) and the other
 * learner-side headers.
 */
#ifndef LSM_POLICY_H
#define LSM_POLICY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LSM_HEAD_ACTOR = 0, LSM_HEAD_CRITIC = 1 };

/* The head's shape, passed by value (the reference's argument names in brackets). */
typedef struct lsm_head_config {
  int32_t in0;          /* width of the first input block (obs / cent_obs); 0 = none */
  int32_t in1;          /* width of the second input block (the encoder's output) */
  int32_t hidden;       /* [hidden_size] */
  int32_t layer_N;      /* [layer_N] */
  int32_t relu;         /* [use_ReLU]: 1 ReLU, 0 Tanh */
  int32_t feature_norm; /* [use_feature_normalization] */
  int32_t recurrent_N;  /* [recurrent_N]; 0 = neither use_recurrent_policy nor use_naive_recurrent_policy */
  int32_t kind;         /* LSM_HEAD_ACTOR / LSM_HEAD_CRITIC */
  int32_t num_actions;  /* actor only: Discrete(num_actions) */
} lsm_head_config;

/* One call's tensors: device pointers for lsm_head_forward, host pointers for lsm_host_head_forward. */
typedef struct lsm_head_io {
  const float* x0;                /* [M][in0], NULL when in0 == 0 */
  const float* x1;                /* [M][in1], NULL when in1 == 0 */
  const float* rnn_states;        /* [M][recurrent_N][hidden]; unread when recurrent_N == 0 */
  const float* masks;             /* [M]; unread when recurrent_N == 0 */
  const float* u;                 /* actor: [M] uniforms in [0, 1), NULL = the mode */
  const float* available_actions; /* actor: [M][num_actions], nullable */
  int32_t* actions_i32;           /* actor: [M], nullable */
  float* actions_f32;             /* actor: [M], nullable */
  float* log_probs;               /* actor: [M], nullable */
  float* logits;                  /* actor: [M][num_actions], nullable */
  float* values;                  /* critic: [M], nullable */
  float* features;                /* [M][hidden], nullable */
  float* rnn_out;                 /* [M][recurrent_N][hidden], nullable */
  int64_t* bad;                   /* [1], nullable */
} lsm_head_io;

/* Length of the packed weight blob in floats; 0 for a config outside the limits. */
size_t lsm_head_weights_floats(lsm_head_config cfg);

int lsm_head_forward(lsm_head_config cfg, const float* weights /* device blob */, const lsm_head_io* io,
                     int64_t M, void* hip_stream);

/* The same routine on host memory (all pointers host pointers), through the same per-row code. */
int lsm_host_head_forward(lsm_head_config cfg, const float* weights, const lsm_head_io* io, int64_t M);

const char* lsm_policy_last_error(void);

/* The launch plan of the three head routines for a config and sizes (what lsm_kernel_name is for the step
 * kernels): filled on the host by the launches' own code; nothing is launched and no pointer is needed.
 * Strides are in floats per tile row (a tile is 64 rows or chunks), offsets in floats from the start of
 * lsm_head_backward's workspace (include/lsm_backward.h); a field the routine does not have is 0. */
enum { LSM_HEAD_PLAN_FORWARD = 0, LSM_HEAD_PLAN_EVALUATE = 1, LSM_HEAD_PLAN_BACKWARD = 2 };
#define LSM_HEAD_PLAN_MAX_JOBS 17

typedef struct lsm_head_plan_job {
  int32_t nout, nin; /* the job's matrix [nout][nin] and its bias column (column nin) */
  int32_t ti_n;      /* its 64-wide tiles along i (columns 0 .. nin); ceil(nout / 64) tiles along j */
  int32_t tile0;     /* its first tile */
} lsm_head_plan_job;

typedef struct lsm_head_launch_plan {
  int32_t SX, SA, SH;     /* the input row, an activation row, a GRU state row (forward: SH = 0, h lives in
                             the input row; backward: stage 1's) */
  int32_t S0, S1, S2, HP; /* backward, stage 2: rows B0, B1, B2 and the gate sections' width in B0 */
  int32_t njobs, ntiles;  /* backward, stage 3 */
  int64_t lds_bytes[2];   /* forward and evaluate: [0], the one launch; backward: stage 1, stage 2 */
  int64_t slabs;          /* backward: ceil(T * C / LSM_BWD_SLAB) */
  int64_t ws_floats;      /* backward: the workspace's documented size in floats */
  int64_t o_feat;         /* backward: the saved features [T*C][hidden] */
  int64_t o_ho[2];        /* backward: GRU layer k's saved h' [T*C][hidden] */
  lsm_head_plan_job job[LSM_HEAD_PLAN_MAX_JOBS];
} lsm_head_launch_plan;

/* Returns 0, or nonzero with the routine's own refusal of the config and sizes in lsm_policy_last_error()
 * (the pointer checks are not made; the forward takes C * T rows); *out is written on success only. */
int lsm_head_plan(lsm_head_config cfg, int32_t which, int64_t C, int32_t T, lsm_head_launch_plan* out);

#ifdef __cplusplus
}
#endif
#endif
