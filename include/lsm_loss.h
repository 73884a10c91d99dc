/*
 * lsm_loss.h -- C ABI of the PPO loss and its gradient at the heads' outputs: the lines of
 * GR_MAPPO.ppo_update and GR_MAPPO.cal_value_loss (onpolicy/algorithms/graph_mappo.py) that turn what
 * evaluate_actions returns into policy_loss, value_loss and a gradient -- the clipped surrogate, the clipped
 * Huber (or MSE) value loss, ValueNorm's update and normalisation of the returns
 * (onpolicy/utils/valuenorm.py, norm_axes 1, one element, per_element_update off) and the active-mask
 * weighting. It ends where the networks begin: dlogits and dvalues are the seeds of
 * torch.autograd.backward([logits, values], [dlogits, dvalues]) or of a heads' backward kernel. No backward
 * pass through the heads, no gradient clipping, no optimiser. Discrete action spaces only. PopArt is not
 * offered. The reference runs these lines under autocast with a GradScaler; here everything is float32 and
 * neither is imitated.
 *
 * M rows, in any order. Per-row arithmetic is float32 without contraction (no FMA); every sum over rows is
 * float64 in a fixed order: rows ascending within a group of LSM_LOSS_GROUP = 256 consecutive rows, then the
 * groups ascending. The sums are Sw_p = sum w_p, Sw_v = sum w_v, Sr = sum returns, Sr2 = sum returns^2
 * (each square taken in float64, so it is exact), and the four weighted sums of the statistics below. A sum
 * used in float32 is rounded to float32 once. No atomics and no last-block-done counter: the groups' sums
 * travel through `scratch` between launches.
 *
 * Weights: w_p = active_masks[m] with use_policy_active_masks, else 1; w_v = active_masks[m] with
 * use_value_active_masks, else 1. kp = w_p / (float)Sw_p, kv = w_v / (float)Sw_v (0 / 0 is NaN, as in torch:
 * with no active row the losses and the gradients are NaN).
 *
 * Actor half (logits != NULL), per row m, in one lane:
 *   the availability mask (-FLT_MAX where available_actions == 0; logits that lsm_head_evaluate wrote hold it
 *   already, and applying it twice changes nothing), mx, e_a = expf(l_a - mx), s = sum of e_a (a ascending)
 *   and ls = logf(s) exactly as csrc/lsm_head_tile.h's masked_softmax and lsm_head_evaluate do, so
 *     logp   = (l_act - mx) - ls             bit-equal to lsm_head_evaluate's log_probs for that row
 *     H      = -(sum over a ascending with e_a > 0 of (e_a / s) * ((l_a - mx) - ls))
 *   act = actions[m] clamped as in lsm_evaluate.h (NaN to 0, else to [0, A - 1], truncated; *bad = 1).
 *     ratio  = expf(logp - old_log_probs[m])                                      -> imp_weights[m]
 *     surr1  = ratio * adv;  surr2 = clamp(ratio, lo, hi) * adv,  lo = (float)(1.0 - c), hi = (float)(1.0 + c)
 *     mn     = min(surr1, surr2)                                  (a NaN in either is a NaN, as torch.min)
 *   policy_loss = -(sum w_p mn) / Sw_p, dist_entropy = (sum w_p H) / Sw_p, stats[3] = (sum ratio) / M.
 *   The gradient is that of policy_loss - entropy_coef * dist_entropy, with torch's conventions: min passes
 *   the gradient to the smaller argument and half to each on a tie; clamp passes it on lo <= ratio <= hi:
 *     g      = adv * (t1 + t2 * in),  (t1, t2) = (1, 0) if surr1 < surr2, (0, 1) if surr2 < surr1, else
 *              (0.5, 0.5);  in = 1 on lo <= ratio <= hi, else 0
 *     dlogp  = -(kp * (g * ratio));   dent = -(entropy_coef * kp)
 *     dlogits[m][a] = dlogp * (1[a == act] - p_a) + dent * (-(p_a * (logp_a + H)))     p_a = e_a / s, e_a > 0
 *                   = dlogp * 1[a == act]                                                e_a == 0
 *                   = 0 exactly where available_actions[m][a] == 0 (the reference's masking assignment cuts
 *                     the graph there).
 *
 * Critic half (values != NULL), per row m:
 *     d   = values - value_preds;  vpc = value_preds + clamp(d, -c, c)
 *     tg  = returns, or (returns - mean) / std with use_valuenorm (below)
 *     e_o = tg - values;  e_c = tg - vpc
 *     loss(e) = a * (e * e) / 2 + b * huber_delta * (|e| - huber_delta / 2),  a = 1[|e| <= delta],
 *               b = 1[e > delta]   (the reference's huber_loss, quirk included: b is not 1[|e| > delta], so
 *               for e < -delta both the loss and its gradient are 0), or (e * e) / 2 without use_huber_loss;
 *               loss'(e) = a * e + b * huber_delta, or e
 *     l   = max(loss(e_o), loss(e_c)) with use_clipped_value_loss, else loss(e_o)
 *   value_loss = (sum w_v l) / Sw_v. dvalues is the gradient of value_loss * value_loss_coef, k = kv *
 *   value_loss_coef: max passes the gradient to the larger loss and half to each on a tie, the clipped branch
 *   only on |d| <= c:
 *     dvalues[m] = -(k * loss'(e_o))                          without use_clipped_value_loss
 *     dvalues[m] = -(k_o * loss'(e_o) + k_c * loss'(e_c)),    k_o = k * t_o if t_o > 0, else 0;
 *                  k_c = k * t_c if t_c > 0 and |d| <= c, else 0;  (t_o, t_c) = (1, 0) if l_o > l_c, (0, 1) if
 *                  l_c > l_o, else (0.5, 0.5). A branch that gets no gradient is selected away, not multiplied
 *                  by 0, as torch's masked_fill / where do: with a NaN k (no active row) such a row's
 *                  dvalues is exactly 0, as in torch.
 *
 * ValueNorm (use_valuenorm, with the critic half): update, then normalize, on all M returns.
 *     bm = (float)(Sr / M);  bs = (float)(Sr2 / M);  wb = (float)vn_beta;  om = (float)(1.0 - vn_beta)
 *     rm = rm * wb + bm * om;  rms = rms * wb + bs * om;  db = db * wb + om          (float32, two roundings
 *                                                                                     per product-and-add)
 *     dm = rm / max(db, 1e-5f);  dms = rms / max(db, 1e-5f);  var = max(dms - dm * dm, 1e-2f)
 *     mean = dm;  std = sqrtf(var)
 *   vn_state = {rm, rms, db} is read and updated in place, every row uses the updated state, and denorm (when
 *   given) gets {std, mean}: the pair lsm_buffer_compute_returns and lsm_buffer_advantages take. Without the
 *   critic half, or without use_valuenorm, vn_state and denorm are neither read nor written.
 *
 * A null `logits` skips the actor half (update_actor=False; dlogits, imp_weights, stats[0], stats[2] and
 * stats[3] are neither written nor checked), a null `values` the critic half (dvalues, stats[1], vn_state,
 * denorm). Both null is refused.
 *
 * lsm_ppo_loss is stream-ordered and asynchronous: no host synchronisation, no allocation. Four launches:
 * the sums that do not depend on the network (Sw_p, Sw_v, Sr, Sr2) per group; one workgroup that adds the
 * groups in order and updates the normaliser; the rows (a workgroup per group of 256 rows, whose logits and
 * dlogits go through LDS so that global memory is read and written in row-major order, lane = row); one
 * workgroup that adds the groups' statistics in order and divides. Two identical calls (same vn_state) give
 * the same bits.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_loss_last_error() (thread-local, prefix "loss: "). Refused: a null io, stats or scratch; both halves
 * null; an enabled half without one of its inputs (actor: actions, old_log_probs, advantages; critic:
 * value_preds, returns) or its gradient output (dlogits; dvalues); active_masks null while a flag of an
 * enabled half needs it; use_valuenorm with the critic half and no vn_state; misaligned pointers (4 bytes;
 * scratch and bad 8); M < 0 or M * A > INT32_MAX; A outside [1, 64]; clip_param, huber_delta or vn_beta that
 * is not finite or is negative; an output that overlaps an input or another output. M == 0 is legal: it
 * writes nothing and leaves vn_state as it was.
 */
#ifndef LSM_LOSS_H
#define LSM_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_LOSS_GROUP 256 /* rows per group of the float64 sums, and per workgroup */

typedef struct lsm_loss_config {
  double vn_beta; /* ValueNorm's beta, 0.99999; a double, since (float)(1.0 - beta) is taken from it */
  float clip_param, huber_delta, value_loss_coef, entropy_coef;
  int32_t use_clipped_value_loss, use_huber_loss;
  int32_t use_value_active_masks, use_policy_active_masks;
  int32_t use_valuenorm; /* 0: the returns are used as they are */
  int32_t num_actions;   /* A in [1, 64], as lsm_head_config */
} lsm_loss_config;

/* One call's tensors, M rows: device pointers for lsm_ppo_loss, host pointers for lsm_host_ppo_loss. */
typedef struct lsm_loss_io {
  const float* logits;            /* [M][A], after the availability mask, as lsm_head_evaluate writes them */
  const float* actions;           /* [M] float32, the buffer's rows */
  const float* available_actions; /* [M][A], nullable */
  const float* old_log_probs;     /* [M] */
  const float* advantages;        /* [M] */
  const float* active_masks;      /* [M]; needed iff a flag of an enabled half asks for it */
  const float* values;            /* [M], the critic's output */
  const float* value_preds;       /* [M] */
  const float* returns;           /* [M] */
  float* vn_state;                /* [3] running_mean, running_mean_sq, debiasing_term; updated in place */
  float* denorm;                  /* [2] = {sqrt(var), mean} after the update, nullable */
  float* dlogits;                 /* [M][A] */
  float* dvalues;                 /* [M] */
  float* imp_weights;             /* [M], nullable */
  float* stats;                   /* [4] policy_loss, value_loss, dist_entropy, mean imp_weight */
  void* scratch;                  /* lsm_ppo_loss_scratch_bytes(M) bytes */
  int64_t* bad;                   /* [1], nullable; only ever set */
} lsm_loss_io;

/* Bytes of scratch for M rows: 8 doubles, and 8 more per group of LSM_LOSS_GROUP rows (at least one group);
 * 0 for M < 0. */
size_t lsm_ppo_loss_scratch_bytes(int64_t M);

int lsm_ppo_loss(lsm_loss_config cfg, const lsm_loss_io* io, int64_t M, void* hip_stream);

/* The same routine on host memory (all pointers host pointers), through the same per-row code. */
int lsm_host_ppo_loss(lsm_loss_config cfg, const lsm_loss_io* io, int64_t M);

const char* lsm_loss_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
