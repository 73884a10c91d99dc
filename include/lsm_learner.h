/*
 * lsm_learner.h -- C ABI of the learner-side hand-off from the device replay buffer.
 *
 * What the reference does with GraphReplayBuffer between the last env step and the first
 * ppo_update, on the device tensors of lsm.buffer.DeviceGraphBuffer:
 *
 *   lsm_buffer_compute_returns  GraphReplayBuffer.compute_returns (onpolicy/utils/graph_buffer.py:285-366)
 *   lsm_host_compute_returns    the same routine on host pointers (CPU tests pin the arithmetic)
 *   lsm_buffer_advantages       the head of GR_MAPPO.train (onpolicy/algorithms/graph_mappo.py:258-268)
 *   lsm_buffer_gather           one minibatch of GraphReplayBuffer.feed_forward_generator
 *                               (graph_buffer.py:368-453): every field's rows in one launch
 *
 * The declarations live apart from lsm_rollout.h: that header is part of the rollout's build id.
 * All device entry points are stream-ordered and asynchronous, with no host synchronisation.
 * Return value: 0 on success; nonzero on an argument error, before any launch, with the text in
 * lsm_returns_last_error() / lsm_gather_last_error() (thread-local).
 */
#ifndef LSM_LEARNER_H
#define LSM_LEARNER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- returns ------------------------------------------------------------------------------------
 * Buffers are [rows][M] float32 with M = n * N (the reference's trailing 1 dropped); one series per
 * column, scanned t = T-1 .. 0. Every operation is rounded to float32, in the reference's order:
 * g = (float)gamma, gl = (float)(gamma * gae_lambda) (product in double), dn(x) = x * denorm[0] +
 * denorm[1] (two roundings) or x without a normaliser, m = masks[t+1], b = bad_masks[t+1].
 *   GAE:    delta = (rewards[t] + (g * dn(v[t+1])) * m) - dn(v[t])
 *           gae = delta + (gl * gae) * m   with use_proper_time_limits and denorm,
 *           gae = delta + (gl * m) * gae   in every other branch; proper: gae = gae * b
 *           returns[t] = gae + dn(v[t])
 *   no GAE: x = ((returns[t+1] * g) * m) + rewards[t]; proper: x = x * b + (1 - b) * dn(v[t])
 *           returns[t] = x
 * Row T: with use_gae value_preds[T] = next_value and returns[T] is not written; without,
 * returns[T] = next_value and value_preds is not written. */
typedef struct lsm_returns_config {
  double gamma, gae_lambda;
  int32_t use_gae, use_proper_time_limits;
} lsm_returns_config;

int lsm_buffer_compute_returns(const float* rewards,   /* [T][M]   */
                               float* value_preds,      /* [T+1][M] */
                               const float* masks,      /* [T+1][M] */
                               const float* bad_masks,  /* [T+1][M]; NULL allowed unless proper */
                               const float* next_value, /* [M] */
                               const float* denorm,     /* device float[2] = {sqrt(var), mean}; NULL = no normaliser */
                               float* returns,          /* [T+1][M] */
                               int32_t T, int64_t M, const lsm_returns_config* cfg, void* hip_stream);
/* The same per-series routine on host memory (all pointers host pointers, denorm included). */
int lsm_host_compute_returns(const float* rewards, float* value_preds, const float* masks,
                             const float* bad_masks, const float* next_value, const float* denorm,
                             float* returns, int32_t T, int64_t M, const lsm_returns_config* cfg);

/* ---- advantages ---------------------------------------------------------------------------------
 * adv = returns - dn(value_preds) in float32 over the first count = T * M entries; mean and population
 * std over entries with active_masks != 0, in float64 with a fixed addition order (no floating-point
 * atomics: the result does not depend on scheduling); advantages = (adv - (float)mean) /
 * (float)(std + 1e-5). stats = {mean, std, active count}. No active entry: mean, std and every
 * advantage are NaN. Two launches: per-workgroup partials into the workspace, then the final sum and
 * the normalisation. */
size_t lsm_buffer_advantages_workspace_bytes(int64_t count);
int lsm_buffer_advantages(const float* returns, const float* value_preds, const float* active_masks,
                          const float* denorm, int64_t count, float* advantages /* [count] */,
                          double* stats /* device [3] */, void* workspace, size_t workspace_bytes,
                          void* hip_stream);
const char* lsm_returns_last_error(void);

/* ---- minibatch gather ---------------------------------------------------------------------------
 * dst[b] = src[indices[b]] for every field in one launch. LSM_GATHER_COMPACT_ADJ expands the compact
 * adjacency on the fly: dst[b][r][c] = (bit r | bit c of masks[i]) ? 0 : A[i / N][r][c], i =
 * indices[b] (a select, not a product). An index outside [0, rows) zero-fills that sample in every
 * field and sets *bad = 1 when bad is given; nothing out of bounds is read or written. Refused as
 * argument errors: a field with more than 2^32 - 2^19 copy units in one call (B * row_bytes / 16 where
 * row_bytes, src and dst are 16-byte aligned, B * row_bytes / 4 otherwise; split the minibatch), and a
 * compact adjacency field with rows >= 2^32. */
enum { LSM_GATHER_ROWS = 0, LSM_GATHER_COMPACT_ADJ = 1 };
enum { LSM_GATHER_MAX_FIELDS = 16 };
typedef struct lsm_gather_field {
  int32_t kind;
  const void* src;
  void* dst;
  int64_t row_bytes;     /* ROWS: bytes per sample row (multiple of 4) */
  const uint64_t* masks; /* COMPACT_ADJ: [rows][W] disconnect words, W = ceil(E/64) */
  int32_t E, N;          /* COMPACT_ADJ: src = A [rows/N][E][E] f32, dst = [B][E][E] f32 */
} lsm_gather_field;

int lsm_buffer_gather(const lsm_gather_field* fields, int32_t nfields /* <= LSM_GATHER_MAX_FIELDS */,
                      const int64_t* indices /* device [B] */, int64_t B, int64_t rows,
                      int64_t* bad /* device [1], nullable */, void* hip_stream);
const char* lsm_gather_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
