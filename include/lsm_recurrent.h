/*
 * lsm_recurrent.h -- C ABI of the recurrent-policy hand-off from the device replay buffer.
 *
 * What the reference's default configuration (use_recurrent_policy, data_chunk_length = 10) does with
 * GraphReplayBuffer beyond include/lsm_learner.h, on the device tensors of lsm.buffer.DeviceGraphBuffer:
 *
 *   lsm_buffer_gather_chunks  one minibatch of GraphReplayBuffer.recurrent_generator
 *                             (onpolicy/utils/graph_buffer.py:597-755): every field's chunks in one launch
 *   lsm_host_gather_chunks    the same routine on host pointers (CPU tests pin the arithmetic)
 *   lsm_buffer_copy_rows      the policy half of GMPERunner.insert + GraphReplayBuffer.insert
 *                             (graph_mpe_runner.py:449-456, graph_buffer.py:229-249): one launch per step
 *
 * The declarations live apart from lsm_rollout.h (part of the rollout's build id) and from
 * lsm_learner.h. The device entry points are stream-ordered and asynchronous, with no host
 * synchronisation. Return value: 0 on success; nonzero on an argument error, before any launch or
 * write, with the text in lsm_recurrent_last_error() (thread-local; prefixes "gather_chunks: " and
 * "copy_rows: ").
 */
#ifndef LSM_RECURRENT_H
#define LSM_RECURRENT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- chunk gather -------------------------------------------------------------------------------
 * Buffers are [T(+1)][M][row], M = n * N, column = env * N + agent. The reference's (env, agent, t)
 * view puts sample f at column f / T and time f % T. Chunk c covers f = c * L + l, l = 0 .. L-1 (it may
 * run from the end of one column's series into the start of the next); data_chunks = (T * M) / L, the
 * tail is dropped. With row(c, l) = (f % T) * M + f / T and b the position of a chunk in chunks[0..C):
 *   LSM_CHUNK_ROWS         dst[l * C + b] = src[row(c_b, l)]
 *   LSM_CHUNK_COMPACT_ADJ  dst[l * C + b][r][k] = (bit r | bit k of masks[i]) ? 0 : A[i / N][r][k],
 *                          i = row(c_b, l) (a select, not a product)
 *   LSM_CHUNK_FIRST_ROW    dst[b] = src[row(c_b, 0)] (the recurrent states at a chunk's first step)
 * A chunk id outside [0, data_chunks) zero-fills its L destination rows (one for FIRST_ROW) in every
 * field and sets *bad = 1 when bad is given; no address is formed from it. Duplicate ids are allowed.
 * Refused as argument errors: L < 1, L > T * M, C < 1, T * M >= 2^32, a field with more than
 * 2^32 - 2^19 copy units in one call (destination rows * row_bytes / 16 where row_bytes, src and dst
 * are 16-byte aligned, / 4 otherwise; split the minibatch), pointers not 4-byte aligned, row_bytes not
 * a positive multiple of 4, an unknown kind, and a compact field with (T * M) % N != 0. */
enum { LSM_CHUNK_ROWS = 0, LSM_CHUNK_COMPACT_ADJ = 1, LSM_CHUNK_FIRST_ROW = 2 };
enum { LSM_CHUNK_MAX_FIELDS = 16 };
typedef struct lsm_chunk_field {
  int32_t kind;
  const void* src;
  void* dst;
  int64_t row_bytes;     /* ROWS, FIRST_ROW: bytes per sample row (multiple of 4) */
  const uint64_t* masks; /* COMPACT_ADJ: [T * M][W] disconnect words, W = ceil(E/64) */
  int32_t E, N;          /* COMPACT_ADJ: src = A [T * M / N][E][E] f32, dst = [L * C][E][E] f32 */
} lsm_chunk_field;

int lsm_buffer_gather_chunks(const lsm_chunk_field* fields, int32_t nfields /* <= LSM_CHUNK_MAX_FIELDS */,
                             const int64_t* chunks /* device [C] */, int64_t C, int64_t L, int64_t T,
                             int64_t M, int64_t* bad /* device [1], nullable */, void* hip_stream);
/* The same routine on host memory (all pointers host pointers). */
int lsm_host_gather_chunks(const lsm_chunk_field* fields, int32_t nfields, const int64_t* chunks, int64_t C,
                           int64_t L, int64_t T, int64_t M, int64_t* bad);

/* ---- per-step row copies ------------------------------------------------------------------------
 * dst[m] = (zero_on_done && dones[m] != 0) ? 0 : src[m] for m = 0 .. M-1 and every copy, in one launch:
 * actions, action_log_probs and value_preds into buffer row t, rnn_states and rnn_states_critic (zeroed
 * where the agent is done) and available_actions into row t + 1. Launch it on the env's stream after
 * the step that produced dones. Refused: ncopies outside 1..8, M < 1, null or misaligned (4 B)
 * pointers, row_bytes not a positive multiple of 4, zero_on_done without dones, and a copy with more
 * than 2^32 - 2^19 copy units. */
enum { LSM_COPY_MAX = 8 };
typedef struct lsm_row_copy {
  const void* src;      /* [M][row_bytes] */
  void* dst;            /* [M][row_bytes] */
  int64_t row_bytes;
  int32_t zero_on_done;
} lsm_row_copy;

int lsm_buffer_copy_rows(const lsm_row_copy* copies, int32_t ncopies /* <= LSM_COPY_MAX */,
                         const uint8_t* dones /* device [M], nullable */, int64_t M, void* hip_stream);

const char* lsm_recurrent_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
