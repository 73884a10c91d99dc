/*
 * lsm_train_info.h -- C ABI of the tail of GR_MAPPO.train (onpolicy/algorithms/graph_mappo.py:271-319): the
 * train_info dict, accumulated on the device over the ppo_epoch * num_mini_batch calls of ppo_update and divided
 * once at the end. The scalars of one update (the loss's stats row, each optimiser group's info row) are only
 * valid until the next update; this unit adds them where they lie, so that no update of a train() call needs a
 * host read.
 *
 * SLOTS. LSM_TRAIN_INFO_SLOTS = 8, in this order:
 *   0 value_loss  1 policy_loss  2 dist_entropy  3 actor_grad_norm  4 critic_grad_norm  5 ratio
 *   6 actor_skipped  7 critic_skipped
 * Slots 0 .. 5 are the reference's six train_info keys in its own order. Slots 6 and 7 have no counterpart there:
 * they count the updates that a non-finite gradient skipped (lsm_optim.h's info.skipped, 0 or 1 per update), which
 * the reference's GradScaler hides.
 *
 * STATE. One object of LSM_TRAIN_INFO_STATE_WORDS = 18 8-byte words, 8-byte aligned:
 *   double  sum[8]            the slots' sums
 *   int64_t n[8]              how many values each slot took
 *   int64_t updates           the add calls since the state was started
 *   int64_t first_nonfinite   the index (0-based, in add calls) of the first call that added a non-finite value;
 *                             -1 while there was none
 *
 * lsm_train_info_add. src holds one nullable pointer per slot, each at one float32 (device memory). With
 * first != 0 the state is taken as started afresh (sums and counts 0, updates 0, first_nonfinite -1) whatever it
 * holds: garbage in it is overwritten and never read. Then, for each slot k with a non-null pointer,
 *   sum[k] = sum[k] + (double)*src[k]   and   n[k] = n[k] + 1
 * (one float64 addition per slot and call, so a sequence of calls adds in call order and is bit-reproducible). A
 * non-finite value is added like any other: the slot's sum, and with it its mean, goes non-finite as the reference's
 * does. If first_nonfinite is -1 and any value added by this call is not finite, first_nonfinite = updates. Then
 * updates = updates + 1. A slot with a null pointer keeps its sum and count. One launch of a single workgroup of
 * LSM_TRAIN_INFO_LANES threads: no atomics, no counter of finished blocks.
 *
 * lsm_train_info_mean. out[k] = (float)(sum[k] / (double)num_updates) for k < 6: the float64 quotient rounded to
 * float32 once; out[6] = (float)sum[6] and out[7] = (float)sum[7], counts that are not divided. num_updates is the
 * CALLER's ppo_epoch * num_mini_batch, as in the reference (graph_mappo.py:314-317); it is not the state's
 * `updates`, and not n[k] either. The reference divides by that product even when a generator yielded fewer
 * minibatches than num_mini_batch, or when a slot took no value (update_actor = False here: 0 / num_updates = 0),
 * and so does this call. The state is not changed. One launch.
 *
 * Both calls are stream-ordered and asynchronous, allocate nothing and never synchronise with the host. The host
 * entry points run the same text on host memory.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_train_info_last_error() (thread-local, prefix "train info: "). Refused: a null state; a null out;
 * num_updates < 1; a state that is not 8-byte aligned; a src[k] or an out that is not 4-byte aligned; an out or a
 * src[k] that overlaps the state.
 */
#ifndef LSM_TRAIN_INFO_H
#define LSM_TRAIN_INFO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSM_TRAIN_INFO_SLOTS 8
#define LSM_TRAIN_INFO_MEANS 6
#define LSM_TRAIN_INFO_STATE_WORDS 18
#define LSM_TRAIN_INFO_LANES 64

typedef struct lsm_train_info_src {
  const float* value[LSM_TRAIN_INFO_SLOTS]; /* one float32 each; null: the slot takes nothing from this call */
} lsm_train_info_src;

/* state, src.value[k]: device pointers. first != 0: the state starts afresh with this call. */
int lsm_train_info_add(void* state, lsm_train_info_src src, int32_t first, void* hip_stream);

/* out: float[LSM_TRAIN_INFO_SLOTS], device memory. num_updates: the caller's ppo_epoch * num_mini_batch. */
int lsm_train_info_mean(const void* state, int64_t num_updates, float* out, void* hip_stream);

/* The same routines on host memory (all pointers host pointers): the same text. */
int lsm_host_train_info_add(void* state, lsm_train_info_src src, int32_t first);
int lsm_host_train_info_mean(const void* state, int64_t num_updates, float* out);

const char* lsm_train_info_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
