// lsm_train_info.hip -- GR_MAPPO.train's train_info on the device (include/lsm_train_info.h): the scalars of each
// ppo_update added where they lie, the means taken once after the last update.
//
// Reference: onpolicy/algorithms/graph_mappo.py:271-319.
//
// Two kernels of one workgroup each; lane k < LSM_TRAIN_INFO_SLOTS owns slot k.
//   add_kernel   lane k adds *src[k] into sum[k] in float64 and counts it; the lanes' non-finite flags meet in LDS
//                and lane 0 advances updates and first_nonfinite
//   mean_kernel  lane k divides (slots 0 .. 5) or copies (the two counts) and rounds to float32
// slot_add, finish_add and slot_mean are ONE __host__ __device__ text; the host entry points run them in the
// kernels' order. A call is bound by its launch: 8 loads, 8 float64 additions.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/lsm_train_info.h"

#define LSM_HD __host__ __device__ __forceinline__

namespace {

constexpr int SLOTS = LSM_TRAIN_INFO_SLOTS;
constexpr int MEANS = LSM_TRAIN_INFO_MEANS;
constexpr int LANES = LSM_TRAIN_INFO_LANES;
static_assert(SLOTS <= LANES, "one lane per slot");

struct State {
  double sum[SLOTS];
  int64_t n[SLOTS];
  int64_t updates;
  int64_t first_nonfinite;
};
static_assert(sizeof(State) == 8 * LSM_TRAIN_INFO_STATE_WORDS, "the header's state");

LSM_HD bool finite_(float x) { return fabsf(x) <= FLT_MAX; }

// slot k of one add call; returns whether it added a value that is not finite
LSM_HD bool slot_add(State* s, const float* p, int k, bool first) {
  if (!first && !p) return false;   // the slot keeps its sum and count
  double sum = first ? 0.0 : s->sum[k];
  int64_t n = first ? 0 : s->n[k];
  bool bad = false;
  if (p) {
    const float x = *p;
    sum = sum + (double)x;
    n = n + 1;
    bad = !finite_(x);
  }
  s->sum[k] = sum;
  s->n[k] = n;
  return bad;
}

// by one thread, after every slot: the call's index and the first non-finite call
LSM_HD void finish_add(State* s, bool any_bad, bool first) {
  const int64_t updates = first ? 0 : s->updates;
  int64_t fn = first ? -1 : s->first_nonfinite;
  if (fn == -1 && any_bad) fn = updates;
  s->first_nonfinite = fn;
  s->updates = updates + 1;
}

LSM_HD float slot_mean(const State* s, int k, int64_t num_updates) {
  return k < MEANS ? (float)(s->sum[k] / (double)num_updates) : (float)s->sum[k];
}

__global__ __launch_bounds__(LANES) void add_kernel(State* s, lsm_train_info_src src, int first) {
  __shared__ int bad[SLOTS];
  const int k = threadIdx.x;
  if (k < SLOTS) bad[k] = slot_add(s, src.value[k], k, first != 0) ? 1 : 0;
  __syncthreads();
  if (k == 0) {
    int any = 0;
    for (int i = 0; i < SLOTS; ++i) any |= bad[i];
    finish_add(s, any != 0, first != 0);
  }
}

__global__ __launch_bounds__(LANES) void mean_kernel(const State* s, int64_t num_updates, float* out) {
  const int k = threadIdx.x;
  if (k < SLOTS) out[k] = slot_mean(s, k, num_updates);
}

thread_local char g_err[256] = "";

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "train info: %s", msg);
  return 1;
}

// by differences: no sum of an address and a size that could wrap
bool overlaps_state(const void* state, const void* p, size_t bytes) {
  const uintptr_t a = (uintptr_t)state, b = (uintptr_t)p;
  return a < b ? b - a < sizeof(State) : a - b < bytes;
}

int check_state(const void* state) {
  if (!state) return fail("state is null");
  if ((uintptr_t)state & 7) return fail("state must be 8-byte aligned");
  return 0;
}

int check_add(const void* state, const lsm_train_info_src& src) {
  if (check_state(state)) return 1;
  for (int k = 0; k < SLOTS; ++k) {
    const float* p = src.value[k];
    if (!p) continue;
    if ((uintptr_t)p & 3) return fail("a src pointer is not 4-byte aligned");
    if (overlaps_state(state, p, sizeof(float))) return fail("a src pointer overlaps the state");
  }
  return 0;
}

int check_mean(const void* state, int64_t num_updates, const float* out) {
  if (check_state(state)) return 1;
  if (!out) return fail("out is null");
  if (num_updates < 1) return fail("num_updates must be >= 1");
  if ((uintptr_t)out & 3) return fail("out is not 4-byte aligned");
  if (overlaps_state(state, out, SLOTS * sizeof(float))) return fail("out overlaps the state");
  return 0;
}

}  // namespace

extern "C" {

const char* lsm_train_info_last_error(void) { return g_err; }

int lsm_train_info_add(void* state, lsm_train_info_src src, int32_t first, void* hip_stream) {
  if (check_add(state, src)) return 1;
  add_kernel<<<dim3(1), dim3(LANES), 0, (hipStream_t)hip_stream>>>(static_cast<State*>(state), src, first);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  return 0;
}

int lsm_train_info_mean(const void* state, int64_t num_updates, float* out, void* hip_stream) {
  if (check_mean(state, num_updates, out)) return 1;
  mean_kernel<<<dim3(1), dim3(LANES), 0, (hipStream_t)hip_stream>>>(static_cast<const State*>(state), num_updates,
                                                                     out);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  return 0;
}

int lsm_host_train_info_add(void* state, lsm_train_info_src src, int32_t first) {
  if (check_add(state, src)) return 1;
  State* s = static_cast<State*>(state);
  bool any = false;
  for (int k = 0; k < SLOTS; ++k) any = slot_add(s, src.value[k], k, first != 0) || any;
  finish_add(s, any, first != 0);
  return 0;
}

int lsm_host_train_info_mean(const void* state, int64_t num_updates, float* out) {
  if (check_mean(state, num_updates, out)) return 1;
  const State* s = static_cast<const State*>(state);
  for (int k = 0; k < SLOTS; ++k) out[k] = slot_mean(s, k, num_updates);
  return 0;
}

}  // extern "C"
