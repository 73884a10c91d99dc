// lsm_returns.hip -- GraphReplayBuffer.compute_returns and the advantage normalisation on the device.
//
// Reference: onpolicy/utils/graph_buffer.py:285-366 (compute_returns: a T-step reverse scan per
// (env, agent) series, GAE or discounted, with or without use_proper_time_limits, with or without the
// value normaliser's denormalize) and onpolicy/algorithms/graph_mappo.py:258-268 (advantages =
// returns[:-1] - denormalize(value_preds[:-1]), normalised by the mean / std of the active entries).
//
// Returns: buffers are [rows][M] float32, M = n * N. One thread per series, no barriers; row t is
// contiguous, so a wave's loads are 256 contiguous bytes. The per-series routine is ONE
// __host__ __device__ function (returns_series): lsm_host_compute_returns runs the same text on the
// CPU, float32 operation by operation in the reference's order (the build has -ffp-contract=off), so
// the kernel is held to bit equality with the reference on a machine without a GPU.
//
// Block size (reasoned, not measured against 256): the scan is a chain of T dependent steps per thread
// with about 16 B loaded per step, so latency should bound it, and at the headline shape (M = 32768)
// there are only 512 waves of work for 256 CUs x 4 SIMDs. 64-thread workgroups make that 512
// workgroups, which can spread over every CU; 256-thread workgroups would be 128 workgroups on at most
// half of the CUs. Nothing is shared within a workgroup (no LDS, no barrier), so the smaller workgroup
// gives nothing up.
//
// Advantages: two launches. advantages_partial_kernel writes adv = returns - dn(value_preds) (float32)
// and each workgroup's float64 (sum, sum of squares, count) over active entries into the workspace;
// advantages_finish_kernel adds the partials (every workgroup the same additions in the same order),
// writes stats and normalises. Every addition order is fixed by (count, grid), never by scheduling:
// no floating-point atomics. The launch boundary is the only ordering between the two.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/lsm_learner.h"

namespace {

constexpr int RET_BLOCK = 64;
constexpr int ADV_BLOCK = 256;
constexpr int ADV_MAX_BLOCKS = 256;   // partials: one per thread of the finishing workgroups
constexpr int ADV_UNROLL = 4;
static_assert(ADV_MAX_BLOCKS <= ADV_BLOCK, "advantages_finish_kernel loads one partial per thread");

template <bool DN>
__host__ __device__ __forceinline__ float dn(float x, float scale, float mean) {
  if (!DN) return x;
  const float p = x * scale;
  return p + mean;
}

// One series (column j). The loads of step t-1 do not depend on the chain, so they are issued before
// step t's arithmetic.
template <bool GAE, bool PROPER, bool DN>
__host__ __device__ __forceinline__ void returns_series(const float* rewards, float* value_preds, const float* masks,
                                                        const float* bad_masks, const float* next_value,
                                                        const float* denorm, float* returns, int32_t T, int64_t M,
                                                        int64_t j, float g, float gl) {
  const float scale = DN ? denorm[0] : 1.0f, mean = DN ? denorm[1] : 0.0f;
  const float nv = next_value[j];
  constexpr bool NEED_V = GAE || PROPER;
  const int64_t top = (int64_t)T * M + j;
  if (GAE) value_preds[top] = nv;
  else returns[top] = nv;
  int64_t at = top - M;   // (t, j), t = T-1
  float r = rewards[at], m = masks[at + M];
  float v = NEED_V ? value_preds[at] : 0.0f;
  float b = PROPER ? bad_masks[at + M] : 1.0f;
  float gae = 0.0f;
  float nxt = GAE ? dn<DN>(nv, scale, mean) : nv;   // GAE: dn(v[t+1]); otherwise returns[t+1]
  for (int32_t t = T - 1; t >= 0; --t) {
    float r1 = 0.0f, m1 = 0.0f, v1 = 0.0f, b1 = 1.0f;
    if (t > 0) {
      r1 = rewards[at - M];
      m1 = masks[at];
      if (NEED_V) v1 = value_preds[at - M];
      if (PROPER) b1 = bad_masks[at];
    }
    float out;
    if (GAE) {
      const float dv = dn<DN>(v, scale, mean);
      const float gv = g * nxt;
      const float gvm = gv * m;
      const float rg = r + gvm;
      const float delta = rg - dv;
      float carry;
      if (PROPER && DN) {
        const float q = gl * gae;
        carry = q * m;
      } else {
        const float q = gl * m;
        carry = q * gae;
      }
      gae = delta + carry;
      if (PROPER) gae = gae * b;
      out = gae + dv;
      nxt = dv;
    } else {
      const float xg = nxt * g;
      const float xm = xg * m;
      float x = xm + r;
      if (PROPER) {
        const float xb = x * b;
        const float ob = 1.0f - b;
        const float dv = dn<DN>(v, scale, mean);
        const float od = ob * dv;
        x = xb + od;
      }
      out = x;
      nxt = x;
    }
    returns[at] = out;
    r = r1;
    m = m1;
    v = v1;
    b = b1;
    at -= M;
  }
}

struct ReturnsArgs {
  const float* rewards;
  float* value_preds;
  const float* masks;
  const float* bad_masks;
  const float* next_value;
  const float* denorm;
  float* returns;
  int32_t T;
  int64_t M;
  float g, gl;
};

template <bool GAE, bool PROPER, bool DN>
__global__ __launch_bounds__(RET_BLOCK) void returns_kernel(ReturnsArgs a) {
  const int64_t j = (int64_t)blockIdx.x * RET_BLOCK + threadIdx.x;
  if (j >= a.M) return;
  returns_series<GAE, PROPER, DN>(a.rewards, a.value_preds, a.masks, a.bad_masks, a.next_value, a.denorm, a.returns,
                                  a.T, a.M, j, a.g, a.gl);
}

template <bool GAE, bool PROPER, bool DN>
void returns_host(const ReturnsArgs& a) {
  for (int64_t j = 0; j < a.M; ++j)
    returns_series<GAE, PROPER, DN>(a.rewards, a.value_preds, a.masks, a.bad_masks, a.next_value, a.denorm,
                                    a.returns, a.T, a.M, j, a.g, a.gl);
}

template <bool GAE, bool PROPER, bool DN>
void returns_launch(const ReturnsArgs& a, hipStream_t st) {
  const unsigned blocks = (unsigned)((a.M + RET_BLOCK - 1) / RET_BLOCK);
  returns_kernel<GAE, PROPER, DN><<<blocks, RET_BLOCK, 0, st>>>(a);
}

// calls F<GAE, PROPER, DN> for the branch (use_gae, proper, denorm != NULL)
#define LSM_RETURNS_DISPATCH(F, gae, proper, den, ...)                   \
  switch (((gae) ? 4 : 0) | ((proper) ? 2 : 0) | ((den) ? 1 : 0)) {      \
    case 0: F<false, false, false>(__VA_ARGS__); break;                  \
    case 1: F<false, false, true>(__VA_ARGS__); break;                   \
    case 2: F<false, true, false>(__VA_ARGS__); break;                   \
    case 3: F<false, true, true>(__VA_ARGS__); break;                    \
    case 4: F<true, false, false>(__VA_ARGS__); break;                   \
    case 5: F<true, false, true>(__VA_ARGS__); break;                    \
    case 6: F<true, true, false>(__VA_ARGS__); break;                    \
    default: F<true, true, true>(__VA_ARGS__); break;                    \
  }

// ---- advantages -----------------------------------------------------------------------------------

struct Sums {
  double s, q, n;
};

// Workgroup total with a fixed order: xor butterfly inside each wave (every lane ends with the same
// bits: each level adds the same two operands in either order), then the wave totals in wave order.
__device__ __forceinline__ Sums block_total(Sums x, double (*lds)[3]) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    x.s = x.s + __shfl_xor(x.s, off);
    x.q = x.q + __shfl_xor(x.q, off);
    x.n = x.n + __shfl_xor(x.n, off);
  }
  const int wv = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds[wv][0] = x.s;
    lds[wv][1] = x.q;
    lds[wv][2] = x.n;
  }
  __syncthreads();
  Sums tot{lds[0][0], lds[0][1], lds[0][2]};
  for (int w = 1; w < ADV_BLOCK / 64; ++w) {
    tot.s += lds[w][0];
    tot.q += lds[w][1];
    tot.n += lds[w][2];
  }
  return tot;
}

// Workgroup k, round i covers elements (i * gridDim.x + k) * ADV_BLOCK * ADV_UNROLL + u * ADV_BLOCK + t:
// which elements a thread adds, and in which order, depends on (count, gridDim.x) only.
template <bool DN>
__global__ __launch_bounds__(ADV_BLOCK) void advantages_partial_kernel(const float* __restrict__ returns,
                                                                       const float* __restrict__ value_preds,
                                                                       const float* __restrict__ active,
                                                                       const float* __restrict__ denorm, int64_t count,
                                                                       float* __restrict__ adv,
                                                                       double* __restrict__ partials) {
  __shared__ double lds[ADV_BLOCK / 64][3];
  const float scale = DN ? denorm[0] : 1.0f, mean = DN ? denorm[1] : 0.0f;
  constexpr int64_t TILE = (int64_t)ADV_BLOCK * ADV_UNROLL;
  Sums acc{0.0, 0.0, 0.0};
  for (int64_t base = (int64_t)blockIdx.x * TILE; base < count; base += (int64_t)gridDim.x * TILE) {
    float rr[ADV_UNROLL], vv[ADV_UNROLL], aa[ADV_UNROLL];
#pragma unroll
    for (int u = 0; u < ADV_UNROLL; ++u) {
      const int64_t i = base + u * ADV_BLOCK + threadIdx.x;
      const bool in = i < count;
      rr[u] = in ? returns[i] : 0.0f;
      vv[u] = in ? value_preds[i] : 0.0f;
      aa[u] = in ? active[i] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < ADV_UNROLL; ++u) {
      const int64_t i = base + u * ADV_BLOCK + threadIdx.x;
      if (i < count) {
        const float d = rr[u] - dn<DN>(vv[u], scale, mean);
        adv[i] = d;
        if (aa[u] != 0.0f) {
          const double x = (double)d;
          acc.s += x;
          acc.q += x * x;
          acc.n += 1.0;
        }
      }
    }
  }
  const Sums tot = block_total(acc, lds);
  if (threadIdx.x == 0) {
    partials[3 * blockIdx.x + 0] = tot.s;
    partials[3 * blockIdx.x + 1] = tot.q;
    partials[3 * blockIdx.x + 2] = tot.n;
  }
}

__global__ __launch_bounds__(ADV_BLOCK) void advantages_finish_kernel(const double* __restrict__ partials,
                                                                      int npartials, int64_t count,
                                                                      float* __restrict__ adv,
                                                                      double* __restrict__ stats) {
  __shared__ double lds[ADV_BLOCK / 64][3];
  Sums x{0.0, 0.0, 0.0};
  if ((int)threadIdx.x < npartials) {   // npartials <= ADV_MAX_BLOCKS == ADV_BLOCK
    x.s = partials[3 * threadIdx.x + 0];
    x.q = partials[3 * threadIdx.x + 1];
    x.n = partials[3 * threadIdx.x + 2];
  }
  const Sums tot = block_total(x, lds);
  // n == 0: 0 / 0 = NaN for the mean, the std and every advantage (np.nanmean of an all-NaN array)
  const double mean = tot.s / tot.n;
  double var = tot.q / tot.n - mean * mean;
  if (var < 0.0) var = 0.0;   // NaN stays NaN
  const double sd = sqrt(var);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = sd;
    stats[2] = tot.n;
  }
  const float mf = (float)mean, df = (float)(sd + 1e-5);
  for (int64_t i = (int64_t)blockIdx.x * ADV_BLOCK + threadIdx.x; i < count; i += (int64_t)gridDim.x * ADV_BLOCK) {
    const float c = adv[i] - mf;
    adv[i] = c / df;
  }
}

int adv_partial_blocks(int64_t count) {
  const int64_t tile = (int64_t)ADV_BLOCK * ADV_UNROLL;
  const int64_t b = (count + tile - 1) / tile;
  return (int)(b < 1 ? 1 : (b > ADV_MAX_BLOCKS ? ADV_MAX_BLOCKS : b));
}

thread_local char g_err[256];

int fail(const char* m) {
  snprintf(g_err, sizeof g_err, "%s", m);
  return 1;
}

// shared argument check of the two compute_returns entry points; 0 when fine
int check_returns(const float* rewards, const float* value_preds, const float* masks, const float* bad_masks,
                  const float* next_value, const float* returns, int32_t T, int64_t M,
                  const lsm_returns_config* cfg) {
  if (!cfg) return fail("compute_returns: null config");
  if (T < 1) return fail("compute_returns: T < 1");
  if (M < 1) return fail("compute_returns: M < 1");
  if (!rewards || !value_preds || !masks || !next_value || !returns)
    return fail("compute_returns: null rewards / value_preds / masks / next_value / returns pointer");
  if (cfg->use_proper_time_limits && !bad_masks) return fail("compute_returns: use_proper_time_limits without bad_masks");
  return 0;
}

ReturnsArgs returns_args(const float* rewards, float* value_preds, const float* masks, const float* bad_masks,
                         const float* next_value, const float* denorm, float* returns, int32_t T, int64_t M,
                         const lsm_returns_config* cfg) {
  return ReturnsArgs{rewards, value_preds, masks, bad_masks, next_value, denorm, returns, T, M,
                     (float)cfg->gamma, (float)(cfg->gamma * cfg->gae_lambda)};
}

}  // namespace

extern "C" {

const char* lsm_returns_last_error(void) { return g_err; }

int lsm_buffer_compute_returns(const float* rewards, float* value_preds, const float* masks, const float* bad_masks,
                               const float* next_value, const float* denorm, float* returns, int32_t T, int64_t M,
                               const lsm_returns_config* cfg, void* hip_stream) {
  if (check_returns(rewards, value_preds, masks, bad_masks, next_value, returns, T, M, cfg)) return 1;
  if ((M + RET_BLOCK - 1) / RET_BLOCK > 0x7fffffffLL) return fail("compute_returns: M too large for one grid");
  const ReturnsArgs a = returns_args(rewards, value_preds, masks, bad_masks, next_value, denorm, returns, T, M, cfg);
  LSM_RETURNS_DISPATCH(returns_launch, cfg->use_gae, cfg->use_proper_time_limits, denorm != nullptr, a,
                       (hipStream_t)hip_stream)
  return hipGetLastError() == hipSuccess ? 0 : fail("returns_kernel launch failed");
}

int lsm_host_compute_returns(const float* rewards, float* value_preds, const float* masks, const float* bad_masks,
                             const float* next_value, const float* denorm, float* returns, int32_t T, int64_t M,
                             const lsm_returns_config* cfg) {
  if (check_returns(rewards, value_preds, masks, bad_masks, next_value, returns, T, M, cfg)) return 1;
  const ReturnsArgs a = returns_args(rewards, value_preds, masks, bad_masks, next_value, denorm, returns, T, M, cfg);
  LSM_RETURNS_DISPATCH(returns_host, cfg->use_gae, cfg->use_proper_time_limits, denorm != nullptr, a)
  return 0;
}

size_t lsm_buffer_advantages_workspace_bytes(int64_t count) {
  return (size_t)adv_partial_blocks(count) * 3 * sizeof(double);
}

int lsm_buffer_advantages(const float* returns, const float* value_preds, const float* active_masks,
                          const float* denorm, int64_t count, float* advantages, double* stats, void* workspace,
                          size_t workspace_bytes, void* hip_stream) {
  if (count < 1) return fail("advantages: count < 1");
  if (!returns || !value_preds || !active_masks || !advantages || !stats)
    return fail("advantages: null returns / value_preds / active_masks / advantages / stats pointer");
  if (!workspace) return fail("advantages: null workspace");
  if (workspace_bytes < lsm_buffer_advantages_workspace_bytes(count)) return fail("advantages: workspace too small");
  if (((uintptr_t)workspace & 7) != 0 || ((uintptr_t)stats & 7) != 0)
    return fail("advantages: workspace / stats not 8-byte aligned");
  const hipStream_t st = (hipStream_t)hip_stream;
  const int nb = adv_partial_blocks(count);
  double* partials = (double*)workspace;
  if (denorm)
    advantages_partial_kernel<true><<<nb, ADV_BLOCK, 0, st>>>(returns, value_preds, active_masks, denorm, count,
                                                               advantages, partials);
  else
    advantages_partial_kernel<false><<<nb, ADV_BLOCK, 0, st>>>(returns, value_preds, active_masks, denorm, count,
                                                                advantages, partials);
  if (hipGetLastError() != hipSuccess) return fail("advantages_partial_kernel launch failed");
  int64_t fb = (count + ADV_BLOCK * ADV_UNROLL - 1) / (ADV_BLOCK * ADV_UNROLL);
  if (fb > 2048) fb = 2048;
  advantages_finish_kernel<<<(unsigned)fb, ADV_BLOCK, 0, st>>>(partials, nb, count, advantages, stats);
  return hipGetLastError() == hipSuccess ? 0 : fail("advantages_finish_kernel launch failed");
}

}  // extern "C"
