// lsm_loss.hip -- the PPO loss and its gradient at the heads' outputs (include/lsm_loss.h): the clipped
// surrogate, the clipped Huber / MSE value loss, ValueNorm's update and normalisation of the returns and the
// active-mask weighting, from the logits and values that the heads' sequence form leaves on the device.
//
// Reference: GR_MAPPO.ppo_update and cal_value_loss (onpolicy/algorithms/graph_mappo.py), huber_loss / mse_loss
// (onpolicy/utils/util.py), ValueNorm.update / normalize (onpolicy/utils/valuenorm.py), FixedCategorical.
//
// Work split: a 256-thread workgroup owns a group of 256 consecutive rows, lane = row. The work is
// memory-bound (A + 8 floats read, A + 1 written per row) and a lane-per-row walk of [M][A] in global memory
// would stride by 4 A bytes, so the group's contiguous rows x A logits are staged through LDS with coalesced
// loads (the availability mask applied on the way), each lane walks its own LDS row -- the row stride is
// A | 1 floats: odd, so the 64 lanes of a wave hit 64 different banks at every a -- overwrites it with the
// row's dlogits, and the tile goes back out coalesced. The per-row scalars are read and written lane = row,
// which is coalesced as it is.
//
// Four launches (the dependencies: every row's value loss needs the normaliser, which needs every row's
// return; every gradient needs the sums of the weights):
//   pre_kernel     per group, the sums that do not depend on the network: Sw_p, Sw_v, Sr, Sr2
//   norm_kernel    one workgroup: the groups' sums in order, then one thread updates vn_state and leaves
//                  Sw_p, Sw_v, mean and std in the scratch's first 8 doubles
//   rows_kernel    per group, the rows: gradients out, the group's four statistics sums to scratch
//   finish_kernel  one workgroup: the groups' statistics in order, divided, rounded once
// Within a group the lanes' float64 terms go through LDS and threads 0 .. 3 add one quantity each, rows
// ascending; the one-workgroup launches stage 256 groups' sums at a time through LDS (coalesced, the next
// stage prefetched into registers) and threads 0 .. 3 add them, groups ascending: one fixed order, no
// atomics, no last-block-done counter.
//
// The per-row text is ONE __host__ __device__ text; lsm_host_ppo_loss runs it with a tile of one row and adds
// the terms in the kernels' order.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_loss.h"
#include "lsm_head_tile.h"

namespace {

using namespace lsm_head_tile;

constexpr int GROUP = LSM_LOSS_GROUP;
static_assert(GROUP == BLOCK, "a workgroup owns one group, lane = row");
constexpr int HEADER = 8;      // scratch[0 .. 8): Sw_p, Sw_v, Sr, Sr2, mean, std, unused, unused
constexpr int PER_GROUP = 8;   // scratch[8 + 8 g ..): the group's Sw_p, Sw_v, Sr, Sr2; then its sums of
                               // w_p * min(surr1, surr2), w_p * H, ratio, w_v * loss
constexpr int MAX_LDS_BYTES = GROUP * (MAX_ACTIONS | 1) * 4 + 4 * GROUP * 8;   // 74752

struct Loss {
  lsm_loss_config c;
  lsm_loss_io io;
  int64_t M, groups;
  int32_t A, S;            // S: the LDS row stride in floats, odd
  int32_t actor, critic;   // the enabled halves
  int32_t pmask, vmask;    // whether w_p / w_v is active_masks
  int32_t vn;              // ValueNorm, with the critic half
  float lo, hi;            // the ratio's clamp: (float)(1.0 - c), (float)(1.0 + c)
  float wb, om;            // (float)beta, (float)(1.0 - beta)
};

// the four sums of row m that do not depend on the network
LSM_HD void pre_row(const Loss& n, int64_t m, double* q) {
  q[0] = n.pmask ? (double)n.io.active_masks[m] : 1.0;
  q[1] = n.vmask ? (double)n.io.active_masks[m] : 1.0;
  const double r = n.critic ? (double)n.io.returns[m] : 0.0;
  q[2] = r;
  q[3] = r * r;
}

// ValueNorm.update, then running_mean_var(): the header's formulas, by one thread
LSM_HD void normalise(const Loss& n, const double* sums, double* header) {
  for (int k = 0; k < 4; ++k) header[k] = sums[k];
  float mean = 0.0f, sd = 1.0f;
  if (n.vn) {
    float* st = n.io.vn_state;
    const float bm = (float)(sums[2] / (double)n.M), bs = (float)(sums[3] / (double)n.M);
    float rm = st[0] * n.wb;
    rm = rm + bm * n.om;
    float rms = st[1] * n.wb;
    rms = rms + bs * n.om;
    float db = st[2] * n.wb;
    db = db + n.om;
    st[0] = rm, st[1] = rms, st[2] = db;
    const float den = db < 1e-5f ? 1e-5f : db;
    const float dm = rm / den, dms = rms / den;
    float var = dms - dm * dm;
    var = var < 1e-2f ? 1e-2f : var;   // a NaN stays a NaN, as under torch's clamp
    mean = dm, sd = sqrtf(var);
    if (n.io.denorm) n.io.denorm[0] = sd, n.io.denorm[1] = mean;
  }
  header[4] = (double)mean;
  header[5] = (double)sd;
  header[6] = header[7] = 0.0;
}

// the reference's huber_loss (b = 1[e > delta], not 1[|e| > delta]) or mse_loss, and its derivative
LSM_HD float value_loss(const Loss& n, float e, float& de) {
  if (!n.c.use_huber_loss) {
    de = e;
    return (e * e) / 2.0f;
  }
  const float dl = n.c.huber_delta;
  const float a = fabsf(e) <= dl ? 1.0f : 0.0f, b = e > dl ? 1.0f : 0.0f;
  de = a * e + b * dl;
  return (a * (e * e)) / 2.0f + (b * dl) * (fabsf(e) - dl / 2.0f);
}

// the larger (sign > 0) or smaller of two floats as torch.max / torch.min give it: a NaN in either is a NaN
LSM_HD float pick(float x, float y, int sign) {
  if (x != x) return x;
  if (y != y) return y;
  return (sign > 0 ? x > y : x < y) ? x : y;
}

// a row's scalars, read before anything else so that the loads are in flight together
struct Row {
  float action, old, adv, am, v, vp, ret;
};

LSM_HD Row load_row(const Loss& n, int64_t m) {
  Row r = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  if (n.actor) r.action = n.io.actions[m], r.old = n.io.old_log_probs[m], r.adv = n.io.advantages[m];
  if (n.pmask || n.vmask) r.am = n.io.active_masks[m];
  if (n.critic) r.v = n.io.values[m], r.vp = n.io.value_preds[m], r.ret = n.io.returns[m];
  return r;
}

// The actor half of row m in one lane. lg: the row's masked logits (an LDS row), overwritten with its
// dlogits. q[0 .. 3): w_p * min(surr1, surr2), w_p * H, ratio.
LSM_HD void actor_row(const Loss& n, int64_t m, const Row& x, float* lg, float swp, double* q) {
  const int A = n.A;
  float mx, s;
  int first;
  masked_softmax(lg, A, nullptr, nullptr, mx, first, s);   // the mask was applied when the row was staged
  bool bad;
  const int act = clamp_action(x.action, A, bad);
  if (bad && n.io.bad) *n.io.bad = 1;
  const float ls = logf(s);
  const float logp = (lg[act] - mx) - ls;
  float sum = 0.0f;
#pragma unroll 4
  for (int a = 0; a < A; ++a) {
    const float d = lg[a] - mx;
    const float e = expf(d);
    if (e > 0.0f) sum += (e / s) * (d - ls);
  }
  const float H = -sum;
  const float ratio = expf(logp - x.old);
  const float adv = x.adv;
  const float surr1 = ratio * adv;
  const float cl = ratio < n.lo ? n.lo : ratio > n.hi ? n.hi : ratio;
  const float surr2 = cl * adv;
  const float mn = pick(surr1, surr2, -1);
  const float t1 = surr1 < surr2 ? 1.0f : surr2 < surr1 ? 0.0f : 0.5f;
  const float inr = ratio >= n.lo && ratio <= n.hi ? 1.0f : 0.0f;
  const float g = adv * (t1 + (1.0f - t1) * inr);
  const float wp = n.pmask ? x.am : 1.0f;
  const float kp = wp / swp;
  const float dlogp = -(kp * (g * ratio));
  const float dent = -(n.c.entropy_coef * kp);
#pragma unroll 4
  for (int a = 0; a < A; ++a) {
    const float d = lg[a] - mx;
    const float e = expf(d);
    const float hot = a == act ? 1.0f : 0.0f;
    float gr;
    if (e > 0.0f) {
      const float p = e / s;
      gr = dlogp * (hot - p) + dent * (-(p * ((d - ls) + H)));
    } else {
      gr = a == act ? dlogp : 0.0f;
    }
    lg[a] = gr;
  }
  if (n.io.imp_weights) n.io.imp_weights[m] = ratio;
  q[0] = (double)mn * (double)wp;
  q[1] = (double)H * (double)wp;
  q[2] = (double)ratio;
}

// The critic half of row m. q[3]: w_v * loss.
LSM_HD void critic_row(const Loss& n, int64_t m, const Row& x, float swv, float mean, float sd, double* q) {
  const float v = x.v, vp = x.vp, ret = x.ret;
  const float c = n.c.clip_param;
  const float d = v - vp;
  const float dc = d < -c ? -c : d > c ? c : d;
  const float vpc = vp + dc;
  const float tg = n.vn ? (ret - mean) / sd : ret;
  float go, gc;
  const float lo = value_loss(n, tg - v, go);
  const float lc = value_loss(n, tg - vpc, gc);
  const float wv = n.vmask ? x.am : 1.0f;
  const float k = (wv / swv) * n.c.value_loss_coef;
  float l = lo, dv = -(k * go);
  if (n.c.use_clipped_value_loss) {
    l = pick(lo, lc, 1);
    const float to = lo > lc ? 1.0f : lc > lo ? 0.0f : 0.5f;
    // selected, not multiplied, as torch's masked_fill / where: a NaN k (no active row) leaves exactly 0
    const float ko = to > 0.0f ? k * to : 0.0f;
    const float kc = to < 1.0f && d >= -c && d <= c ? k * (1.0f - to) : 0.0f;
    dv = -(ko * go + kc * gc);
  }
  n.io.dvalues[m] = dv;
  q[3] = (double)l * (double)wv;
}

constexpr int BATCH = 8;   // elements a thread moves per round of the staging loops: that many loads in flight

// One tile: rows m0 .. m0 + rows - 1, one thread per row of the tile's capacity R (256 on the device, 1 on
// the host); lane >= rows: an idle lane that keeps the barriers uniform. L: R rows of S floats; P: [4][R]
// doubles, the lanes' terms (0 for an idle lane or a skipped half). No path leaves before the last barrier.
LSM_HD void loss_tile(const Loss& n, int64_t m0, int rows, int lane, int R, float* L, double* P) {
  const int A = n.A, S = n.S, total = rows * A;
  const double* hd = reinterpret_cast<const double*>(n.io.scratch);
  const int64_t base = m0 * A;
  const float* av = n.io.available_actions;
  Row x = {0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f};
  if (lane < rows) x = load_row(n, m0 + lane);
  // element i = r * A + c of the tile, i = lane, lane + R, ...: (r, c) advance by (R / A, R % A) with a carry,
  // one division per thread instead of one per element; BATCH elements are read before the first is used
  const int qa = R / A, ra = R - qa * A;
  const int r0 = lane / A, c0 = lane - r0 * A;
  if (n.actor) {
    for (int i0 = lane, r = r0, c = c0; i0 < total; i0 += BATCH * R) {
      float l[BATCH], m[BATCH];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        const int i = i0 + k * R;
        l[k] = i < total ? n.io.logits[base + i] : 0.0f;
        m[k] = av && i < total ? av[base + i] : 1.0f;
      }
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        if (i0 + k * R < total) L[r * S + c] = m[k] == 0.0f ? -FLT_MAX : l[k];
        r += qa, c += ra;
        if (c >= A) c -= A, ++r;
      }
    }
    LSM_SYNC();
  }
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  if (lane < rows) {
    const int64_t m = m0 + lane;
    if (n.actor) actor_row(n, m, x, L + lane * S, (float)hd[0], q);
    if (n.critic) critic_row(n, m, x, (float)hd[1], (float)hd[4], (float)hd[5], q);
  }
  for (int k = 0; k < 4; ++k) P[k * R + lane] = q[k];
  LSM_SYNC();
  if (n.actor) {
    for (int i0 = lane, r = r0, c = c0; i0 < total; i0 += BATCH * R) {
      float m[BATCH];
#pragma unroll
      for (int k = 0; k < BATCH; ++k) m[k] = av && i0 + k * R < total ? av[base + i0 + k * R] : 1.0f;
#pragma unroll
      for (int k = 0; k < BATCH; ++k) {
        if (i0 + k * R < total) n.io.dlogits[base + i0 + k * R] = m[k] == 0.0f ? 0.0f : L[r * S + c];
        r += qa, c += ra;
        if (c >= A) c -= A, ++r;
      }
    }
  }
}

// the statistics from the groups' sums and the weights' sums
LSM_HD void finish(const Loss& n, const double* sums, const double* header) {
  if (n.actor) {
    n.io.stats[0] = (float)(-sums[0] / header[0]);
    n.io.stats[2] = (float)(sums[1] / header[0]);
    n.io.stats[3] = (float)(sums[2] / (double)n.M);
  }
  if (n.critic) n.io.stats[1] = (float)(sums[3] / header[1]);
}

// threads 0 .. 3 add the tile's lanes in order and write the group's four sums
__device__ void group_sums(const double* P, int rows, double* dst) {
  __syncthreads();
  if (threadIdx.x < 4) {
    double acc = 0.0;
#pragma unroll 16
    for (int r = 0; r < rows; ++r) acc += P[threadIdx.x * GROUP + r];
    dst[threadIdx.x] = acc;
  }
}

// One workgroup: quantity k of every group (src[8 g + k], k < 4) added by thread k, g ascending, 256 groups
// staged through P at a time (coalesced; the next 256 are read into registers while these are added, so one
// global-memory latency is paid, not one per stage). out[0 .. 4) is valid in every thread after the call.
__device__ void add_groups(const double* src, int64_t groups, double* P, double* out) {
  const int t = threadIdx.x;
  double acc = 0.0, nxt[4];
  auto fetch = [&](int64_t g0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = t + k * BLOCK;   // element i of the stage: group g0 + i / 4, quantity i % 4
      nxt[k] = g0 + (i >> 2) < groups ? src[(g0 + (i >> 2)) * PER_GROUP + (i & 3)] : 0.0;
    }
  };
  fetch(0);
  for (int64_t g0 = 0; g0 < groups; g0 += GROUP) {
    const int cnt = groups - g0 < GROUP ? (int)(groups - g0) : GROUP;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = t + k * BLOCK;
      P[(i & 3) * GROUP + (i >> 2)] = nxt[k];
    }
    __syncthreads();
    if (g0 + GROUP < groups) fetch(g0 + GROUP);
    if (t < 4) {
#pragma unroll 16
      for (int g = 0; g < cnt; ++g) acc += P[t * GROUP + g];
    }
    __syncthreads();
  }
  if (t < 4) P[t] = acc;
  __syncthreads();
  for (int k = 0; k < 4; ++k) out[k] = P[k];
}

__global__ __launch_bounds__(BLOCK) void pre_kernel(Loss n) {
  __shared__ double P[4 * GROUP];
  const int64_t m0 = (int64_t)blockIdx.x * GROUP;
  const int64_t left = n.M - m0;
  const int rows = left < GROUP ? (int)left : GROUP;
  double q[4] = {0.0, 0.0, 0.0, 0.0};
  if ((int)threadIdx.x < rows) pre_row(n, m0 + threadIdx.x, q);
  for (int k = 0; k < 4; ++k) P[k * GROUP + threadIdx.x] = q[k];
  group_sums(P, rows, reinterpret_cast<double*>(n.io.scratch) + HEADER + (int64_t)blockIdx.x * PER_GROUP);
}

__global__ __launch_bounds__(BLOCK) void norm_kernel(Loss n) {
  __shared__ double P[4 * GROUP];
  double* sc = reinterpret_cast<double*>(n.io.scratch);
  double sums[4];
  add_groups(sc + HEADER, n.groups, P, sums);
  if (threadIdx.x == 0) normalise(n, sums, sc);
}

__global__ __launch_bounds__(BLOCK) void rows_kernel(Loss n) {
  extern __shared__ double lds8[];
  double* P = lds8;                                     // [4][GROUP]
  float* L = reinterpret_cast<float*>(lds8 + 4 * GROUP);   // [GROUP][S]
  const int64_t m0 = (int64_t)blockIdx.x * GROUP;
  const int64_t left = n.M - m0;
  const int rows = left < GROUP ? (int)left : GROUP;
  loss_tile(n, m0, rows, (int)threadIdx.x, GROUP, L, P);
  group_sums(P, rows, reinterpret_cast<double*>(n.io.scratch) + HEADER + (int64_t)blockIdx.x * PER_GROUP + 4);
}

__global__ __launch_bounds__(BLOCK) void finish_kernel(Loss n) {
  __shared__ double P[4 * GROUP];
  const double* sc = reinterpret_cast<const double*>(n.io.scratch);
  double sums[4];
  add_groups(sc + HEADER + 4, n.groups, P, sums);
  if (threadIdx.x == 0) finish(n, sums, sc);
}

thread_local char g_err[512] = "";

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "loss: %s", msg);
  return 1;
}

int64_t groups_of(int64_t M) { return (M + GROUP - 1) / GROUP; }

size_t rows_lds_bytes(const Loss& n) { return 4 * GROUP * sizeof(double) + (((size_t)GROUP * n.S * 4 + 7) & ~(size_t)7); }

struct Range {
  const void* p;
  size_t bytes;
  bool out;
};

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_loss(const lsm_loss_config& c, const lsm_loss_io* io, int64_t M, Loss* n) {
  if (!io) return fail("io is null");
  if (!in_range(c.num_actions, 1, MAX_ACTIONS)) return fail("num_actions must be in [1, 64]");
  if (!(c.clip_param >= 0.0f) || !std::isfinite(c.clip_param)) return fail("clip_param must be finite and >= 0");
  if (!(c.huber_delta >= 0.0f) || !std::isfinite(c.huber_delta)) return fail("huber_delta must be finite and >= 0");
  if (!(c.vn_beta >= 0.0) || !std::isfinite(c.vn_beta)) return fail("vn_beta must be finite and >= 0");
  if (M < 0) return fail("M < 0");
  const int A = c.num_actions;
  if (M > INT32_MAX / (int64_t)A) return fail("M * num_actions exceeds INT32_MAX; split the minibatch");
  lsm_loss_io f = *io;
  const bool actor = f.logits != nullptr, critic = f.values != nullptr;
  if (!actor && !critic) return fail("logits and values are both null: nothing to do");
  if (!f.stats) return fail("stats is null");
  if (!f.scratch) return fail("scratch is null");
  // the fields a skipped half would use are dropped first: they are not checked either
  if (!actor) f.actions = f.available_actions = f.old_log_probs = f.advantages = nullptr, f.dlogits = f.imp_weights = nullptr, f.bad = nullptr;
  if (!critic) f.value_preds = f.returns = nullptr, f.dvalues = nullptr;
  const bool vn = critic && c.use_valuenorm != 0;
  if (!vn) f.vn_state = f.denorm = nullptr;
  const bool pmask = actor && c.use_policy_active_masks != 0, vmask = critic && c.use_value_active_masks != 0;
  if (!pmask && !vmask) f.active_masks = nullptr;
  if (actor && (!f.actions || !f.old_log_probs || !f.advantages)) return fail("the actor half needs actions, old_log_probs and advantages");
  if (actor && !f.dlogits) return fail("the actor half needs dlogits");
  if (critic && (!f.value_preds || !f.returns)) return fail("the critic half needs value_preds and returns");
  if (critic && !f.dvalues) return fail("the critic half needs dvalues");
  if ((pmask || vmask) && !f.active_masks) return fail("an active-mask flag is set and active_masks is null");
  if (vn && !f.vn_state) return fail("use_valuenorm needs vn_state");
  const size_t m4 = (size_t)M * 4, ma4 = m4 * A;
  const size_t sb = (size_t)(HEADER + PER_GROUP * (groups_of(M) < 1 ? 1 : groups_of(M))) * sizeof(double);
  const Range rg[] = {{f.logits, ma4, false},      {f.actions, m4, false},      {f.available_actions, ma4, false},
                      {f.old_log_probs, m4, false}, {f.advantages, m4, false},   {f.active_masks, m4, false},
                      {f.values, m4, false},        {f.value_preds, m4, false},  {f.returns, m4, false},
                      {f.vn_state, 12, true},       {f.denorm, 8, true},         {f.dlogits, ma4, true},
                      {f.dvalues, m4, true},        {f.imp_weights, m4, true},   {f.stats, 16, true},
                      {f.scratch, sb, true},        {f.bad, 8, true}};
  constexpr int NR = sizeof rg / sizeof rg[0];
  for (int i = 0; i < NR; ++i) {
    const bool wide = i >= NR - 2;   // scratch and bad
    if ((uintptr_t)rg[i].p & (wide ? 7 : 3)) return fail(wide ? "misaligned pointer (scratch and bad: 8 bytes)" : "misaligned pointer");
  }
  for (int i = 0; i < NR; ++i) {
    if (!rg[i].out || !rg[i].p || !rg[i].bytes) continue;
    for (int j = 0; j < NR; ++j) {
      if (j == i || !rg[j].p || !rg[j].bytes || (rg[j].out && j < i)) continue;
      const uintptr_t x = (uintptr_t)rg[i].p, y = (uintptr_t)rg[j].p;
      if (x < y + rg[j].bytes && y < x + rg[i].bytes)
        return fail(rg[j].out ? "two outputs overlap" : "an output overlaps an input");
    }
  }
  n->c = c;
  n->io = f;
  n->M = M;
  n->groups = groups_of(M);
  n->A = A;
  n->S = A | 1;
  n->actor = actor, n->critic = critic, n->pmask = pmask, n->vmask = vmask, n->vn = vn;
  n->lo = (float)(1.0 - (double)c.clip_param);
  n->hi = (float)(1.0 + (double)c.clip_param);
  n->wb = (float)c.vn_beta;
  n->om = (float)(1.0 - c.vn_beta);
  return 0;
}

}  // namespace

extern "C" {

const char* lsm_loss_last_error(void) { return g_err; }

size_t lsm_ppo_loss_scratch_bytes(int64_t M) {
  if (M < 0) return 0;
  const int64_t g = groups_of(M);
  return (size_t)(HEADER + PER_GROUP * (g < 1 ? 1 : g)) * sizeof(double);
}

int lsm_ppo_loss(lsm_loss_config cfg, const lsm_loss_io* io, int64_t M, void* hip_stream) {
  Loss n;
  if (make_loss(cfg, io, M, &n)) return 1;
  if (M == 0) return 0;
  static std::atomic<bool> raised[MAX_DEVICES];   // the rows kernel's, to what A = 64 needs
  if (const char* why = raise_lds_once(raised, (const void*)rows_kernel, MAX_LDS_BYTES,
                                       "could not reserve the rows kernel's LDS"))
    return fail(why);
  const hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid((unsigned)n.groups), block(BLOCK);
  pre_kernel<<<grid, block, 0, st>>>(n);
  norm_kernel<<<1, block, 0, st>>>(n);
  rows_kernel<<<grid, block, rows_lds_bytes(n), st>>>(n);
  finish_kernel<<<1, block, 0, st>>>(n);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  return 0;
}

int lsm_host_ppo_loss(lsm_loss_config cfg, const lsm_loss_io* io, int64_t M) {
  Loss n;
  if (make_loss(cfg, io, M, &n)) return 1;
  if (M == 0) return 0;
  double* sc = reinterpret_cast<double*>(n.io.scratch);
  for (int64_t g = 0; g < n.groups; ++g) {   // pre_kernel: the group's rows in order
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t m = g * GROUP; m < M && m < (g + 1) * GROUP; ++m) {
      double q[4];
      pre_row(n, m, q);
      for (int k = 0; k < 4; ++k) acc[k] += q[k];
    }
    for (int k = 0; k < 4; ++k) sc[HEADER + g * PER_GROUP + k] = acc[k];
  }
  double sums[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t g = 0; g < n.groups; ++g)   // norm_kernel: the groups in order
    for (int k = 0; k < 4; ++k) sums[k] += sc[HEADER + g * PER_GROUP + k];
  normalise(n, sums, sc);
  std::vector<float> L(n.S);
  for (int64_t g = 0; g < n.groups; ++g) {   // rows_kernel
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t m = g * GROUP; m < M && m < (g + 1) * GROUP; ++m) {
      double P[4];
      loss_tile(n, m, 1, 0, 1, L.data(), P);
      for (int k = 0; k < 4; ++k) acc[k] += P[k];
    }
    for (int k = 0; k < 4; ++k) sc[HEADER + g * PER_GROUP + 4 + k] = acc[k];
  }
  for (int k = 0; k < 4; ++k) sums[k] = 0.0;
  for (int64_t g = 0; g < n.groups; ++g)   // finish_kernel
    for (int k = 0; k < 4; ++k) sums[k] += sc[HEADER + g * PER_GROUP + 4 + k];
  finish(n, sums, sc);
  return 0;
}

}  // extern "C"
