// lsm_optim.hip -- the gradient norm, clip_grad_norm_'s coefficient and Adam's step on the packed weight blobs
// (include/lsm_optim.h): the last lines of each half of GR_MAPPO.ppo_update.
//
// Reference: torch.nn.utils.clip_grad_norm_, torch.optim.Adam (_single_tensor_adam without amsgrad),
// GradScaler.step's skip on a non-finite gradient, get_gard_norm (onpolicy/utils/util.py).
//
// The blobs are small (a head about 35k floats, an encoder about 8k at the reference's defaults), so a call is
// bound by its launches, not by its traffic: three of them, shared by every group of the call.
//   norm_kernel      one workgroup per chunk of LSM_OPT_CHUNK floats: lane j squares and adds elements j, j + 256,
//                    ... in float64 (dword loads, coalesced whatever the segment's alignment), the lanes' sums fold
//                    through LDS, the chunk's partial goes to the workspace
//   finalise_kernel  one workgroup per group: the group's partials ascending, then thread 0 runs finalise()
//   apply_kernel     one workgroup per chunk, four elements per thread. The segment's (weights, grads, exp_avg,
//                    exp_avg_sq) are 4-byte aligned only; where all four sit at the same offset from a 16-byte
//                    boundary the chunk is cut into a head of up to three floats, whole aligned float4 and a tail,
//                    and only the head and the tail go through scalar accesses.
// A block finds its (group, segment, chunk) by walking the table in the kernel arguments: block-uniform, scalar.
//
// chunk_lane_sum, fold, finalise and adam_element are ONE __host__ __device__ text; lsm_host_optim_step runs them
// in the kernels' order.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/lsm_optim.h"

#define LSM_HD __host__ __device__ __forceinline__

namespace {

constexpr int LANES = LSM_OPT_LANES;
constexpr int CHUNK = LSM_OPT_CHUNK;
constexpr int MAXG = LSM_OPT_MAX_GROUPS;
constexpr int MAXS = LSM_OPT_MAX_SEGMENTS;
constexpr int HEADER = 4 * MAXG;   // workspace doubles before the chunks' partials: 4 per group, see Step
static_assert(CHUNK == 4 * LANES, "apply_kernel: four elements per thread");

struct Seg {
  float* w;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  int64_t chunk0;   // the segment's first chunk, counted over the whole call
};

struct Grp {
  Seg seg[MAXS];
  int32_t nseg, use_max, skip_nonfinite;
  int64_t chunk0, nchunks;
  double lr, beta1, beta2;
  float b2f, omb1, omb2, epsf, wdf, maxf;
  double* state;
  float* info;
};

struct Table {
  Grp grp[MAXG];
  int32_t n_groups;
  int64_t chunks;
  double* ws;
};

// what finalise leaves for apply, in the group's 4 header doubles of the workspace (the first 16 bytes used)
struct Step {
  float clip_coef, step_size, s2;
  int32_t skipped;
};
static_assert(sizeof(Step) <= 4 * sizeof(double), "a group's header slot");

// lane j's float64 sum of the chunk's squares: elements j, j + LANES, ... ascending
LSM_HD double chunk_lane_sum(const float* g, int len, int j) {
  double q = 0.0;
  for (int i = j; i < len; i += LANES) {
    const double d = (double)g[i];
    q += d * d;
  }
  return q;
}

LSM_HD bool finite_(float x) { return fabsf(x) <= FLT_MAX; }

// by one thread, after the group's partials were added: info, state and the step's scalars
LSM_HD void finalise(const Grp& p, double sum, Step* out) {
  const float norm = (float)sqrt(sum);
  float coef = 1.0f;
  if (p.use_max) {
    const float c = p.maxf / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;
  }
  const bool skipped = p.skip_nonfinite && !finite_(norm);
  Step s = {coef, 0.0f, 1.0f, skipped ? 1 : 0};
  if (!skipped) {
    const double steps = p.state[0] + 1.0, p1 = p.state[1] * p.beta1, p2 = p.state[2] * p.beta2;
    p.state[0] = steps;
    p.state[1] = p1;
    p.state[2] = p2;
    s.step_size = (float)(p.lr / (1.0 - p1));
    s.s2 = (float)sqrt(1.0 - p2);
  }
  p.info[0] = norm;
  p.info[1] = coef;
  p.info[2] = skipped ? 1.0f : 0.0f;
  p.info[3] = 0.0f;
  *out = s;
}

LSM_HD void adam_element(const Grp& p, const Step& s, float grad, float& w, float& m, float& v) {
  float g = s.clip_coef * grad;
  if (p.wdf != 0.0f) g = g + p.wdf * w;
  m = m + p.omb1 * (g - m);
  v = v * p.b2f + (p.omb2 * g) * g;
  w = w - s.step_size * (m / (sqrtf(v) / s.s2 + p.epsf));
}

// block b's group, segment and chunk: the table in order
__device__ __forceinline__ const Seg& locate(const Table& t, int64_t b, int* gi, int64_t* k) {
  int g = 0;
  while (g + 1 < t.n_groups && b >= t.grp[g + 1].chunk0) ++g;
  const Grp& p = t.grp[g];
  int s = 0;
  // empty segments have no chunk: the last segment whose first chunk is <= b holds it
  for (int i = 1; i < p.nseg; ++i)
    if (b >= p.seg[i].chunk0) s = i;
  *gi = g;
  *k = b - p.seg[s].chunk0;
  return p.seg[s];
}

__global__ __launch_bounds__(LANES) void norm_kernel(Table t) {
  __shared__ double q[LANES];
  int gi;
  int64_t k;
  const Seg& sg = locate(t, blockIdx.x, &gi, &k);
  const int64_t left = sg.n - k * CHUNK;
  const int len = left < CHUNK ? (int)left : CHUNK;
  const int j = threadIdx.x;
  q[j] = chunk_lane_sum(sg.g + k * CHUNK, len, j);
  __syncthreads();
  for (int s = LANES / 2; s > 0; s >>= 1) {
    if (j < s) q[j] += q[j + s];
    __syncthreads();
  }
  if (j == 0) t.ws[HEADER + blockIdx.x] = q[0];
}

__global__ __launch_bounds__(LANES) void finalise_kernel(Table t) {
  __shared__ double stage[LANES];
  const Grp& p = t.grp[blockIdx.x];
  const double* part = t.ws + HEADER + p.chunk0;
  double sum = 0.0;
  for (int64_t c0 = 0; c0 < p.nchunks; c0 += LANES) {   // coalesced into LDS, then thread 0 adds them in order
    const int64_t left = p.nchunks - c0;
    const int cnt = left < LANES ? (int)left : LANES;
    if ((int)threadIdx.x < cnt) stage[threadIdx.x] = part[c0 + threadIdx.x];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < cnt; ++i) sum += stage[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) finalise(p, sum, reinterpret_cast<Step*>(t.ws + 4 * blockIdx.x));
}

__global__ __launch_bounds__(LANES) void apply_kernel(Table t) {
  int gi;
  int64_t k;
  const Seg& sg = locate(t, blockIdx.x, &gi, &k);
  const Grp& p = t.grp[gi];
  const Step s = *reinterpret_cast<const Step*>(t.ws + 4 * gi);
  if (s.skipped) return;
  const int64_t left = sg.n - k * CHUNK;
  const int len = left < CHUNK ? (int)left : CHUNK;
  float* w = sg.w + k * CHUNK;
  const float* g = sg.g + k * CHUNK;
  float* m = sg.m + k * CHUNK;
  float* v = sg.v + k * CHUNK;
  const int j = threadIdx.x;
  const uintptr_t off = (uintptr_t)w & 15;
  const bool same = ((uintptr_t)g & 15) == off && ((uintptr_t)m & 15) == off && ((uintptr_t)v & 15) == off;
  if (!same) {   // block-uniform
    for (int i = j; i < len; i += LANES) adam_element(p, s, g[i], w[i], m[i], v[i]);
    return;
  }
  int head = (int)((16 - off) & 15) / 4;   // floats before the first 16-byte boundary
  if (head > len) head = len;
  const int nvec = (len - head) / 4, tail0 = head + 4 * nvec;
  if (j < nvec) {
    const int i = head + 4 * j;
    float4 w4 = *reinterpret_cast<float4*>(w + i), m4 = *reinterpret_cast<float4*>(m + i);
    float4 v4 = *reinterpret_cast<float4*>(v + i);
    const float4 g4 = *reinterpret_cast<const float4*>(g + i);
    adam_element(p, s, g4.x, w4.x, m4.x, v4.x);
    adam_element(p, s, g4.y, w4.y, m4.y, v4.y);
    adam_element(p, s, g4.z, w4.z, m4.z, v4.z);
    adam_element(p, s, g4.w, w4.w, m4.w, v4.w);
    *reinterpret_cast<float4*>(w + i) = w4;
    *reinterpret_cast<float4*>(m + i) = m4;
    *reinterpret_cast<float4*>(v + i) = v4;
  }
  // the head [0, head) and the tail [tail0, len): at most 3 + 3 elements, one thread each
  const int extra = head + (len - tail0);
  if (j < extra) {
    const int i = j < head ? j : tail0 + (j - head);
    adam_element(p, s, g[i], w[i], m[i], v[i]);
  }
}

thread_local char g_err[512] = "";

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "optim: %s", msg);
  return 1;
}

bool good(double x) { return std::isfinite(x) && x >= 0.0; }

// the counts alone (what lsm_optim_workspace_bytes can answer for); *chunks: the call's chunks
int count_chunks(const lsm_optim_group* groups, int32_t n_groups, int64_t* chunks) {
  if (n_groups < 0 || n_groups > MAXG) return fail("n_groups must be in [0, LSM_OPT_MAX_GROUPS]");
  if (n_groups > 0 && !groups) return fail("the group table is null");
  int64_t total = 0;
  for (int gi = 0; gi < n_groups; ++gi) {
    const lsm_optim_group& G = groups[gi];
    if (G.n_segments < 0 || G.n_segments > MAXS) return fail("n_segments must be in [0, LSM_OPT_MAX_SEGMENTS]");
    for (int si = 0; si < G.n_segments; ++si) {
      const int64_t n = G.segments[si].n;
      if (n < 0) return fail("a segment has n < 0");
      if (n > (int64_t)INT32_MAX * CHUNK) return fail("more than INT32_MAX chunks in one call");
      total += (n + CHUNK - 1) / CHUNK;
      if (total > INT32_MAX) return fail("more than INT32_MAX chunks in one call");
    }
  }
  *chunks = total;
  return 0;
}

struct Range {
  uintptr_t p;
  size_t bytes;
};

// by differences: no sum of an address and a size that could wrap
bool overlap(const Range& a, const Range& b) { return a.p < b.p ? b.p - a.p < a.bytes : a.p - b.p < b.bytes; }

// every check of one call, shared by the device and the host entry point; fills t; 0 when fine
int make_table(const lsm_optim_group* groups, int32_t n_groups, void* workspace, Table* t) {
  int64_t chunks = 0;
  if (count_chunks(groups, n_groups, &chunks)) return 1;
  if (n_groups > 0 && !workspace) return fail("workspace is null");
  if ((uintptr_t)workspace & 7) return fail("misaligned pointer (state and workspace: 8 bytes)");
  static thread_local Range wr[MAXG * (3 * MAXS + 2) + 1], rd[MAXG * MAXS];
  int nw = 0, nr = 0;
  if (n_groups > 0) wr[nw++] = {(uintptr_t)workspace, (size_t)(HEADER + chunks) * sizeof(double)};
  t->n_groups = n_groups;
  t->chunks = chunks;
  t->ws = static_cast<double*>(workspace);
  int64_t c = 0;
  for (int gi = 0; gi < n_groups; ++gi) {
    const lsm_optim_group& G = groups[gi];
    Grp& p = t->grp[gi];
    if (!good(G.lr)) return fail("lr must be finite and >= 0");
    if (!good(G.eps)) return fail("eps must be finite and >= 0");
    if (!good(G.weight_decay)) return fail("weight_decay must be finite and >= 0");
    if (!good(G.max_grad_norm)) return fail("max_grad_norm must be finite and >= 0");
    if (!(G.beta1 >= 0.0 && G.beta1 < 1.0) || !(G.beta2 >= 0.0 && G.beta2 < 1.0)) return fail("the betas must be in [0, 1)");
    if (!G.state || !G.info) return fail("state or info is null");
    if ((uintptr_t)G.state & 7) return fail("misaligned pointer (state and workspace: 8 bytes)");
    if ((uintptr_t)G.info & 3) return fail("misaligned pointer");
    wr[nw++] = {(uintptr_t)G.state, 4 * sizeof(double)};
    wr[nw++] = {(uintptr_t)G.info, 4 * sizeof(float)};
    p.nseg = G.n_segments;
    p.use_max = G.use_max_grad_norm != 0;
    p.skip_nonfinite = G.skip_nonfinite != 0;
    p.chunk0 = c;
    p.lr = G.lr, p.beta1 = G.beta1, p.beta2 = G.beta2;
    p.b2f = (float)G.beta2;
    p.omb1 = (float)(1.0 - G.beta1);
    p.omb2 = (float)(1.0 - G.beta2);
    p.epsf = (float)G.eps, p.wdf = (float)G.weight_decay, p.maxf = (float)G.max_grad_norm;
    p.state = G.state, p.info = G.info;
    for (int si = 0; si < G.n_segments; ++si) {
      const lsm_optim_segment& S = G.segments[si];
      Seg& q = p.seg[si];
      q = Seg{S.weights, S.grads, S.exp_avg, S.exp_avg_sq, S.n, c};
      if (S.n == 0) {
        q = Seg{nullptr, nullptr, nullptr, nullptr, 0, c};
        continue;
      }
      if (!S.weights || !S.grads || !S.exp_avg || !S.exp_avg_sq) return fail("a segment with n > 0 has a null pointer");
      if (((uintptr_t)S.weights | (uintptr_t)S.grads | (uintptr_t)S.exp_avg | (uintptr_t)S.exp_avg_sq) & 3)
        return fail("misaligned pointer");
      const size_t bytes = (size_t)S.n * sizeof(float);
      wr[nw++] = {(uintptr_t)S.weights, bytes};
      wr[nw++] = {(uintptr_t)S.exp_avg, bytes};
      wr[nw++] = {(uintptr_t)S.exp_avg_sq, bytes};
      rd[nr++] = {(uintptr_t)S.grads, bytes};
      c += (S.n + CHUNK - 1) / CHUNK;
    }
    p.nchunks = c - p.chunk0;
  }
  for (int i = 0; i < nw; ++i) {
    for (int j = i + 1; j < nw; ++j)
      if (overlap(wr[i], wr[j])) return fail("two written ranges overlap");
    for (int j = 0; j < nr; ++j)
      if (overlap(wr[i], rd[j])) return fail("a written range overlaps grads");
  }
  return 0;
}

}  // namespace

extern "C" {

const char* lsm_optim_last_error(void) { return g_err; }

size_t lsm_optim_workspace_bytes(const lsm_optim_group* groups, int32_t n_groups) {
  int64_t chunks = 0;
  if (count_chunks(groups, n_groups, &chunks)) return 0;
  return (size_t)(HEADER + chunks) * sizeof(double);
}

int lsm_optim_step(const lsm_optim_group* groups, int32_t n_groups, void* workspace, void* hip_stream) {
  static thread_local Table t;
  if (make_table(groups, n_groups, workspace, &t)) return 1;
  if (n_groups == 0) return 0;
  const hipStream_t st = (hipStream_t)hip_stream;
  const dim3 block(LANES);
  if (t.chunks > 0) norm_kernel<<<dim3((unsigned)t.chunks), block, 0, st>>>(t);
  finalise_kernel<<<dim3((unsigned)n_groups), block, 0, st>>>(t);
  if (t.chunks > 0) apply_kernel<<<dim3((unsigned)t.chunks), block, 0, st>>>(t);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  return 0;
}

int lsm_host_optim_step(const lsm_optim_group* groups, int32_t n_groups, void* workspace) {
  static thread_local Table t;
  if (make_table(groups, n_groups, workspace, &t)) return 1;
  for (int gi = 0; gi < n_groups; ++gi) {   // norm_kernel: every chunk's lanes, then the fold
    const Grp& p = t.grp[gi];
    for (int si = 0; si < p.nseg; ++si) {
      const Seg& sg = p.seg[si];
      for (int64_t k = 0; k * CHUNK < sg.n; ++k) {
        const int64_t left = sg.n - k * CHUNK;
        const int len = left < CHUNK ? (int)left : CHUNK;
        double q[LANES];
        for (int j = 0; j < LANES; ++j) q[j] = chunk_lane_sum(sg.g + k * CHUNK, len, j);
        for (int s = LANES / 2; s > 0; s >>= 1)
          for (int j = 0; j < s; ++j) q[j] += q[j + s];
        t.ws[HEADER + sg.chunk0 + k] = q[0];
      }
    }
  }
  for (int gi = 0; gi < n_groups; ++gi) {   // finalise_kernel
    const Grp& p = t.grp[gi];
    double sum = 0.0;
    for (int64_t c = 0; c < p.nchunks; ++c) sum += t.ws[HEADER + p.chunk0 + c];
    finalise(p, sum, reinterpret_cast<Step*>(t.ws + 4 * gi));
  }
  for (int gi = 0; gi < n_groups; ++gi) {   // apply_kernel
    const Grp& p = t.grp[gi];
    const Step s = *reinterpret_cast<const Step*>(t.ws + 4 * gi);
    if (s.skipped) continue;
    for (int si = 0; si < p.nseg; ++si) {
      const Seg& sg = p.seg[si];
      for (int64_t i = 0; i < sg.n; ++i) adam_element(p, s, sg.g[i], sg.w[i], sg.m[i], sg.v[i]);
    }
  }
  return 0;
}

}  // extern "C"
