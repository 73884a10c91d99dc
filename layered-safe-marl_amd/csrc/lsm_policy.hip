// lsm_policy.hip -- the actor and critic heads in one launch (include/lsm_policy.h).
//
// Reference: GR_Actor.forward / GR_Critic.forward after gnn_base (graph_actor_critic.py:162-172, 406-418):
// torch.cat, MLPBase (feature norm, fc1, fc2[i], a LayerNorm behind each), RNNLayer's one-step GRU with its
// norm, then ACTLayer's Categorical (mask, softmax, sample or mode, log-probability) or v_out: about two
// dozen small launches per network, nn.GRU and torch.multinomial among them. Here a row never leaves
// its workgroup: the two input blocks are read once into one LDS row, every activation lives in LDS, and
// only the outputs are written.
//
// Work split. A 256-thread workgroup owns a tile of 64 rows, lane = row; its four waves split each
// layer's output columns in blocks of four (wave w: blocks w, w + 4, ..). For one block a lane reads its
// row from LDS 16 bytes at a time and runs 16 FMAs per read, the weights lane-uniform through the scalar
// cache (four weight rows, scalar operands of the FMAs). Each Linear writes its activated outputs to the
// other activation buffer; after a barrier every thread computes its row's LayerNorm statistics (the
// same order in every wave, so the four waves hold the same bits) and writes its own columns back to the
// first buffer; one more barrier. A GRU layer stages h = state * mask of the tile into LDS, then runs six
// dot products per hidden unit (W_i{r,z,n} x, W_h{r,z,n} h) and the gate arithmetic in the owning lane;
// h' goes to LDS and, after the layer's barrier, from there to rnn_out, consecutive threads writing
// consecutive floats (as features is written). The weight blob is a __restrict__ kernel argument of its
// own, so these stores do not keep the later layers' weight loads off the scalar cache. The
// actor's logits go through LDS to wave 0, whose lane walks its row's num_actions entries in ascending
// order three times (max; sum; running sum against u * s). Every sum runs in one lane in a fixed order (four
// partial sums over the inputs i mod 4, each ascending, see dot4): no atomics, no cross-lane reduction,
// bit-reproducible.
//
// LDS (floats per tile row): the input row pad(max(in, Hd)) (h lives there during the GRU) and two
// activation rows pad(max(Hd, A)), pad(w) = round_up(w, 4) + 4: 16-byte aligned rows whose stride is not a
// multiple of 64 banks (lane r's row starts 4 (r mod 16) banks on for width 64).
//
// tile_forward is ONE __host__ __device__ text; lsm_host_head_forward runs it with a tile of one row and
// one "wave".
#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_policy.h"

namespace {

#define LSM_HD __host__ __device__ __forceinline__
#if defined(__HIP_DEVICE_COMPILE__)
#define LSM_SYNC() __syncthreads()
#else
#define LSM_SYNC() ((void)0)
#endif

constexpr int BLOCK = 256;
constexpr int TILE = 64;            // rows per workgroup, lane = row
constexpr int WAVES = BLOCK / TILE;
constexpr int MAX_IN = 256, MAX_HIDDEN = 128, MAX_LAYERS = 4, MAX_RNN = 2, MAX_ACTIONS = 64;
constexpr int MAX_DEVICES = 64;

struct Head {
  const float* w;
  lsm_head_io io;
  int64_t M;
  int32_t in0, in1, in, Hd, L, relu, fnorm, RN, kind, A;
  int32_t SX, SA;          // padded LDS row strides: the input row, an activation row
  int32_t o_fn, o_fc[MAX_LAYERS + 1], o_gru[MAX_RNN], o_rn, o_out;
};

LSM_HD float fma_(float a, float b, float c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_fmaf(a, b, c);
#else
  return a * b + c;
#endif
}

LSM_HD float rsq_(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return rsqrtf(v);
#else
  return 1.0f / sqrtf(v);
#endif
}

LSM_HD float sigmoid_(float v) { return 1.0f / (1.0f + expf(-v)); }

// acc[jj] += <w[jj * ld + 0 .. n), row[0 .. n)> for jj < nj <= 4 (the other accumulators follow row 0 and
// are dropped by the caller); row is a 16-byte aligned LDS row. Each product sum runs as four partial sums
// over the inputs i mod 4 (inputs ascending, the first one starting from acc[jj]), added as (p0 + p1) +
// (p2 + p3), then the n mod 4 last inputs in turn: a fixed order with a quarter of the sequential sum's
// rounding growth, and sixteen independent FMA chains per 16-byte read
LSM_HD void dot4(const float* __restrict__ w, int ld, int nj, const float* row, int n, float (&acc)[4]) {
  const float* __restrict__ w0 = w;
  const float* __restrict__ w1 = w + (nj > 1 ? ld : 0);
  const float* __restrict__ w2 = w + (nj > 2 ? 2 * ld : 0);
  const float* __restrict__ w3 = w + (nj > 3 ? 3 * ld : 0);
  float p0[4] = {acc[0], 0.0f, 0.0f, 0.0f}, p1[4] = {acc[1], 0.0f, 0.0f, 0.0f};
  float p2[4] = {acc[2], 0.0f, 0.0f, 0.0f}, p3[4] = {acc[3], 0.0f, 0.0f, 0.0f};
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    const float4 h = *reinterpret_cast<const float4*>(row + i);
    p0[0] = fma_(w0[i], h.x, p0[0]);
    p1[0] = fma_(w1[i], h.x, p1[0]);
    p2[0] = fma_(w2[i], h.x, p2[0]);
    p3[0] = fma_(w3[i], h.x, p3[0]);
    p0[1] = fma_(w0[i + 1], h.y, p0[1]);
    p1[1] = fma_(w1[i + 1], h.y, p1[1]);
    p2[1] = fma_(w2[i + 1], h.y, p2[1]);
    p3[1] = fma_(w3[i + 1], h.y, p3[1]);
    p0[2] = fma_(w0[i + 2], h.z, p0[2]);
    p1[2] = fma_(w1[i + 2], h.z, p1[2]);
    p2[2] = fma_(w2[i + 2], h.z, p2[2]);
    p3[2] = fma_(w3[i + 2], h.z, p3[2]);
    p0[3] = fma_(w0[i + 3], h.w, p0[3]);
    p1[3] = fma_(w1[i + 3], h.w, p1[3]);
    p2[3] = fma_(w2[i + 3], h.w, p2[3]);
    p3[3] = fma_(w3[i + 3], h.w, p3[3]);
  }
  acc[0] = (p0[0] + p0[1]) + (p0[2] + p0[3]);
  acc[1] = (p1[0] + p1[1]) + (p1[2] + p1[3]);
  acc[2] = (p2[0] + p2[1]) + (p2[2] + p2[3]);
  acc[3] = (p3[0] + p3[1]) + (p3[2] + p3[3]);
  for (; i < n; ++i) {
    const float h = row[i];
    acc[0] = fma_(w0[i], h, acc[0]);
    acc[1] = fma_(w1[i], h, acc[1]);
    acc[2] = fma_(w2[i], h, acc[2]);
    acc[3] = fma_(w3[i], h, acc[3]);
  }
}

// the four accumulators of output block j0 start from the bias
LSM_HD void bias4(const float* __restrict__ b, int nj, float (&acc)[4]) {
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) acc[jj] = b[jj < nj ? jj : 0];
}

// dst[0 .. nout) = act(W src + b) for this wave's column blocks. act: 0 none, 1 ReLU (NaN stays NaN), 2 Tanh
LSM_HD void linear(const float* __restrict__ W, const float* __restrict__ b, int nout, int nin, const float* src,
                   float* dst, int wv, int nw, int act) {
  for (int j0 = 4 * wv; j0 < nout; j0 += 4 * nw) {
    const int nj = nout - j0 < 4 ? nout - j0 : 4;
    float acc[4];
    bias4(b + j0, nj, acc);
    dot4(W + (int64_t)j0 * nin, nin, nj, src, nin, acc);
    if (act == 1) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[jj] = acc[jj] < 0.0f ? 0.0f : acc[jj];
    } else if (act == 2) {
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[jj] = tanhf(acc[jj]);
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      if (jj < nj) dst[j0 + jj] = acc[jj];
  }
}

// the sum of f(row[i]) over i < n as four partial sums over i mod 4, (p0 + p1) + (p2 + p3), then the
// n mod 4 last ones in turn; f(v) = v - sub, squared when sq
LSM_HD float row_sum(const float* row, int n, float sub, bool sq) {
  float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    const float4 h = *reinterpret_cast<const float4*>(row + i);
    const float d[4] = {h.x - sub, h.y - sub, h.z - sub, h.w - sub};
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = sq ? fma_(d[k], d[k], p[k]) : p[k] + d[k];
  }
  float s = (p[0] + p[1]) + (p[2] + p[3]);
  for (; i < n; ++i) {
    const float d = row[i] - sub;
    s = sq ? fma_(d, d, s) : s + d;
  }
  return s;
}

// nn.LayerNorm(n) of src's row into dst's row: the statistics over the whole row in every wave (the same
// order in each, so the waves hold the same bits), the wave's own column blocks written. src == dst needs
// the barrier between the two halves.
LSM_HD void layer_norm(const float* src, float* dst, int n, const float* __restrict__ gamma,
                       const float* __restrict__ beta, int wv, int nw) {
  const float mean = row_sum(src, n, 0.0f, false) / (float)n;
  const float rs = rsq_(row_sum(src, n, mean, true) / (float)n + 1e-5f);
  if (src == dst) LSM_SYNC();
  for (int j0 = 4 * wv; j0 < n; j0 += 4 * nw)
    for (int j = j0; j < n && j < j0 + 4; ++j) dst[j] = fma_((src[j] - mean) * rs, gamma[j], beta[j]);
}

// One tile: rows row0 .. row0 + rows - 1, lane = row (lane >= rows: an idle lane that keeps the barriers
// uniform and writes nothing), wave wv of nw; R = the tile's capacity in rows (64 on the device, 1 on the host).
// w is the weight blob as a parameter of its own: as a __restrict__ kernel argument it is known not to alias
// the outputs, so the stores between the layers do not stop its loads from going through the scalar cache.
LSM_HD void tile_forward(const Head& n, const float* __restrict__ w, int64_t row0, int rows, int lane, int wv, int nw,
                         int R, float* lds) {
  const int tid = wv * R + lane, nt = nw * R;
  const int in = n.in, Hd = n.Hd, SX = n.SX, SA = n.SA, RN = n.RN;
  float* X = lds;
  float* cur = X + R * SX;
  float* nxt = cur + R * SA;
  const bool active = lane < rows;
  const int64_t m = row0 + lane;
  float* xrow = X + lane * SX;

  // ---- the virtual cat([x0, x1]): one LDS row per tile row, read coalesced --------------------------
  for (int k = tid; k < rows * n.in0; k += nt) {
    const int r = k / n.in0, c = k - r * n.in0;
    X[r * SX + c] = n.io.x0[row0 * n.in0 + k];
  }
  for (int k = tid; k < rows * n.in1; k += nt) {
    const int r = k / n.in1, c = k - r * n.in1;
    X[r * SX + n.in0 + c] = n.io.x1[row0 * n.in1 + k];
  }
  LSM_SYNC();
  if (n.fnorm) {
    layer_norm(xrow, xrow, in, w + n.o_fn, w + n.o_fn + in, wv, nw);
    LSM_SYNC();
  }

  // ---- MLPLayer: fc1, fc2[i]; each Linear, activation, LayerNorm ---------------------------------------
  for (int k = 0; k <= n.L; ++k) {
    const int din = k == 0 ? in : Hd;
    const float* W = w + n.o_fc[k];
    const float* b = W + Hd * din;
    linear(W, b, Hd, din, k == 0 ? xrow : cur + lane * SA, nxt + lane * SA, wv, nw, n.relu ? 1 : 2);
    LSM_SYNC();
    layer_norm(nxt + lane * SA, cur + lane * SA, Hd, b + Hd, b + 2 * Hd, wv, nw);
    LSM_SYNC();
  }

  // ---- RNNLayer: recurrent_N GRU cells on h = state * mask, then its norm --------------------------------
  for (int l = 0; l < RN; ++l) {
    for (int k = tid; k < rows * Hd; k += nt) {
      const int r = k / Hd, c = k - r * Hd;
      X[r * SX + c] = n.io.rnn_states[((row0 + r) * RN + l) * Hd + c] * n.io.masks[row0 + r];
    }
    LSM_SYNC();
    const float* Wih = w + n.o_gru[l];
    const float* Whh = Wih + 3 * Hd * Hd;
    const float* bih = Whh + 3 * Hd * Hd;
    const float* bhh = bih + 3 * Hd;
    const float* x = cur + lane * SA;
    float* o = nxt + lane * SA;
    for (int j0 = 4 * wv; j0 < Hd; j0 += 4 * nw) {
      const int nj = Hd - j0 < 4 ? Hd - j0 : 4;
      float ir[4], iz[4], ig[4], hr[4], hz[4], hg[4];
      bias4(bih + j0, nj, ir);
      bias4(bih + Hd + j0, nj, iz);
      bias4(bih + 2 * Hd + j0, nj, ig);
      bias4(bhh + j0, nj, hr);
      bias4(bhh + Hd + j0, nj, hz);
      bias4(bhh + 2 * Hd + j0, nj, hg);
      dot4(Wih + j0 * Hd, Hd, nj, x, Hd, ir);
      dot4(Wih + (Hd + j0) * Hd, Hd, nj, x, Hd, iz);
      dot4(Wih + (2 * Hd + j0) * Hd, Hd, nj, x, Hd, ig);
      dot4(Whh + j0 * Hd, Hd, nj, xrow, Hd, hr);
      dot4(Whh + (Hd + j0) * Hd, Hd, nj, xrow, Hd, hz);
      dot4(Whh + (2 * Hd + j0) * Hd, Hd, nj, xrow, Hd, hg);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        if (jj >= nj) continue;
        const float r = sigmoid_(ir[jj] + hr[jj]);
        const float z = sigmoid_(iz[jj] + hz[jj]);
        const float g = tanhf(fma_(r, hg[jj], ig[jj]));
        const float hp = fma_(z, xrow[j0 + jj], (1.0f - z) * g);
        o[j0 + jj] = hp;
      }
    }
    LSM_SYNC();
    float* t = cur;
    cur = nxt;
    nxt = t;
    // h'_l of the tile, from LDS: consecutive threads write consecutive floats of a row
    if (n.io.rnn_out)
      for (int k = tid; k < rows * Hd; k += nt) {
        const int r = k / Hd, c = k - r * Hd;
        n.io.rnn_out[((row0 + r) * RN + l) * Hd + c] = cur[r * SA + c];
      }
  }
  if (RN > 0) {
    layer_norm(cur + lane * SA, nxt + lane * SA, Hd, w + n.o_rn, w + n.o_rn + Hd, wv, nw);
    LSM_SYNC();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }
  if (n.io.features)
    for (int k = tid; k < rows * Hd; k += nt) {
      const int r = k / Hd, c = k - r * Hd;
      n.io.features[row0 * Hd + k] = cur[r * SA + c];
    }

  // ---- the output layer -------------------------------------------------------------------------------------
  const float* Wo = w + n.o_out;
  const float* feat = cur + lane * SA;
  if (n.kind == LSM_HEAD_CRITIC) {
    if (wv == 0 && active && n.io.values) {
      float v = Wo[Hd];
      for (int i = 0; i < Hd; ++i) v = fma_(Wo[i], feat[i], v);
      n.io.values[m] = v;
    }
    return;
  }
  const int A = n.A;
  float* lg = nxt + lane * SA;
  linear(Wo, Wo + A * Hd, A, Hd, feat, lg, wv, nw, 0);
  LSM_SYNC();
  if (wv != 0 || !active) return;
  float mx = 0.0f;
  int first = 0;
  for (int a = 0; a < A; ++a) {
    float l = lg[a];
    if (n.io.available_actions && n.io.available_actions[m * A + a] == 0.0f) l = -FLT_MAX;
    lg[a] = l;
    if (n.io.logits) n.io.logits[m * A + a] = l;
    if (a == 0 || l > mx) mx = l, first = a;
  }
  float s = 0.0f;
  for (int a = 0; a < A; ++a) s += expf(lg[a] - mx);
  int pick = first;
  if (n.io.u) {
    float u = n.io.u[m];
    if (!(u >= 0.0f && u < 1.0f)) {
      if (n.io.bad) *n.io.bad = 1;
      u = u >= 1.0f ? 0.99999994f : 0.0f;   // NaN and negatives: 0
    }
    const float t = u * s;
    float run = 0.0f;
    int last = -1;
    pick = -1;
    for (int a = 0; a < A; ++a) {
      const float e = expf(lg[a] - mx);
      run += e;
      if (e > 0.0f) last = a;
      if (pick < 0 && run > t) pick = a;
    }
    if (pick < 0) pick = last < 0 ? 0 : last;
  }
  if (n.io.actions_i32) n.io.actions_i32[m] = pick;
  if (n.io.actions_f32) n.io.actions_f32[m] = (float)pick;
  if (n.io.log_probs) n.io.log_probs[m] = (lg[pick] - mx) - logf(s);
}

__global__ __launch_bounds__(BLOCK) void head_kernel(Head n, const float* __restrict__ w) {
  extern __shared__ float4 lds4[];
  const int64_t row0 = (int64_t)blockIdx.x * TILE;
  const int64_t left = n.M - row0;
  // the wave's index as a scalar: the weight addresses derived from it are then lane-uniform to the compiler
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / TILE);
  tile_forward(n, w, row0, left < TILE ? (int)left : TILE, (int)threadIdx.x & (TILE - 1), wv, WAVES, TILE,
               reinterpret_cast<float*>(lds4));
}

thread_local char g_err[256];

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "head: %s", msg);
  return 1;
}

constexpr int pad(int w) { return ((w + 3) & ~3) + 4; }

// the largest tile the limits allow (in = 256, hidden = 128): 134144 bytes, within one workgroup's 160 KB
constexpr int MAX_TILE_BYTES = TILE * (pad(MAX_IN) + 2 * pad(MAX_HIDDEN)) * (int)sizeof(float);
static_assert(MAX_TILE_BYTES <= 163840, "the worst-case tile must fit one workgroup's LDS");

bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

// the config's checks and the blob's offsets; returns the blob's length in floats, 0 with a text on refusal
size_t layout(const lsm_head_config& c, Head* n) {
  if (c.in0 < 0 || c.in1 < 0) return fail("in0 and in1 must be >= 0"), 0;
  if (c.in0 > MAX_IN || c.in1 > MAX_IN || !in_range(c.in0 + c.in1, 1, MAX_IN))
    return fail("in0 + in1 must be in [1, 256]"), 0;
  if (!in_range(c.hidden, 1, MAX_HIDDEN)) return fail("hidden must be in [1, 128]"), 0;
  if (!in_range(c.layer_N, 0, MAX_LAYERS)) return fail("layer_N must be in [0, 4]"), 0;
  if (!in_range(c.recurrent_N, 0, MAX_RNN)) return fail("recurrent_N must be in [0, 2]"), 0;
  if (c.kind != LSM_HEAD_ACTOR && c.kind != LSM_HEAD_CRITIC) return fail("unknown kind"), 0;
  if (c.kind == LSM_HEAD_ACTOR && !in_range(c.num_actions, 1, MAX_ACTIONS))
    return fail("num_actions must be in [1, 64]"), 0;
  n->in0 = c.in0;
  n->in1 = c.in1;
  n->in = c.in0 + c.in1;
  n->Hd = c.hidden;
  n->L = c.layer_N;
  n->relu = c.relu != 0;
  n->fnorm = c.feature_norm != 0;
  n->RN = c.recurrent_N;
  n->kind = c.kind;
  n->A = c.kind == LSM_HEAD_ACTOR ? c.num_actions : 1;
  const int Hd = n->Hd;
  int o = 0;
  n->o_fn = o, o += 2 * n->in;
  for (int k = 0; k <= MAX_LAYERS; ++k) {
    n->o_fc[k] = o;
    if (k <= n->L) o += Hd * (k == 0 ? n->in : Hd) + 3 * Hd;
  }
  for (int l = 0; l < MAX_RNN; ++l) {
    n->o_gru[l] = o;
    if (l < n->RN) o += 6 * Hd * Hd + 6 * Hd;
  }
  n->o_rn = o;
  if (n->RN > 0) o += 2 * Hd;
  n->o_out = o, o += n->A * Hd + n->A;
  n->SX = pad(n->in > Hd ? n->in : Hd);
  n->SA = pad(Hd > n->A ? Hd : n->A);
  return (size_t)o;
}

bool overlap(const void* a, const void* b, size_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + bytes && y < x + bytes;
}

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_head(const lsm_head_config& c, const float* weights, const lsm_head_io* io, int64_t M, Head* n) {
  if (layout(c, n) == 0) return 1;
  if (!weights) return fail("weights is null");
  if (!io) return fail("io is null");
  if (M < 0) return fail("M < 0");
  if (M > INT32_MAX) return fail("M exceeds INT32_MAX rows; split the batch");
  // the fields this config does not read or write are dropped first: they are not checked either
  lsm_head_io f = *io;
  if (n->in0 == 0) f.x0 = nullptr;
  if (n->in1 == 0) f.x1 = nullptr;
  if (n->RN == 0) f.rnn_states = f.masks = nullptr, f.rnn_out = nullptr;
  if (n->kind == LSM_HEAD_ACTOR) {
    f.values = nullptr;
  } else {
    f.u = f.available_actions = nullptr;
    f.actions_i32 = nullptr;
    f.actions_f32 = f.log_probs = f.logits = nullptr;
  }
  if (M > 0 && ((n->in0 > 0 && !f.x0) || (n->in1 > 0 && !f.x1))) return fail("x0 / x1 is null");
  const void* p4[] = {weights, f.x0, f.x1, f.rnn_states, f.masks, f.u, f.available_actions, f.actions_i32,
                      f.actions_f32, f.log_probs, f.logits, f.values, f.features, f.rnn_out};
  for (const void* p : p4)
    if ((uintptr_t)p & 3) return fail("misaligned pointer");
  if ((uintptr_t)f.bad & 7) return fail("misaligned pointer");
  if (n->RN > 0) {
    if (M > 0 && (!f.rnn_states || !f.masks)) return fail("the recurrent form needs rnn_states and masks");
    if (f.rnn_out && M > 0 && overlap(f.rnn_out, f.rnn_states, (size_t)M * n->RN * n->Hd * sizeof(float)))
      return fail("rnn_out overlaps rnn_states");
  }
  if (n->kind == LSM_HEAD_ACTOR && !f.actions_i32 && !f.actions_f32)
    return fail("the actor needs actions_i32 or actions_f32");
  n->w = weights;
  n->io = f;
  n->M = M;
  return 0;
}

}  // namespace

extern "C" {

const char* lsm_policy_last_error(void) { return g_err; }

size_t lsm_head_weights_floats(lsm_head_config cfg) {
  Head n;
  return layout(cfg, &n);
}

int lsm_head_forward(lsm_head_config cfg, const float* weights, const lsm_head_io* io, int64_t M, void* hip_stream) {
  Head n;
  if (make_head(cfg, weights, io, M, &n)) return 1;
  if (M == 0) return 0;
  const size_t lds = (size_t)TILE * (n.SX + 2 * n.SA) * sizeof(float);
  if (lds > (size_t)MAX_TILE_BYTES) return fail("the tile exceeds the LDS of one workgroup");
  const dim3 grid((unsigned)((M + TILE - 1) / TILE)), block(BLOCK);
  // the kernel's dynamic-LDS limit is raised once per device, to the limits' worst case: the value never
  // depends on the call, so concurrent callers with different configs cannot lower it under one another
  static std::atomic<bool> raised[MAX_DEVICES];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return fail("no current device");
  if (!raised[dev].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute((const void*)head_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MAX_TILE_BYTES) !=
        hipSuccess)
      return fail("could not reserve the workgroup's LDS");
    raised[dev].store(true, std::memory_order_release);
  }
  head_kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(n, n.w);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_host_head_forward(lsm_head_config cfg, const float* weights, const lsm_head_io* io, int64_t M) {
  Head n;
  if (make_head(cfg, weights, io, M, &n)) return 1;
  std::vector<float4> scratch((size_t)(n.SX + 2 * n.SA) / 4 + 1);
  for (int64_t m = 0; m < M; ++m) tile_forward(n, n.w, m, 1, 0, 0, 1, 1, reinterpret_cast<float*>(scratch.data()));
  return 0;
}

}  // extern "C"
