// lsm_head_tile.h -- what the three head units share (lsm_policy.hip: one step; lsm_evaluate.hip: the sequence
// form; lsm_backward.hip: the backward pass). Device side: the kernels' entry (block_tile), the tile-row
// copies (load_rows, save_rows), dot4 / linear / layer_norm, the input staging, MLPBase, one GRU layer's cells
// and the softmax walks. MLPBase and the GRU cells take a hook (NoSaves by default: nothing kept, nothing
// paid) through which stage 1 of the backward keeps what its sweep needs. Host side: the config's checks and
// the weight blob's offsets, the checks of a call that the units share (each unit keeps its own order of
// them) and launch(). Every device piece is ONE __host__ __device__ text: the host entry points run it with a
// tile of one row and one "wave".
//
// Work split and LDS layout are described in lsm_policy.hip; what a piece expects of the barriers around
// it stands at the piece.
#ifndef LSM_HEAD_TILE_H
#define LSM_HEAD_TILE_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../include/lsm_policy.h"

// the text of lsm_policy_last_error() (thread-local, lsm_policy.hip): "<prefix><msg>"
__attribute__((visibility("hidden"))) void lsm_policy_set_error(const char* prefix, const char* msg);

// lsm_head_plan's parts that lsm_evaluate.hip and lsm_backward.hip fill from their own launch code
__attribute__((visibility("hidden"))) int lsm_evaluate_fill_plan(const lsm_head_config& c, int64_t C, int32_t T,
                                                                 lsm_head_launch_plan* out);
__attribute__((visibility("hidden"))) int lsm_backward_fill_plan(const lsm_head_config& c, int64_t C, int32_t T,
                                                                 lsm_head_launch_plan* out);

namespace lsm_head_tile {

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
constexpr int WORKGROUP_LDS_BYTES = 163840;   // 160 KB: what one workgroup can have

// Raise kernel's dynamic-LDS limit to bytes, once per device (raised: the caller's own static flags, one set
// per kernel). bytes is the kernel's worst case and never depends on the call, so concurrent callers with
// different configs cannot lower it under one another. Returns nullptr, or the refusal's text.
inline const char* raise_lds_once(std::atomic<bool> (&raised)[MAX_DEVICES], const void* kernel, int bytes,
                                  const char* refused = "could not reserve the workgroup's LDS") {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) return "no current device";
  if (!raised[dev].load(std::memory_order_acquire)) {
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return refused;
    raised[dev].store(true, std::memory_order_release);
  }
  return nullptr;
}

// One launch on the stream: Kernel's dynamic-LDS limit raised to LdsLimit bytes first (raise_lds: once per
// device, the flags being that instantiation's own; 0: the kernel has no dynamic LDS), the launch, its check.
// Returns nullptr, or the refusal's text. A call of several kernels raises every limit before its first launch.
template <auto Kernel, int LdsLimit>
const char* raise_lds() {
  static std::atomic<bool> raised[MAX_DEVICES];
  return raise_lds_once(raised, (const void*)Kernel, LdsLimit);
}

template <auto Kernel, int LdsLimit = 0, class... Args>
const char* launch(dim3 grid, dim3 block, size_t lds, void* hip_stream, const Args&... args) {
  if constexpr (LdsLimit > 0)
    if (const char* why = raise_lds<Kernel, LdsLimit>()) return why;
  Kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(args...);
  return hipGetLastError() == hipSuccess ? nullptr : "launch failed";
}

// the head's shape and the offsets of its weights in the packed blob
struct Shape {
  int32_t in0, in1, in, Hd, L, relu, fnorm, RN, kind, A;
  int32_t SX, SA;          // padded LDS row strides: the input row, an activation row
  int32_t o_fn, o_fc[MAX_LAYERS + 1], o_gru[MAX_RNN], o_rn, o_out;
};

// A kernel's entry: this block's tile of a call of total rows, as the tile functions' leading arguments (rows
// row0 .. row0 + rows - 1, lane = row, the wave's index, the tile's LDS)
struct Tile {
  int64_t row0;
  int rows, lane, wv;
  float* lds;
};

__device__ __forceinline__ Tile block_tile(int64_t total) {
  extern __shared__ float4 lds4[];
  const int64_t row0 = (int64_t)blockIdx.x * TILE;
  const int64_t left = total - row0;
  // the wave's index as a scalar: the weight addresses derived from it are then lane-uniform to the compiler
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x / TILE);
  return {row0, left < TILE ? (int)left : TILE, (int)threadIdx.x & (TILE - 1), wv, reinterpret_cast<float*>(lds4)};
}

// What MLPBase and a GRU layer hand out on their way, for lsm_backward.hip's stage 1 to keep. rows(): the
// tile's rows of layer k's array are whole (every thread calls it behind the barrier; the hook knows the
// buffers). gates(): GRU layer l's r, z, n and hg = W_hn h + b_hn of column j, from the thread that computed
// them. The default keeps nothing and compiles to nothing.
enum Saved { SAVED_INPUT, SAVED_ACT, SAVED_NORM };   // fc1's input (X), a layer's activation (nxt), its norm (cur)
struct NoSaves {
  LSM_HD void rows(Saved, int) const {}
  LSM_HD void gates(int, int, float, float, float, float) const {}
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

// The tile-row copies, by all of the tile's threads, consecutive threads on consecutive floats of a row: n
// floats of each of rows rows, between LDS rows stride floats apart (from column col on) and rows m0 .. of a
// global array whose rows are n + gap floats apart. Float i is column c of row r: LDS index r * stride + col
// + c, global index m0 * n + i + (m0 + r) * gap (gap 0, a [.][n] array: m0 * n + i). The caller's barrier
// precedes save_rows and follows load_rows. load_rows reads through f(value, r): nothing, or a row's factor.
struct AsIs {
  LSM_HD float operator()(float v, int) const { return v; }
};
struct TimesRow {   // factor[m0 + r]: a [.] array's rows m0 ..
  const float* factor;
  int64_t m0;
  LSM_HD float operator()(float v, int r) const { return v * factor[m0 + r]; }
};

LSM_HD void save_rows(const float* src, int stride, int n, float* dst, int64_t m0, int rows, int tid, int nt,
                      int gap = 0, int col = 0) {
  for (int i = tid; i < rows * n; i += nt) {
    const int r = i / n, c = i - r * n;
    dst[m0 * n + i + (m0 + r) * gap] = src[r * stride + col + c];
  }
}

template <class F = AsIs>
LSM_HD void load_rows(float* dst, int stride, int n, const float* src, int64_t m0, int rows, int tid, int nt,
                      int gap = 0, F f = {}, int col = 0) {
  for (int i = tid; i < rows * n; i += nt) {
    const int r = i / n, c = i - r * n;
    dst[r * stride + col + c] = f(src[m0 * n + i + (m0 + r) * gap], r);
  }
}

// the virtual cat([x0, x1]) of rows row0 .. row0 + rows - 1: one LDS row per tile row, read coalesced. The
// caller's barrier follows.
LSM_HD void load_inputs(const Shape& n, const float* x0, const float* x1, int64_t row0, int rows, float* X, int tid,
                        int nt) {
  load_rows(X, n.SX, n.in0, x0, row0, rows, tid, nt);
  load_rows(X, n.SX, n.in1, x1, row0, rows, tid, nt, 0, AsIs{}, n.in0);
}

// MLPBase on the lane's staged input row: the feature norm, then fc1 and fc2[i], each Linear, activation,
// LayerNorm. xrow is overwritten by the feature norm; the result is in cur (nxt is scratch); the last
// barrier has been passed on return. The hook sees fc1's input and every layer's activation and LayerNorm
// output, each behind the barrier that makes the tile's rows whole.
template <class Hook = NoSaves>
LSM_HD void mlp(const Shape& n, const float* __restrict__ w, float* xrow, float* cur, float* nxt, int wv, int nw,
                Hook hook = {}) {
  const int in = n.in, Hd = n.Hd;
  if (n.fnorm) {
    layer_norm(xrow, xrow, in, w + n.o_fn, w + n.o_fn + in, wv, nw);
    LSM_SYNC();
  }
  hook.rows(SAVED_INPUT, 0);
  for (int k = 0; k <= n.L; ++k) {
    const int din = k == 0 ? in : Hd;
    const float* W = w + n.o_fc[k];
    const float* b = W + Hd * din;
    linear(W, b, Hd, din, k == 0 ? xrow : cur, nxt, wv, nw, n.relu ? 1 : 2);
    LSM_SYNC();
    hook.rows(SAVED_ACT, k);
    layer_norm(nxt, cur, Hd, b + Hd, b + 2 * Hd, wv, nw);
    LSM_SYNC();
    hook.rows(SAVED_NORM, k);
  }
}

// GRU layer l of the lane's row: o[j] = h'_j for this wave's column blocks, from the layer's input x and
// its state h (both whole LDS rows; h already holds state * mask). No barrier inside: the caller's follows.
template <class Hook = NoSaves>
LSM_HD void gru_layer(const Shape& n, const float* __restrict__ w, int l, const float* x, const float* h, float* o,
                      int wv, int nw, Hook hook = {}) {
  const int Hd = n.Hd;
  const float* Wih = w + n.o_gru[l];
  const float* Whh = Wih + 3 * Hd * Hd;
  const float* bih = Whh + 3 * Hd * Hd;
  const float* bhh = bih + 3 * Hd;
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
    dot4(Whh + j0 * Hd, Hd, nj, h, Hd, hr);
    dot4(Whh + (Hd + j0) * Hd, Hd, nj, h, Hd, hz);
    dot4(Whh + (2 * Hd + j0) * Hd, Hd, nj, h, Hd, hg);
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      if (jj >= nj) continue;
      const float r = sigmoid_(ir[jj] + hr[jj]);
      const float z = sigmoid_(iz[jj] + hz[jj]);
      const float g = tanhf(fma_(r, hg[jj], ig[jj]));
      const float hp = fma_(z, h[j0 + jj], (1.0f - z) * g);
      o[j0 + jj] = hp;
      hook.gates(l, j0 + jj, r, z, g, hg[jj]);
    }
  }
}

// The first two walks over a row's A logits, a ascending, in one lane: the availability mask (-FLT_MAX where
// avail[a] == 0; avail NULL: none), written back to lg and, when given, to logits; mx, the first a
// attaining it, and s = sum of exp(lg[a] - mx).
LSM_HD void masked_softmax(float* lg, int A, const float* avail, float* logits, float& mx, int& first, float& s) {
  mx = 0.0f;
  first = 0;
  for (int a = 0; a < A; ++a) {
    float l = lg[a];
    if (avail && avail[a] == 0.0f) l = -FLT_MAX;
    lg[a] = l;
    if (logits) logits[a] = l;
    if (a == 0 || l > mx) mx = l, first = a;
  }
  s = 0.0f;
  for (int a = 0; a < A; ++a) s += expf(lg[a] - mx);
}

// include/lsm_evaluate.h's clamp of a stored action (lsm_evaluate.hip, lsm_loss.hip); flags what it had to change
LSM_HD int clamp_action(float a, int A, bool& bad) {
  bad = !(a >= 0.0f && a < (float)A && a == floorf(a));
  if (!(a == a)) return 0;
  const float c = a < 0.0f ? 0.0f : a > (float)(A - 1) ? (float)(A - 1) : a;
  return (int)c;
}

// ---- host side: the config's checks ----------------------------------------------------------------------

constexpr int pad(int w) { return ((w + 3) & ~3) + 4; }

inline bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

inline int refuse(const char* prefix, const char* msg) { return lsm_policy_set_error(prefix, msg), 1; }

// the workgroups of a call: one per TILE rows
inline int64_t tiles_of(int64_t rows) { return (rows + TILE - 1) / TILE; }

// a tile's LDS bytes, from its floats per row
inline size_t tile_bytes(size_t row_floats) { return (size_t)TILE * row_floats * sizeof(float); }

// whether [a, a + na) and [b, b + nb) share a byte; a null pointer or an empty range shares none
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// The sizes of a call: T >= 1 steps of C >= 0 rows each, T * C rows within INT32_MAX. c, tc and whole: the
// unit's words for C, for T * C and for what the caller should split. 0 when fine.
inline int check_sizes(const char* prefix, const char* c, const char* tc, const char* whole, int64_t C, int32_t T) {
  char msg[96];
  if (T < 1) return refuse(prefix, "T < 1");
  if (C < 0) return snprintf(msg, sizeof msg, "%s < 0", c), refuse(prefix, msg);
  if (C <= INT32_MAX / (int64_t)T) return 0;
  return snprintf(msg, sizeof msg, "%s exceeds INT32_MAX rows; split the %s", tc, whole), refuse(prefix, msg);
}

// The checks of a call's io struct (lsm_head_io, lsm_eval_io, lsm_bwd_io: the same field names) that the units
// share. Each returns nullptr or the refusal's text; rows: of the call, 0 asks for no input. The fields a
// config does not read are dropped first, so they are not checked either.
template <class Io>
void drop_unread(const Shape& n, Io* f) {
  if (n.in0 == 0) f->x0 = nullptr;
  if (n.in1 == 0) f->x1 = nullptr;
  if (n.RN == 0) f->rnn_states = f->masks = nullptr;
}

template <class Io>
const char* inputs_missing(const Shape& n, const Io& f, int64_t rows) {
  return rows > 0 && ((n.in0 > 0 && !f.x0) || (n.in1 > 0 && !f.x1)) ? "x0 / x1 is null" : nullptr;
}

template <class Io>
const char* states_missing(const Shape& n, const Io& f, int64_t rows) {
  const bool missing = rows > 0 && n.RN > 0 && (!f.rnn_states || !f.masks);
  return missing ? "the recurrent form needs rnn_states and masks" : nullptr;
}

inline const char* misaligned(std::initializer_list<const void*> ps, uintptr_t mask = 3,
                              const char* text = "misaligned pointer") {
  for (const void* p : ps)
    if ((uintptr_t)p & mask) return text;
  return nullptr;
}

// lsm_head_forward's and lsm_head_evaluate's order of them, after the unit's own drops: the inputs, 4-byte
// alignment (p4: the unit's own pointers besides the common ones), 8-byte alignment (p8, with the unit's
// text), the states, rnn_out against rnn_states (rows rows of RN * Hd floats each)
template <class Io>
const char* check_io(const Shape& n, const float* weights, const Io& f, int64_t rows,
                     std::initializer_list<const void*> p4, std::initializer_list<const void*> p8,
                     const char* p8_text) {
  const char* why = inputs_missing(n, f, rows);
  if (!why) why = misaligned({weights, f.x0, f.x1, f.rnn_states, f.masks, f.features, f.rnn_out});
  if (!why) why = misaligned(p4);
  if (!why) why = misaligned(p8, 7, p8_text);
  if (!why) why = states_missing(n, f, rows);
  const size_t bytes = (size_t)rows * n.RN * n.Hd * sizeof(float);
  if (!why && overlap(f.rnn_out, bytes, f.rnn_states, bytes)) why = "rnn_out overlaps rnn_states";
  return why;
}

// the config's checks and the blob's offsets; returns the blob's length in floats, 0 with a text
// ("<prefix>...") on refusal
inline size_t layout(const lsm_head_config& c, Shape* n, const char* prefix) {
  auto fail = [prefix](const char* msg) { return lsm_policy_set_error(prefix, msg), (size_t)0; };
  if (c.in0 < 0 || c.in1 < 0) return fail("in0 and in1 must be >= 0");
  if (c.in0 > MAX_IN || c.in1 > MAX_IN || !in_range(c.in0 + c.in1, 1, MAX_IN))
    return fail("in0 + in1 must be in [1, 256]");
  if (!in_range(c.hidden, 1, MAX_HIDDEN)) return fail("hidden must be in [1, 128]");
  if (!in_range(c.layer_N, 0, MAX_LAYERS)) return fail("layer_N must be in [0, 4]");
  if (!in_range(c.recurrent_N, 0, MAX_RNN)) return fail("recurrent_N must be in [0, 2]");
  if (c.kind != LSM_HEAD_ACTOR && c.kind != LSM_HEAD_CRITIC) return fail("unknown kind");
  if (c.kind == LSM_HEAD_ACTOR && !in_range(c.num_actions, 1, MAX_ACTIONS))
    return fail("num_actions must be in [1, 64]");
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

}  // namespace lsm_head_tile
#endif
