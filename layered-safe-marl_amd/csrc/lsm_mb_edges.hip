// lsm_mb_edges.hip -- GNNBase.process_adj of a minibatch whose graphs are named by ids into the device
// replay buffer (include/lsm_minibatch_edges.h): the dense [G][E][E] minibatch adjacency is never built.
//
// Reference: the minibatch adj of GraphReplayBuffer.feed_forward_generator / recurrent_generator
// (onpolicy/utils/graph_buffer.py:368-453, 597-755) has one consumer, GNNBase.forward
// (onpolicy/algorithms/utils/gnn.py:545-564), which passes it to process_adj (gnn.py:376-407) and uses
// only edge_index / edge_attr from then on. Here graph g of the minibatch is read where the buffer
// holds it: row i(g) of the reference layout's adj[rows][E][E], or table i(g) / N and disconnect words
// i(g) of the compact layout, expanded on the fly ((bit r | bit c) ? +0 : A[r][c], a select).
//
// The work split and the element loop are lsm_edges.hip's, carried over rather than shared (that file
// stays as it is): one wave per graph, four graphs per 256-thread workgroup; the graph walked as a flat
// index in 64-lane chunks (16-B loads when E is even and adj 16-byte aligned, 4-B otherwise), every load of a batch issued
// before its first use; counts from ballots; the emit kernel compacts a chunk's edges in the wave's LDS
// slice at their mbcnt prefix and consecutive lanes store them. The disconnect words stay in registers
// as SSA values and the mask is a branch-free AND on the bit pattern (mbit / mask_val, no indexable
// array of mask words: DESIGN.md, round 6's note on the edge kernels' masked select).
// The kernels are compiled twice over the mask test: graphs with one mask word (E <= 64) and the general form.
// Three launches: count kernel, hipcub's inclusive scan, emit kernel; the launch boundaries order them.
// No floating-point atomics, no device-scope fences; *bad is a plain store of 1.
//
// New here is resolving i(g) before anything else: the wave's graph number is made scalar
// (readfirstlane), so the id is loaded once per wave; for chunk ids g = l * C + b, f = ids[b] * L + l and
// row (f % T) * M + f / T use lsm_chunks.hip's fast_div with host-made reciprocals, as does i / N for
// the compact table. The id is range-checked first: a bad id's wave forms no address from it, counts
// zero edges and leaves the kernel. The source-row function (source_row) and the per-element value
// (graph_value: mask, then the != 0 test of nonzero()) are ONE __host__ __device__ text that
// lsm_host_mb_edges also runs, so tests without a GPU pin the arithmetic the kernels run.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_scan.hpp>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/lsm_minibatch_edges.h"

namespace {

constexpr int WAVE = 64;
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int GRAPHS_PER_BLOCK = 4;   // 256-thread workgroups, one wave per graph
constexpr int CH = 4;                 // chunks of WAVE * VEC elements per memory round trip

#define LSM_HD __host__ __device__ __forceinline__

// Division by a launch-invariant d >= 1 with its host-made reciprocal m = floor(2^32 / d)
// (2^32 - 1 for d = 1): exact for every n < 2^32 after one correction step (lsm_chunks.hip).
struct Div {
  uint32_t d, m;
};

Div make_div(uint32_t d) { return Div{d, d <= 1 ? 0xffffffffu : (uint32_t)((1ULL << 32) / d)}; }

LSM_HD uint32_t fast_div(uint32_t n, Div v, uint32_t& rem) {
  uint32_t q = (uint32_t)(((uint64_t)n * v.m) >> 32);
  uint32_t r = n - q * v.d;
  if (r >= v.d) {
    ++q;
    r -= v.d;
  }
  rem = r;
  return q;
}

struct MbSrc {
  const float* adj;         // reference: [rows][E][E]; compact: [rows / N][E][E]
  const uint64_t* masks;    // compact only: [rows][W]; nullptr for reference
  const int64_t* ids;       // [C]
  int64_t G;                // graphs: C (indices) or L * C (chunks)
  int64_t limit;            // ids are valid in [0, limit): rows, or rows / L for chunks
  int64_t* bad;
  Div C, T, N;
  uint32_t L, M;
  int32_t E, W, kind;
  float inv_e;              // 1 / E for the flat-index row split
};

// Source row i(g) of graph g < G (< 2^31); ok = false for an id outside its range, from which nothing
// is computed. c < rows / L and l < L, so f = c * L + l < rows < 2^32.
LSM_HD uint32_t source_row(const MbSrc& s, uint32_t g, bool& ok) {
  if (s.kind == LSM_MB_INDICES) {
    const int64_t id = s.ids[g];
    ok = id >= 0 && id < s.limit;
    return ok ? (uint32_t)id : 0u;
  }
  uint32_t b, t;
  const uint32_t l = fast_div(g, s.C, b);
  const int64_t c = s.ids[b];
  ok = c >= 0 && c < s.limit;
  if (!ok) return 0u;
  const uint32_t col = fast_div((uint32_t)c * s.L + l, s.T, t);
  return t * s.M + col;
}

// Row of flat index k (< E*E <= 65536): floor((k + 0.5) / E) in fp32 is exact here -- the
// distance of (k + 0.5) / E from an integer is >= 0.5 / E >= 1/512, far above fp32 rounding.
LSM_HD int row_of(int k, float inv_e) { return (int)(((float)k + 0.5f) * inv_e); }

// The compact layout's disconnect words of one graph (W = ceil(E / 64) <= 4), loaded once per graph
// before its element loads and held in registers.
struct MaskRegs {
  uint64_t w0, w1, w2, w3;
  bool on;   // compact layout
};

LSM_HD MaskRegs load_masks(const uint64_t* m, int W) {
  MaskRegs M;
  M.on = m != nullptr;
  M.w0 = M.w1 = M.w2 = M.w3 = 0ull;
  if (M.on) {
    // wave-uniform address: one load per word for the wave, complete before the first use
    M.w0 = m[0];
    if (W > 1) M.w1 = m[1];
    if (W > 2) M.w2 = m[2];
    if (W > 3) M.w3 = m[3];
  }
  return M;
}

// bit r of the graph's disconnect words: an OR of masked words (no selection by index). ONE: the graph
// has one word (E <= 64, the headline shape's 24), a compile-time choice made per launch -- the general
// form costs about twenty 64-bit selects and ORs per bit, two bits per element
template <bool ONE>
LSM_HD uint32_t mbit(const MaskRegs M, int r) {
  if (ONE) return (uint32_t)(M.w0 >> (r & 63)) & 1u;
  const uint32_t q = (uint32_t)r >> 6;
  const uint64_t x = (M.w0 & (0ull - (uint64_t)(q == 0u))) | (M.w1 & (0ull - (uint64_t)(q == 1u))) |
                     (M.w2 & (0ull - (uint64_t)(q == 2u))) | (M.w3 & (0ull - (uint64_t)(q == 3u)));
  return (uint32_t)(x >> (r & 63)) & 1u;
}

// v, or +0.0 when row r or column c is disconnected: an AND with an all-ones / all-zeros word
template <bool ONE>
LSM_HD float mask_val(float v, const MaskRegs M, int r, int c) {
  const uint32_t drop = mbit<ONE>(M, r) | mbit<ONE>(M, c);
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) & (drop - 1u));
}

// Element k of the graph whose stored value is v: masked in the compact layout. It is an edge when
// the result != 0.0f (NaN is, -0.0 is not: torch's nonzero).
template <bool ONE>
LSM_HD float graph_value(const MbSrc& s, const MaskRegs M, int k, float v) {
  if (M.on) {   // wave-uniform
    const int r = row_of(k, s.inv_e);
    v = mask_val<ONE>(v, M, r, k - r * s.E);
  }
  return v;
}

// The stored matrix and the disconnect words of source row i (an in-range row: source_row's ok).
LSM_HD const float* graph_ptr(const MbSrc& s, uint32_t i) {
  const int64_t EE = (int64_t)s.E * s.E;
  uint32_t agent;
  return s.adj + (int64_t)(s.masks ? fast_div(i, s.N, agent) : i) * EE;
}

LSM_HD MaskRegs graph_masks(const MbSrc& s, uint32_t i) {
  return load_masks(s.masks ? s.masks + (int64_t)i * s.W : nullptr, s.W);
}

__device__ __forceinline__ int lane_id() { return __lane_id(); }

// VEC = 4 (E even, so every graph and row pair is 16-B aligned): each lane takes 4 consecutive
// elements with one 16-B load; its nonzero count c in [0, 4] is spread over 3 ballots (bit k of c),
// so the exclusive prefix over lanes is sum_k 2^k * popcount(ballot_k below the lane).
// A graph is walked in batches of CH chunks of WAVE * VEC elements: every chunk's load of a batch is
// issued before the first is used (E = 24: the whole 576-element graph in one round trip). Addresses
// are clamped into the graph (a chunk past EE re-reads the graph's first elements, L2 hits) and values
// past EE zeroed by select.
template <int VEC>
__device__ __forceinline__ void load_batch(const float* g, int k0, int EE, float (&v)[CH][VEC]) {
  const int lane = lane_id();
  typedef float f32x1 __attribute__((ext_vector_type(1)));
  typedef typename std::conditional<VEC == 4, f32x4, f32x1>::type vec_t;
  vec_t q[CH];
#pragma unroll
  for (int h = 0; h < CH; ++h) {   // every load issued first: no use, no branch between them
    const int k = k0 + h * WAVE * VEC + VEC * lane;
    q[h] = __builtin_nontemporal_load((const vec_t*)(g + (k < EE ? k : 0)));
  }
#pragma unroll
  for (int h = 0; h < CH; ++h) {
    const bool in = k0 + h * WAVE * VEC + VEC * lane < EE;
#pragma unroll
    for (int i = 0; i < VEC; ++i) v[h][i] = in ? q[h][i] : 0.0f;
  }
}

// the lane's elements k .. k + VEC - 1 of a chunk as graph values, and their nonzero count
template <int VEC, bool ONE>
__device__ __forceinline__ int mask_count(const MbSrc& s, const MaskRegs M, int k, float (&v)[VEC]) {
  int c = 0;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    v[i] = graph_value<ONE>(s, M, k + i, v[i]);
    c += v[i] != 0.0f;
  }
  return c;
}

__device__ __forceinline__ uint32_t below(uint64_t bal) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
}

// the wave's graph: a scalar, so that the id, the mask words and the graph's base are loaded once
__device__ __forceinline__ int64_t wave_graph(int& w) {
  w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  return (int64_t)blockIdx.x * GRAPHS_PER_BLOCK + w;
}

template <int VEC, bool ONE>
__global__ __launch_bounds__(256) void mb_count_kernel(MbSrc s, int64_t* __restrict__ counts,
                                                       int64_t* __restrict__ offsets) {
  int w;
  const int64_t g = wave_graph(w);
  if (g >= s.G) return;   // whole wave exits together
  if (g == 0 && lane_id() == 0) offsets[0] = 0;   // the scan fills offsets[1..G]
  bool ok;
  const uint32_t i = source_row(s, (uint32_t)g, ok);
  if (!ok) {   // wave-uniform: no address is formed from the id
    if (lane_id() == 0) {
      counts[g] = 0;
      if (s.bad) *s.bad = 1;
    }
    return;
  }
  const float* a = graph_ptr(s, i);
  const MaskRegs M = graph_masks(s, i);
  const int EE = s.E * s.E;
  int cnt = 0;
  for (int k0 = 0; k0 < EE; k0 += WAVE * VEC * CH) {
    float v[CH][VEC];
    load_batch<VEC>(a, k0, EE, v);
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      if (k0 + h * WAVE * VEC >= EE) break;   // wave-uniform: a chunk wholly past the graph
      const int c = mask_count<VEC, ONE>(s, M, k0 + h * WAVE * VEC + VEC * lane_id(), v[h]);
      if (VEC == 1) {
        cnt += __popcll(__ballot(c != 0));
      } else {
        cnt += __popcll(__ballot(c & 1)) + 2 * __popcll(__ballot(c & 2)) + 4 * __popcll(__ballot(c & 4));
      }
    }
  }
  if (lane_id() == 0) counts[g] = cnt;
}

// The chunk's edges are first compacted into the wave's LDS slice (flat index + value at their
// exclusive-prefix slot), then written out by consecutive lanes, so every store instruction covers
// consecutive edge slots. nnz < 0: read it on the device (offsets[G]); the outputs then hold `cap`
// edges, and nothing is written when nnz > cap (the caller sees nnz and reports it).
template <int VEC, bool ONE>
__global__ __launch_bounds__(256) void mb_emit_kernel(MbSrc s, const int64_t* __restrict__ offsets, int64_t nnz,
                                                      int64_t cap, int64_t* __restrict__ edge_index,
                                                      float* __restrict__ edge_attr) {
  __shared__ int32_t sk[GRAPHS_PER_BLOCK][WAVE * VEC];
  __shared__ float sv[GRAPHS_PER_BLOCK][WAVE * VEC];
  int w;
  const int64_t g = wave_graph(w);
  if (g >= s.G) return;
  if (nnz < 0) {
    nnz = offsets[s.G];
    if (nnz > cap) return;
  }
  const int64_t pos0 = offsets[g];
  const int64_t end = offsets[g + 1];
  if (pos0 >= end || end > nnz || pos0 < 0) return;   // no edges (a bad id among them), or a stale nnz
  bool ok;
  const uint32_t i = source_row(s, (uint32_t)g, ok);
  if (!ok) return;
  const float* a = graph_ptr(s, i);
  const MaskRegs M = graph_masks(s, i);
  const int EE = s.E * s.E;
  const int lane = lane_id();
  const int64_t node0 = g * s.E;
  int64_t pos = pos0;
  for (int kb = 0; kb < EE && pos < end; kb += WAVE * VEC * CH) {
    float vb[CH][VEC];
    load_batch<VEC>(a, kb, EE, vb);
#pragma unroll
    for (int h = 0; h < CH; ++h) {
      const int k0 = kb + h * WAVE * VEC;
      if (k0 >= EE || pos >= end) break;   // wave-uniform
      const int k = k0 + VEC * lane;
      float (&v)[VEC] = vb[h];
      const int c = mask_count<VEC, ONE>(s, M, k, v);
      uint32_t pre;
      int tot;
      if (VEC == 1) {
        const uint64_t bal = __ballot(c != 0);
        pre = below(bal);
        tot = __popcll(bal);
      } else {
        const uint64_t b0 = __ballot(c & 1), b1 = __ballot(c & 2), b2 = __ballot(c & 4);
        pre = below(b0) + 2 * below(b1) + 4 * below(b2);
        tot = __popcll(b0) + 2 * __popcll(b1) + 4 * __popcll(b2);
      }
      if (c) {
        int o = (int)pre;   // pre + c <= tot <= WAVE * VEC: inside the wave's slice
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
          if (v[e] != 0.0f) {
            sk[w][o] = k + e;
            sv[w][o] = v[e];
            ++o;
          }
        }
      }
      // intra-wave LDS hand-off (the block's waves run different graphs: no block barrier)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      const int room = (int)(end - pos < (int64_t)tot ? end - pos : (int64_t)tot);   // never past the slot
      for (int t = lane; t < room; t += WAVE) {
        const int kk = sk[w][t];
        const int r = row_of(kk, s.inv_e);
        edge_index[pos + t] = node0 + r;
        edge_index[nnz + pos + t] = node0 + (kk - r * s.E);
        edge_attr[pos + t] = sv[w][t];
      }
      __builtin_amdgcn_wave_barrier();   // slots are rewritten by the next chunk
      pos += room;
    }
  }
}

thread_local char g_err[256];

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "mb_edges: %s", msg);
  return 1;
}

// the descriptor's checks, shared by every entry point; fills s; 0 when fine
int make_src(const lsm_mb_graphs& d, int64_t* bad, MbSrc* s) {
  if (!d.adj) return fail("adj is null");
  if (d.E < 1 || d.E > 256) return fail("E must be in [1, 256]");
  if (d.rows < 0) return fail("rows < 0");
  if (d.rows > 0xffffffffLL) return fail("rows >= 2^32");
  if (d.masks && (d.N < 1 || d.rows % d.N != 0)) return fail("compact layout: rows must be a multiple of N > 0");
  if (d.count < 0) return fail("count < 0");
  if (d.count > 0 && !d.ids) return fail("ids is null");
  if (((uintptr_t)d.ids & 7) != 0 || ((uintptr_t)d.masks & 7) != 0 || ((uintptr_t)d.adj & 3) != 0)
    return fail("adj / masks / ids misaligned");
  if (bad && ((uintptr_t)bad & 7) != 0) return fail("bad not 8-byte aligned");
  int64_t G = d.count, limit = d.rows;
  uint32_t L = 1, M = 1, T = 1;
  if (d.kind == LSM_MB_CHUNKS) {
    if (d.L < 1) return fail("chunks: L < 1");
    if (d.L > d.rows) return fail("chunks: L > rows");
    if (d.T < 1 || d.M < 1) return fail("chunks: T < 1 or M < 1");
    if (d.M > 0xffffffffLL / d.T || d.T * d.M != d.rows) return fail("chunks: T * M != rows");
    if (d.count > INT32_MAX / d.L) return fail("G exceeds INT32_MAX graphs; split the minibatch");
    G = d.L * d.count;
    limit = d.rows / d.L;
    L = (uint32_t)d.L;
    T = (uint32_t)d.T;
    M = (uint32_t)d.M;
  } else if (d.kind != LSM_MB_INDICES) {
    return fail("unknown id kind");
  }
  if (G > INT32_MAX) return fail("G exceeds INT32_MAX graphs; split the minibatch");
  s->adj = d.adj;
  s->masks = d.masks;
  s->ids = d.ids;
  s->G = G;
  s->limit = limit;
  s->bad = bad;
  s->C = make_div((uint32_t)(d.count > 0 ? d.count : 1));
  s->T = make_div(T);
  s->N = make_div((uint32_t)(d.masks ? d.N : 1));
  s->L = L;
  s->M = M;
  s->E = d.E;
  s->W = (d.E + 63) / 64;
  s->kind = d.kind;
  s->inv_e = 1.0f / (float)d.E;
  return 0;
}

size_t scan_temp_bytes(int64_t G) {
  size_t bytes = 0;
  if (hipcub::DeviceScan::InclusiveSum(nullptr, bytes, (const int64_t*)nullptr, (int64_t*)nullptr, (int)G) !=
      hipSuccess)
    return 0;   // lsm_mb_edges_count then reports "scan failed"
  return bytes;
}

// 16-B loads: E even makes every graph a multiple of 16 bytes; the base has to be aligned as well
bool wide(const MbSrc& s) { return s.E % 2 == 0 && ((uintptr_t)s.adj & 15) == 0; }

size_t counts_bytes(int64_t G) { return ((size_t)G * sizeof(int64_t) + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

const char* lsm_mb_edges_last_error(void) { return g_err; }

size_t lsm_mb_edges_workspace_bytes(int64_t G) {
  if (G < 0 || G > INT32_MAX) return 0;
  return counts_bytes(G) + scan_temp_bytes(G) + 256;
}

int lsm_mb_edges_count(lsm_mb_graphs graphs, int64_t* offsets, void* workspace, size_t workspace_bytes,
                       int64_t* bad, void* hip_stream) {
  MbSrc s;
  if (make_src(graphs, bad, &s)) return 1;
  if (!offsets) return fail("offsets is null");
  if (!workspace) return fail("workspace is null");
  if (((uintptr_t)offsets & 7) != 0 || ((uintptr_t)workspace & 7) != 0) return fail("offsets / workspace misaligned");
  if (workspace_bytes < lsm_mb_edges_workspace_bytes(s.G)) return fail("workspace too small");
  hipStream_t st = (hipStream_t)hip_stream;
  if (s.G == 0) return hipMemsetAsync(offsets, 0, sizeof(int64_t), st) == hipSuccess ? 0 : fail("memset failed");
  int64_t* counts = (int64_t*)workspace;
  const size_t cbytes = counts_bytes(s.G);
  void* temp = (char*)workspace + cbytes;
  size_t tbytes = workspace_bytes - cbytes;
  const unsigned blocks = (unsigned)((s.G + GRAPHS_PER_BLOCK - 1) / GRAPHS_PER_BLOCK);
  const dim3 grid(blocks);
  if (wide(s) && s.W == 1) mb_count_kernel<4, true><<<grid, 256, 0, st>>>(s, counts, offsets);
  else if (wide(s)) mb_count_kernel<4, false><<<grid, 256, 0, st>>>(s, counts, offsets);
  else if (s.W == 1) mb_count_kernel<1, true><<<grid, 256, 0, st>>>(s, counts, offsets);
  else mb_count_kernel<1, false><<<grid, 256, 0, st>>>(s, counts, offsets);
  if (hipcub::DeviceScan::InclusiveSum(temp, tbytes, counts, offsets + 1, (int)s.G, st) != hipSuccess)
    return fail("scan failed");
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_mb_edges_emit(lsm_mb_graphs graphs, const int64_t* offsets, int64_t nnz, int64_t cap, int64_t* edge_index,
                      float* edge_attr, void* hip_stream) {
  MbSrc s;
  if (make_src(graphs, nullptr, &s)) return 1;
  if (!offsets) return fail("offsets is null");
  if (((uintptr_t)offsets & 7) != 0) return fail("offsets misaligned");
  if (nnz < 0 && cap < 0) return fail("cap < 0");
  const int64_t room = nnz < 0 ? cap : nnz;
  if (room > 0 && (!edge_index || !edge_attr)) return fail("edge_index / edge_attr is null");
  if (((uintptr_t)edge_index & 7) != 0 || ((uintptr_t)edge_attr & 3) != 0) return fail("edge_index / edge_attr misaligned");
  if (s.G == 0 || room == 0) return 0;
  const unsigned blocks = (unsigned)((s.G + GRAPHS_PER_BLOCK - 1) / GRAPHS_PER_BLOCK);
  hipStream_t st = (hipStream_t)hip_stream;
  const dim3 grid(blocks);
  if (nnz < 0) nnz = -1;
  if (wide(s) && s.W == 1) mb_emit_kernel<4, true><<<grid, 256, 0, st>>>(s, offsets, nnz, cap, edge_index, edge_attr);
  else if (wide(s)) mb_emit_kernel<4, false><<<grid, 256, 0, st>>>(s, offsets, nnz, cap, edge_index, edge_attr);
  else if (s.W == 1) mb_emit_kernel<1, true><<<grid, 256, 0, st>>>(s, offsets, nnz, cap, edge_index, edge_attr);
  else mb_emit_kernel<1, false><<<grid, 256, 0, st>>>(s, offsets, nnz, cap, edge_index, edge_attr);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_host_mb_edges(lsm_mb_graphs graphs, int64_t cap, int64_t* edge_index, float* edge_attr, int64_t* nnz_out,
                      int64_t* bad) {
  MbSrc s;
  if (make_src(graphs, bad, &s)) return 1;
  if (!nnz_out) return fail("nnz_out is null");
  if (cap < 0) return fail("cap < 0");
  if (cap > 0 && (!edge_index || !edge_attr)) return fail("edge_index / edge_attr is null");
  const int EE = s.E * s.E;
  int64_t nnz = 0;
  // pass 0 counts (and reports bad ids); pass 1 runs only when the edges fit and writes them
  for (int pass = 0; pass < 2; ++pass) {
    int64_t pos = 0;
    for (int64_t g = 0; g < s.G; ++g) {
      bool ok;
      const uint32_t i = source_row(s, (uint32_t)g, ok);
      if (!ok) {
        if (pass == 0 && s.bad) *s.bad = 1;
        continue;
      }
      const float* a = graph_ptr(s, i);
      const MaskRegs M = graph_masks(s, i);
      for (int k = 0; k < EE; ++k) {
        const float v = s.W == 1 ? graph_value<true>(s, M, k, a[k]) : graph_value<false>(s, M, k, a[k]);
        if (v != 0.0f) {
          if (pass == 1) {
            const int r = row_of(k, s.inv_e);
            edge_index[pos] = g * s.E + r;
            edge_index[nnz + pos] = g * s.E + (k - r * s.E);
            edge_attr[pos] = v;
          }
          ++pos;
        }
      }
    }
    if (pass == 0) {
      nnz = pos;
      *nnz_out = nnz;
      if (nnz > cap) break;
    }
  }
  return 0;
}

}  // extern "C"
