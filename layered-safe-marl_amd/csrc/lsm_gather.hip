// lsm_gather.hip -- one minibatch of GraphReplayBuffer.feed_forward_generator in one launch.
//
// Reference: onpolicy/utils/graph_buffer.py:401-453: every field is reshaped to [T * n * N][row] and
// indexed with the minibatch's sample indices (share_obs[indices], obs[indices], ...). Here all fields
// are gathered by one kernel: dst[b] = src[indices[b]], the field descriptors passed by value in the
// kernel arguments (blockIdx.y = field). A row is copied in 16-B units where row_bytes, src and dst
// allow it, else in 4-B units (the same split as insert_kernel in lsm_buffer.hip); unit q of a field
// belongs to sample q / units_per_row, so consecutive lanes store consecutive addresses.
//
// LSM_GATHER_COMPACT_ADJ serves the compact adjacency layout, which has no per-sample row to copy:
// sample i's [E][E] matrix is the table A[i / N] with the rows and columns of its disconnect bits
// zeroed, dst[b][r][c] = (bit r | bit c of masks[i]) ? 0 : A[i / N][r][c] -- a select, not a product
// (the reference assigns 0 in place, whatever the table holds; see vec_env.expand_compact_adj).
//
// An index outside [0, rows) zero-fills the sample in every field and sets *bad = 1 (a plain store);
// no address is formed from it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/lsm_learner.h"

namespace {

constexpr int GATHER_BLOCK = 256;
constexpr int GATHER_MAX_BLOCKS_X = 2048;   // 256 CUs x 8 workgroups; the rest is grid-strided
// most copy units (B * units per row) in one field of one call: 32-bit unit counters with room for one grid stride
constexpr int64_t GATHER_MAX_UNITS = 0xffffffffLL - (int64_t)GATHER_MAX_BLOCKS_X * GATHER_BLOCK;

struct GatherField {
  const void* src;
  void* dst;
  const uint64_t* masks;
  int64_t units;   // copy units per sample row: 16-B units when vec, else 4-B units
  int32_t kind, vec, E, N;
};

struct GatherArgs {
  GatherField f[LSM_GATHER_MAX_FIELDS];
  const int64_t* indices;
  int64_t B, rows;
  int64_t* bad;
};

__device__ __forceinline__ bool mask_bit(const uint64_t* w, int e) { return (w[e >> 6] >> (e & 63)) & 1; }

// Units are counted in 32 bits (the cheap division): the host refuses a field with more than
// GATHER_MAX_UNITS of them, so q + stride cannot wrap.
__device__ __forceinline__ void gather_field(const GatherField& f, const int64_t* __restrict__ indices, uint32_t total,
                                             int64_t rows, int64_t* bad) {
  const uint32_t units = (uint32_t)f.units;
  const uint32_t stride = gridDim.x * GATHER_BLOCK;
  for (uint32_t q = blockIdx.x * GATHER_BLOCK + threadIdx.x; q < total; q += stride) {
    const uint32_t b = q / units, u = q - b * units;
    const int64_t i = indices[b];
    const bool ok = i >= 0 && i < rows;
    if (!ok && u == 0 && bad) *bad = 1;
    if (f.kind == LSM_GATHER_ROWS) {
      if (f.vec) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (ok) v = ((const uint4*)f.src)[(int64_t)i * f.units + u];
        ((uint4*)f.dst)[q] = v;
      } else {
        uint32_t v = 0u;
        if (ok) v = ((const uint32_t*)f.src)[(int64_t)i * f.units + u];
        ((uint32_t*)f.dst)[q] = v;
      }
    } else {
      const int E = f.E, W = (E + 63) >> 6;
      const uint64_t* w = f.masks + (ok ? i : 0) * W;
      const int64_t tab = ok ? (int64_t)((uint32_t)i / (uint32_t)f.N) : 0;   // rows < 2^32 (host check)
      const float* A = (const float*)f.src + tab * E * E;
      if (f.vec) {   // E % 4 == 0: the unit's four columns share a row
        const int e0 = (int)u * 4, r = e0 / E, c = e0 - r * E;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok && !mask_bit(w, r)) {
          v = ((const float4*)A)[u];
          const uint32_t cb = (uint32_t)(w[c >> 6] >> (c & 63));   // c % 4 == 0: bits c .. c+3 share a word
          if (cb & 1u) v.x = 0.0f;
          if (cb & 2u) v.y = 0.0f;
          if (cb & 4u) v.z = 0.0f;
          if (cb & 8u) v.w = 0.0f;
        }
        ((float4*)f.dst)[q] = v;
      } else {
        const int e = (int)u, r = e / E, c = e - r * E;
        float v = 0.0f;
        if (ok && !mask_bit(w, r) && !mask_bit(w, c)) v = A[e];
        ((float*)f.dst)[q] = v;
      }
    }
  }
}

__global__ __launch_bounds__(GATHER_BLOCK) void gather_kernel(GatherArgs a) {
  const GatherField& f = a.f[blockIdx.y];
  gather_field(f, a.indices, (uint32_t)(a.B * f.units), a.rows, a.bad);
}

thread_local char g_err[256];

int fail(const char* m) {
  snprintf(g_err, sizeof g_err, "%s", m);
  return 1;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" {

const char* lsm_gather_last_error(void) { return g_err; }

int lsm_buffer_gather(const lsm_gather_field* fields, int32_t nfields, const int64_t* indices, int64_t B,
                      int64_t rows, int64_t* bad, void* hip_stream) {
  if (!fields) return fail("gather: null fields");
  if (nfields < 1 || nfields > LSM_GATHER_MAX_FIELDS) return fail("gather: nfields outside 1..16");
  if (!indices) return fail("gather: null indices");
  if (B < 1) return fail("gather: B < 1");
  if (rows < 1) return fail("gather: rows < 1");
  GatherArgs a;
  int64_t most = 0;
  for (int k = 0; k < nfields; ++k) {
    const lsm_gather_field& in = fields[k];
    GatherField& f = a.f[k];
    if (!in.src || !in.dst) return fail("gather: null src / dst in a field");
    if (!aligned4(in.src) || !aligned4(in.dst)) return fail("gather: src / dst not 4-byte aligned");
    f.src = in.src;
    f.dst = in.dst;
    f.kind = in.kind;
    f.masks = nullptr;
    f.E = f.N = 0;
    if (in.kind == LSM_GATHER_ROWS) {
      if (in.row_bytes < 4 || (in.row_bytes & 3) != 0) return fail("gather: row_bytes not a positive multiple of 4");
      f.vec = (in.row_bytes & 15) == 0 && aligned16(in.src) && aligned16(in.dst);
      f.units = in.row_bytes / (f.vec ? 16 : 4);
    } else if (in.kind == LSM_GATHER_COMPACT_ADJ) {
      if (!in.masks) return fail("gather: compact adjacency field without masks");
      if (((uintptr_t)in.masks & 7) != 0) return fail("gather: masks not 8-byte aligned");
      if (in.E < 1 || in.E > 4096) return fail("gather: compact adjacency field with E outside 1..4096");
      if (in.N < 1) return fail("gather: compact adjacency field with N < 1");
      if (rows % in.N != 0) return fail("gather: rows not a multiple of N in a compact adjacency field");
      if (rows > 0xffffffffLL) return fail("gather: more than 2^32 - 1 rows with a compact adjacency field");
      f.masks = in.masks;
      f.E = in.E;
      f.N = in.N;
      f.vec = (in.E & 3) == 0 && aligned16(in.src) && aligned16(in.dst);
      f.units = (int64_t)in.E * in.E / (f.vec ? 4 : 1);
    } else {
      return fail("gather: unknown field kind");
    }
    if (f.units > GATHER_MAX_UNITS / B) return fail("gather: more than 2^32 - 2^19 copy units in a field; split the minibatch");
    if (B * f.units > most) most = B * f.units;
  }
  for (int k = nfields; k < LSM_GATHER_MAX_FIELDS; ++k) a.f[k] = GatherField{nullptr, nullptr, nullptr, 0, 0, 0, 0, 0};
  a.indices = indices;
  a.B = B;
  a.rows = rows;
  a.bad = bad;
  int64_t bx = (most + GATHER_BLOCK - 1) / GATHER_BLOCK;
  if (bx > GATHER_MAX_BLOCKS_X) bx = GATHER_MAX_BLOCKS_X;
  gather_kernel<<<dim3((unsigned)bx, (unsigned)nfields), GATHER_BLOCK, 0, (hipStream_t)hip_stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : fail("gather_kernel launch failed");
}

}  // extern "C"
