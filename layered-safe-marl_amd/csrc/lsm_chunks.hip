// lsm_chunks.hip -- one minibatch of GraphReplayBuffer.recurrent_generator in one launch, and the
// policy-side rows of one env step in one launch (include/lsm_recurrent.h).
//
// Reference: onpolicy/utils/graph_buffer.py:597-755. Every field is viewed (env, agent, t)-major
// (_cast / transpose(1, 2, 0, ...)), cut into chunks of L consecutive samples, and a minibatch stacks
// its C chunks time-major: destination row l * C + b holds step l of the b-th chunk; the recurrent
// states are taken at l = 0 only. Here the buffers stay [T][M][row]: sample f = c * L + l of that view
// is buffer row (f % T) * M + f / T (chunk_row), and one kernel gathers all fields, the descriptors
// passed by value in the kernel arguments (blockIdx.y = field), as gather_kernel in lsm_gather.hip does
// for the feed-forward generator.
//
// Shape of the kernel: one thread per copy unit (16 B where row_bytes, src and dst allow it, else 4 B),
// unit q of a field belongs to destination row q / units, so consecutive lanes store consecutive
// addresses; 2048 workgroups at most, the rest grid-strided. A unit needs q / units, then row / C and
// f / T to find its source row (and i / N, e / E for the compact adjacency). hipcc expands a 32-bit
// division by a run-time divisor into about 20 instructions (a float reciprocal refined in integers:
// 7, then multiply-high and two correction steps: 10 or more); three to five of those per unit, in
// threads that mostly copy one unit each, would weigh on a path DESIGN.md already suspects of being
// instruction-bound, and most fields have one to six units per row, so "once per row" saves little.
// Instead every divisor comes with a reciprocal computed on the host, m = floor(2^32 / d):
// q^ = mulhi(n, m) is floor(n / d) or one less for every n < 2^32 (n * m / 2^32 = n / d - n * e / 2^32
// with 0 <= e < 1), so one multiply-high, one multiply and one compare-and-correct, 8 instructions,
// give the exact quotient and remainder (fast_div). Everything is counted in 32 bits; the host refuses
// T * M >= 2^32 and fields with more than CHUNK_MAX_UNITS units.
//
// The per-unit routine (chunk_unit) and the chunk-to-row function are ONE __host__ __device__ text:
// lsm_host_gather_chunks runs them on the CPU, so tests without a GPU pin the arithmetic the kernel
// runs. No LDS, no atomics; *bad is a plain store of 1.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/lsm_recurrent.h"

namespace {

constexpr int CHUNK_BLOCK = 256;
constexpr int CHUNK_MAX_BLOCKS_X = 2048;   // 256 CUs x 8 workgroups; the rest is grid-strided
// most copy units in one field of one call: 32-bit unit counters with room for one grid stride
constexpr int64_t CHUNK_MAX_UNITS = 0xffffffffLL - (int64_t)CHUNK_MAX_BLOCKS_X * CHUNK_BLOCK;

#define LSM_HD __host__ __device__ __forceinline__

// Division by a launch-invariant d >= 1 with its host-made reciprocal m = floor(2^32 / d)
// (2^32 - 1 for d = 1): exact for every n < 2^32 after one correction step.
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

// Buffer row of step l of chunk c: sample f = c * L + l of the (column, t)-major view.
// c < (T * M) / L and l < L, so f < T * M < 2^32 and the result is below T * M.
LSM_HD uint32_t chunk_row(uint32_t c, uint32_t l, uint32_t L, Div T, uint32_t M) {
  uint32_t t;
  const uint32_t col = fast_div(c * L + l, T, t);
  return t * M + col;
}

struct ChunkField {
  const void* src;
  void* dst;
  const uint64_t* masks;
  Div units;   // copy units per row: 16-B units when vec, else 4-B units
  Div N, E;    // compact adjacency
  int32_t kind, vec;
};

struct ChunkArgs {
  ChunkField f[LSM_CHUNK_MAX_FIELDS];
  const int64_t* chunks;
  Div C, T;
  uint32_t L, M;
  int64_t nchunks;   // (T * M) / L
  int64_t* bad;
};

LSM_HD bool mask_bit(const uint64_t* w, uint32_t e) { return (w[e >> 6] >> (e & 63)) & 1; }

// Copy unit q of field f.
LSM_HD void chunk_unit(const ChunkArgs& a, const ChunkField& f, uint32_t q) {
  uint32_t u, b, l = 0;
  const uint32_t drow = fast_div(q, f.units, u);
  if (f.kind == LSM_CHUNK_FIRST_ROW) b = drow;
  else l = fast_div(drow, a.C, b);
  const int64_t c = a.chunks[b];
  const bool ok = c >= 0 && c < a.nchunks;
  if (!ok && u == 0 && l == 0 && a.bad) *a.bad = 1;
  const uint32_t i = ok ? chunk_row((uint32_t)c, l, a.L, a.T, a.M) : 0u;
  if (f.kind != LSM_CHUNK_COMPACT_ADJ) {
    const int64_t s = (int64_t)i * f.units.d + u;
    if (f.vec) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (ok) v = ((const uint4*)f.src)[s];
      ((uint4*)f.dst)[q] = v;
    } else {
      uint32_t v = 0u;
      if (ok) v = ((const uint32_t*)f.src)[s];
      ((uint32_t*)f.dst)[q] = v;
    }
  } else {
    const uint32_t E = f.E.d, W = (E + 63) >> 6;
    const uint64_t* w = f.masks + (int64_t)i * W;
    uint32_t agent;
    const uint32_t tab = fast_div(i, f.N, agent);
    const float* A = (const float*)f.src + (int64_t)tab * E * E;
    uint32_t col;
    if (f.vec) {   // E % 4 == 0: the unit's four columns share a row
      const uint32_t r = fast_div(u * 4u, f.E, col);
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (ok && !mask_bit(w, r)) {
        v = ((const float4*)A)[u];
        const uint32_t cb = (uint32_t)(w[col >> 6] >> (col & 63));   // col % 4 == 0: bits col .. col+3 share a word
        if (cb & 1u) v.x = 0.0f;
        if (cb & 2u) v.y = 0.0f;
        if (cb & 4u) v.z = 0.0f;
        if (cb & 8u) v.w = 0.0f;
      }
      ((float4*)f.dst)[q] = v;
    } else {
      const uint32_t r = fast_div(u, f.E, col);
      float v = 0.0f;
      if (ok && !mask_bit(w, r) && !mask_bit(w, col)) v = A[u];
      ((float*)f.dst)[q] = v;
    }
  }
}

// destination rows of a field: C for the chunks' first rows, L * C otherwise
LSM_HD uint32_t field_rows(const ChunkArgs& a, const ChunkField& f) {
  return f.kind == LSM_CHUNK_FIRST_ROW ? a.C.d : a.L * a.C.d;
}

__global__ __launch_bounds__(CHUNK_BLOCK) void gather_chunks_kernel(ChunkArgs a) {
  const ChunkField& f = a.f[blockIdx.y];
  const uint32_t total = field_rows(a, f) * f.units.d;   // <= CHUNK_MAX_UNITS: q + stride cannot wrap
  const uint32_t stride = gridDim.x * CHUNK_BLOCK;
  for (uint32_t q = blockIdx.x * CHUNK_BLOCK + threadIdx.x; q < total; q += stride) chunk_unit(a, f, q);
}

// ---- per-step row copies ----------------------------------------------------------------------------

struct RowCopy {
  const void* src;
  void* dst;
  Div units;
  int32_t vec, zero;
};

struct CopyArgs {
  RowCopy c[LSM_COPY_MAX];
  const uint8_t* dones;
  uint32_t M;
};

__global__ __launch_bounds__(CHUNK_BLOCK) void copy_rows_kernel(CopyArgs a) {
  const RowCopy& c = a.c[blockIdx.y];
  const uint32_t total = a.M * c.units.d;
  const uint32_t stride = gridDim.x * CHUNK_BLOCK;
  for (uint32_t q = blockIdx.x * CHUNK_BLOCK + threadIdx.x; q < total; q += stride) {
    bool keep = true;
    if (c.zero) {
      uint32_t u;
      keep = a.dones[fast_div(q, c.units, u)] == 0;
    }
    if (c.vec) {
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (keep) v = ((const uint4*)c.src)[q];
      ((uint4*)c.dst)[q] = v;
    } else {
      uint32_t v = 0u;
      if (keep) v = ((const uint32_t*)c.src)[q];
      ((uint32_t*)c.dst)[q] = v;
    }
  }
}

thread_local char g_err[256];

int fail(const char* m) {
  snprintf(g_err, sizeof g_err, "%s", m);
  return 1;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

// shared argument check of the two gather_chunks entry points; fills a and the largest field's unit
// count; 0 when fine
int chunk_args(const lsm_chunk_field* fields, int32_t nfields, const int64_t* chunks, int64_t C, int64_t L, int64_t T,
               int64_t M, int64_t* bad, ChunkArgs& a, int64_t& most) {
  if (!fields) return fail("gather_chunks: null fields");
  if (nfields < 1 || nfields > LSM_CHUNK_MAX_FIELDS) return fail("gather_chunks: nfields outside 1..16");
  if (!chunks) return fail("gather_chunks: null chunks");
  if (((uintptr_t)chunks & 7) != 0) return fail("gather_chunks: chunks not 8-byte aligned");
  if (bad && ((uintptr_t)bad & 7) != 0) return fail("gather_chunks: bad not 8-byte aligned");
  if (C < 1) return fail("gather_chunks: C < 1");
  if (T < 1) return fail("gather_chunks: T < 1");
  if (M < 1) return fail("gather_chunks: M < 1");
  if (M > 0xffffffffLL / T) return fail("gather_chunks: T * M >= 2^32 samples");
  const int64_t rows = T * M;
  if (L < 1) return fail("gather_chunks: L < 1");
  if (L > rows) return fail("gather_chunks: L > T * M");
  if (C > CHUNK_MAX_UNITS / L) return fail("gather_chunks: more than 2^32 - 2^19 copy units in a field; split the minibatch");
  most = 0;
  for (int k = 0; k < nfields; ++k) {
    const lsm_chunk_field& in = fields[k];
    ChunkField& f = a.f[k];
    if (!in.src || !in.dst) return fail("gather_chunks: null src / dst in a field");
    if (!aligned4(in.src) || !aligned4(in.dst)) return fail("gather_chunks: src / dst not 4-byte aligned");
    f.src = in.src;
    f.dst = in.dst;
    f.kind = in.kind;
    f.masks = nullptr;
    f.N = f.E = make_div(1);
    int64_t units;
    if (in.kind == LSM_CHUNK_ROWS || in.kind == LSM_CHUNK_FIRST_ROW) {
      if (in.row_bytes < 4 || (in.row_bytes & 3) != 0)
        return fail("gather_chunks: row_bytes not a positive multiple of 4");
      f.vec = (in.row_bytes & 15) == 0 && aligned16(in.src) && aligned16(in.dst);
      units = in.row_bytes / (f.vec ? 16 : 4);
    } else if (in.kind == LSM_CHUNK_COMPACT_ADJ) {
      if (!in.masks) return fail("gather_chunks: compact adjacency field without masks");
      if (((uintptr_t)in.masks & 7) != 0) return fail("gather_chunks: masks not 8-byte aligned");
      if (in.E < 1 || in.E > 4096) return fail("gather_chunks: compact adjacency field with E outside 1..4096");
      if (in.N < 1) return fail("gather_chunks: compact adjacency field with N < 1");
      if (rows % in.N != 0) return fail("gather_chunks: T * M not a multiple of N in a compact adjacency field");
      f.masks = in.masks;
      f.E = make_div((uint32_t)in.E);
      f.N = make_div((uint32_t)in.N);
      f.vec = (in.E & 3) == 0 && aligned16(in.src) && aligned16(in.dst);
      units = (int64_t)in.E * in.E / (f.vec ? 4 : 1);
    } else {
      return fail("gather_chunks: unknown field kind");
    }
    const int64_t drows = in.kind == LSM_CHUNK_FIRST_ROW ? C : L * C;
    if (units > CHUNK_MAX_UNITS / drows)
      return fail("gather_chunks: more than 2^32 - 2^19 copy units in a field; split the minibatch");
    f.units = make_div((uint32_t)units);
    if (drows * units > most) most = drows * units;
  }
  for (int k = nfields; k < LSM_CHUNK_MAX_FIELDS; ++k)
    a.f[k] = ChunkField{nullptr, nullptr, nullptr, make_div(1), make_div(1), make_div(1), 0, 0};
  a.chunks = chunks;
  a.C = make_div((uint32_t)C);
  a.T = make_div((uint32_t)T);
  a.L = (uint32_t)L;
  a.M = (uint32_t)M;
  a.nchunks = rows / L;
  a.bad = bad;
  return 0;
}

}  // namespace

extern "C" {

const char* lsm_recurrent_last_error(void) { return g_err; }

int lsm_buffer_gather_chunks(const lsm_chunk_field* fields, int32_t nfields, const int64_t* chunks, int64_t C,
                             int64_t L, int64_t T, int64_t M, int64_t* bad, void* hip_stream) {
  ChunkArgs a;
  int64_t most;
  if (chunk_args(fields, nfields, chunks, C, L, T, M, bad, a, most)) return 1;
  int64_t bx = (most + CHUNK_BLOCK - 1) / CHUNK_BLOCK;
  if (bx > CHUNK_MAX_BLOCKS_X) bx = CHUNK_MAX_BLOCKS_X;
  gather_chunks_kernel<<<dim3((unsigned)bx, (unsigned)nfields), CHUNK_BLOCK, 0, (hipStream_t)hip_stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : fail("gather_chunks: kernel launch failed");
}

int lsm_host_gather_chunks(const lsm_chunk_field* fields, int32_t nfields, const int64_t* chunks, int64_t C, int64_t L,
                           int64_t T, int64_t M, int64_t* bad) {
  ChunkArgs a;
  int64_t most;
  if (chunk_args(fields, nfields, chunks, C, L, T, M, bad, a, most)) return 1;
  for (int k = 0; k < nfields; ++k) {
    const ChunkField& f = a.f[k];
    const uint32_t total = field_rows(a, f) * f.units.d;
    for (uint32_t q = 0; q < total; ++q) chunk_unit(a, f, q);
  }
  return 0;
}

int lsm_buffer_copy_rows(const lsm_row_copy* copies, int32_t ncopies, const uint8_t* dones, int64_t M,
                         void* hip_stream) {
  if (!copies) return fail("copy_rows: null copies");
  if (ncopies < 1 || ncopies > LSM_COPY_MAX) return fail("copy_rows: ncopies outside 1..8");
  if (M < 1) return fail("copy_rows: M < 1");
  if (M > CHUNK_MAX_UNITS) return fail("copy_rows: more than 2^32 - 2^19 copy units in a copy");
  CopyArgs a;
  int64_t most = 0;
  for (int k = 0; k < ncopies; ++k) {
    const lsm_row_copy& in = copies[k];
    RowCopy& c = a.c[k];
    if (!in.src || !in.dst) return fail("copy_rows: null src / dst in a copy");
    if (!aligned4(in.src) || !aligned4(in.dst)) return fail("copy_rows: src / dst not 4-byte aligned");
    if (in.row_bytes < 4 || (in.row_bytes & 3) != 0) return fail("copy_rows: row_bytes not a positive multiple of 4");
    if (in.zero_on_done && !dones) return fail("copy_rows: zero_on_done without dones");
    c.src = in.src;
    c.dst = in.dst;
    c.vec = (in.row_bytes & 15) == 0 && aligned16(in.src) && aligned16(in.dst);
    c.zero = in.zero_on_done != 0;
    const int64_t units = in.row_bytes / (c.vec ? 16 : 4);
    if (units > CHUNK_MAX_UNITS / M) return fail("copy_rows: more than 2^32 - 2^19 copy units in a copy");
    c.units = make_div((uint32_t)units);
    if (M * units > most) most = M * units;
  }
  for (int k = ncopies; k < LSM_COPY_MAX; ++k) a.c[k] = RowCopy{nullptr, nullptr, make_div(1), 0, 0};
  a.dones = dones;
  a.M = (uint32_t)M;
  int64_t bx = (most + CHUNK_BLOCK - 1) / CHUNK_BLOCK;
  if (bx > CHUNK_MAX_BLOCKS_X) bx = CHUNK_MAX_BLOCKS_X;
  copy_rows_kernel<<<dim3((unsigned)bx, (unsigned)ncopies), CHUNK_BLOCK, 0, (hipStream_t)hip_stream>>>(a);
  return hipGetLastError() == hipSuccess ? 0 : fail("copy_rows: kernel launch failed");
}

}  // extern "C"
