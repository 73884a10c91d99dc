// lsm_gnn_embed_backward.hip -- EmbedConv's backward pass (include/lsm_gnn_embed_backward.h states the formulas
// and the sum order): from dh0, the gradient at EmbedConv's output, to the gradient of the blob's EmbedConv
// entries (entity embedding, lin1, the shared LayerNorm, the embed layers).
//
// A team of TS lanes per graph, G graphs per workgroup, one workgroup per slab of LSM_GNN_BWD_SLAB graphs, as
// lsm_gnn_backward.hip; but lane r owns SOURCE r. Per group of G graphs:
//   0   lane r: disconnect bit, entity type, lin1's node part P_r (graph_forward phase 0's text), the graph's
//       dh0 rows, the transposed adjacency; the graph's float32 accumulators are cleared
//   W   the walk over the targets c = 0 .. E-1, uniform in the team: lane r, where r -> c is an edge, recomputes
//       the per-edge MLP (graph_forward phase 1's text) keeping a_k, xh_k and rstd_k, then steps back through it,
//       k = EL .. 0. At each step it stages dz_k and the Linear's input n_{k-1} (at lin1: dz_0, e and the edge's
//       LayerNorm terms) in its LDS rows, a lane without the edge stages zeros, and after a barrier the team's
//       lanes split the Linear's entries: each entry's chain runs over the E staged rows into the graph's
//       accumulator (tile_chains: a lane runs 8 or 4 entries of one output row at once). dP_r is summed in the
//       lane's own LDS row.
//   N   the node-fed entries (lin1's node columns and bias, the entity embedding), once per graph
//   S   the workgroup's threads add the group's graphs, ascending, to the slab's float64 accumulators
// A second kernel adds the slabs' partials in float64 and writes dembed.
//
// The per-edge state (EdgeState) is one struct per lane on the device (TS >= E: a lane owns at most one source)
// and one per node on the host, where a team of one lane runs the same text. The k loops are unrolled over
// MAX_LAYERS + 1 with a uniform guard, so that the <16> instance keeps the state in registers.
// Teams past the slab's end recompute graph B - 1 and write nothing.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_gnn_embed_backward.h"
#include "lsm_gnn_tile.h"

namespace {

constexpr int SLAB = LSM_GNN_BWD_SLAB;

struct Emb {
  Net net;              // the forward's view (the conv fields unused)
  const float* dh0;
  float* dembed;
  double* ws;           // [slabs][n]
  float* wsacc;         // [slabs][G][2 * n4], acc_lds == 0
  int32_t S;            // row stride of P, dh0, dP and the staged rows
  int32_t o_dh, o_dp, o_d, o_n, o_x, o_dis, o_ty, o_out, o_e, o_adjT, o_acc;   // float offsets in a graph's region
  int32_t n, n4;        // the EmbedConv entries, rounded up to 4
  int32_t acc_lds;
  int64_t slabs;
};

template <int HN>
struct EdgeState {
  float a[MAX_LAYERS + 1][HN];    // a_k
  float xh[MAX_LAYERS + 1][HN];   // xh_k (layer norm)
  float rs[MAX_LAYERS + 1];       // rstd_k
  float dn[HN];                   // the gradient at n_k, stepping down
  float gg[HN], gb[HN];           // the edge's LayerNorm terms
  float e;
  bool has;
};

// the owned sources of a lane and the slot of their state
#if defined(__HIP_DEVICE_COMPILE__)
#define LSM_OWNED(r) if (const int r = tid; r < E)
#define LSM_SLOT(r) 0
#else
#define LSM_OWNED(r) for (int r = tid; r < E; r += nt)
#define LSM_SLOT(r) (r)
#endif

// s += x with the addition's rounding collected in c (lsm_gnn_backward.hip's two-sum)
LSM_HD void add2(float& s, float& c, float x) {
  const float t = s + x;
  const float b = t - s;
  c += (s - (t - b)) + (x - b);
  s = t;
}

// dW[j][i] += sum over the staged rows r ascending of dz_r[j] * n_r[i]: one FMA chain per entry, continued from
// acc. Tiles of W consecutive i (W divides hd; rows are 16-byte aligned and W is 1 or a multiple of 4).
template <int W>
LSM_HD void tile_chains(float* acc, const float* sD, const float* sN, int hd, int E, int S, int tid, int nt) {
  const int per_row = hd / W;
  for (int t = tid; t < hd * per_row; t += nt) {
    const int j = t / per_row, i0 = (t - j * per_row) * W;
    float* ap = acc + j * hd + i0;
    float a[W];
#pragma unroll
    for (int u = 0; u < W; ++u) a[u] = ap[u];
#pragma unroll 4
    for (int r = 0; r < E; ++r) {
      const float d = sD[r * S + j];
      const float* nr = sN + r * S + i0;
      if constexpr (W == 1) {
        a[0] = fma_(d, nr[0], a[0]);
      } else {
#pragma unroll
        for (int u = 0; u < W; u += 4) {
          const float4 v = *reinterpret_cast<const float4*>(nr + u);
          a[u] = fma_(d, v.x, a[u]);
          a[u + 1] = fma_(d, v.y, a[u + 1]);
          a[u + 2] = fma_(d, v.z, a[u + 2]);
          a[u + 3] = fma_(d, v.w, a[u + 3]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < W; ++u) ap[u] = a[u];
  }
}

// the per-edge MLP of graph_forward's phase 1, expression by expression, with what the way back needs kept
template <int HP>
LSM_HD void edge_forward(const Emb& b, EdgeState<(HP ? HP : MAX_DIM)>& s, const float* P, const float* dhc) {
  constexpr int HN = HP ? HP : MAX_DIM;
  const Net& net = b.net;
  const int hd = HP ? HP : net.Hd, K = net.K;
  const float* __restrict__ w = net.w;
  const float e = s.e;
  float m[HN], t[HN];
#pragma unroll
  for (int i = 0; i < hd; ++i) m[i] = fma_(e, w[net.o_w1 + i * K + K - 1], P[i]);
#pragma unroll
  for (int k = 0; k <= MAX_LAYERS; ++k) {
    if (k > net.EL) continue;
    if (k > 0) {
      const float* wl = w + net.o_el + (k - 1) * (hd * hd + hd);
#pragma unroll
      for (int j = 0; j < hd; ++j) {
        float a = wl[hd * hd + j];
#pragma unroll
        for (int i = 0; i < hd; ++i) a = fma_(wl[j * hd + i], m[i], a);
        t[j] = a;
      }
#pragma unroll
      for (int j = 0; j < hd; ++j) m[j] = t[j];
    }
    act_n(m, hd, net.relu_e);
#pragma unroll
    for (int i = 0; i < hd; ++i) s.a[k][i] = m[i];
    if (net.ln) {   // layer_norm()'s expressions, with xh kept
      float sum = 0.0f;
#pragma unroll
      for (int i = 0; i < hd; ++i) sum += m[i];
      const float mean = sum / (float)hd;
      float q = 0.0f;
#pragma unroll
      for (int i = 0; i < hd; ++i) {
        const float d = m[i] - mean;
        q = fma_(d, d, q);
      }
      const float rs = rsq_(q / (float)hd + 1e-5f);
      s.rs[k] = rs;
#pragma unroll
      for (int i = 0; i < hd; ++i) {
        const float xh = (m[i] - mean) * rs;
        s.xh[k][i] = xh;
        m[i] = fma_(xh, w[net.o_gamma + i], w[net.o_beta + i]);
      }
    }
  }
#pragma unroll
  for (int i = 0; i < hd; ++i) {
    s.dn[i] = dhc[i];
    s.gg[i] = 0.0f;
    s.gb[i] = 0.0f;
  }
}

// One step back, at position k (a compile-time constant after unrolling): from dn_k to dz_k, staged in rowD with
// the Linear's input n_{k-1} in rowN (k == 0: the edge's LayerNorm terms in rowN and rowX), and on to dn_{k-1}.
template <int HP>
LSM_HD void edge_step(const Emb& b, EdgeState<(HP ? HP : MAX_DIM)>& s, int k, float* rowD, float* rowN, float* rowX) {
  constexpr int HN = HP ? HP : MAX_DIM;
  const Net& net = b.net;
  const int hd = HP ? HP : net.Hd;
  const float* __restrict__ w = net.w;
  float dz[HN];
  if (net.ln) {
    float g[HN];
    float sg = 0.0f, sgx = 0.0f;
#pragma unroll
    for (int i = 0; i < hd; ++i) {
      s.gg[i] = fma_(s.dn[i], s.xh[k][i], s.gg[i]);
      s.gb[i] += s.dn[i];
      g[i] = s.dn[i] * w[net.o_gamma + i];
      sg += g[i];
      sgx = fma_(g[i], s.xh[k][i], sgx);
    }
    const float mg = sg / (float)hd, mgx = sgx / (float)hd;
#pragma unroll
    for (int i = 0; i < hd; ++i) dz[i] = s.rs[k] * ((g[i] - mg) - s.xh[k][i] * mgx);
  } else {
#pragma unroll
    for (int i = 0; i < hd; ++i) dz[i] = s.dn[i];
  }
  if (net.relu_e) {
#pragma unroll
    for (int i = 0; i < hd; ++i) dz[i] = s.a[k][i] <= 0.0f ? 0.0f : dz[i];
  } else {
#pragma unroll
    for (int i = 0; i < hd; ++i) dz[i] *= 1.0f - s.a[k][i] * s.a[k][i];
  }
#pragma unroll
  for (int i = 0; i < hd; ++i) rowD[i] = dz[i];
  if (k > 0) {
    const float* wl = w + net.o_el + (k - 1) * (hd * hd + hd);
#pragma unroll
    for (int i = 0; i < hd; ++i) {
      rowN[i] = net.ln ? fma_(s.xh[k - 1][i], w[net.o_gamma + i], w[net.o_beta + i]) : s.a[k - 1][i];
      s.dn[i] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < hd; ++j) {
#pragma unroll
      for (int i = 0; i < hd; ++i) s.dn[i] = fma_(wl[j * hd + i], dz[j], s.dn[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < hd; ++i) {
      rowN[i] = s.gg[i];
      rowX[i] = s.gb[i];
    }
  }
}

// One graph of one group: lanes tid = 0 .. nt-1 of its team (1 on the host). acc: the graph's float32
// accumulators, [0, n) the sums and [n4, n4 + n) the collected roundings. live: the team's graph exists (g is
// B - 1 otherwise; nothing outside the team's own region is written).
template <int HP>
LSM_HD void graph_embed_backward(const Emb& b, int64_t g, int tid, int nt, float* lds, float* acc, bool live,
                                 EdgeState<(HP ? HP : MAX_DIM)>* states) {
  const Net& net = b.net;
  const int E = net.E, F = net.F, K = net.K, S = b.S, ES = net.ES, EL = net.EL;
  const int hd = HP ? HP : net.Hd;
  const float* __restrict__ w = net.w;
  float* sP = lds;
  float* sDh = lds + b.o_dh;
  float* sDP = lds + b.o_dp;
  float* sD = lds + b.o_d;
  float* sN = lds + b.o_n;
  float* sX = lds + b.o_x;
  int32_t* dis = reinterpret_cast<int32_t*>(lds + b.o_dis);
  int32_t* ty = reinterpret_cast<int32_t*>(lds + b.o_ty);
  int32_t* outf = reinterpret_cast<int32_t*>(lds + b.o_out);
  float* sE = lds + b.o_e;
  float* sAdjT = lds + b.o_adjT;
  float* accS = acc;
  float* accC = acc + b.n4;
  const float* ag = net.adj + (net.masks ? g / net.N : g) * ((int64_t)E * E);
  const float* xg = net.x + g * ((int64_t)E * F);
  const float* dhg = b.dh0 + g * ((int64_t)E * hd);

  // ---- 0: the accumulators, the node state, P (graph_forward phase 0's text), dh0 -------------------------------
  for (int t = tid; t < 2 * b.n4; t += nt) acc[t] = 0.0f;
  for (int r = tid; r < E; r += nt) {
    dis[r] = net.masks ? (int32_t)((net.masks[g * net.W + (r >> 6)] >> (r & 63)) & 1ull) : 0;
    const float* xr = xg + (int64_t)r * F;
    const float t = xr[F - 1];
    const bool okt = t > -1.0f && t < (float)net.NE;   // trunc(t) in [0, NE); NaN and inf fail
    const int ti = okt ? (int)t : 0;
    if (!okt && live && net.bad) *net.bad = 1;
    ty[r] = okt ? ti : -1;
    outf[r] = 0;
    float* P = sP + r * S;
    for (int i = 0; i < hd; ++i) {
      const float* wi = w + net.o_w1 + i * K;
      float a = w[net.o_b1 + i];
      for (int f = 0; f < F - 1; ++f) a = fma_(wi[f], xr[f], a);
      if (okt)
        for (int s = 0; s < ES; ++s) a = fma_(wi[F - 1 + s], w[net.o_emb + ti * ES + s], a);
      P[i] = a;
      sDP[r * S + i] = 0.0f;
      sDh[r * S + i] = dhg[r * hd + i];
    }
  }
  LSM_SYNC();
  if (net.adj_lds) {
    for (int k = tid; k < E * E; k += nt) {
      const int r = k / E, c = k - r * E;
      const float v = ag[k];
      sAdjT[c * E + r] = (dis[r] | dis[c]) ? 0.0f : v;
    }
    LSM_SYNC();
  }

  // ---- W: the walk over the targets -------------------------------------------------------------------------------
  for (int c = 0; c < E; ++c) {
    const float* dhc = sDh + c * S;
    LSM_OWNED(r) {
      auto& s = states[LSM_SLOT(r)];
      const float e = net.adj_lds ? sAdjT[c * E + r] : ((dis[r] | dis[c]) ? 0.0f : ag[r * E + c]);
      s.e = e;
      s.has = !(e == 0.0f);   // NaN is an edge, -0.0 is not
      if (s.has) edge_forward<HP>(b, s, sP + r * S, dhc);
    }
#pragma unroll
    for (int k = MAX_LAYERS; k >= 0; --k) {
      if (k > EL) continue;
      LSM_OWNED(r) {
        auto& s = states[LSM_SLOT(r)];
        float* rowD = sD + r * S;
        float* rowN = sN + r * S;
        float* rowX = sX + r * S;
        if (s.has) {
          edge_step<HP>(b, s, k, rowD, rowN, rowX);
          if (k == 0) {
            sE[r] = s.e;
            outf[r] = 1;
            for (int i = 0; i < hd; ++i) sDP[r * S + i] += rowD[i];
          }
        } else {   // zeros in both rows: a stale n next to a zero dz must never meet a NaN
          for (int i = 0; i < hd; ++i) {
            rowD[i] = 0.0f;
            rowN[i] = 0.0f;
          }
          if (k == 0) {
            sE[r] = 0.0f;
            for (int i = 0; i < hd; ++i) rowX[i] = 0.0f;
          }
        }
      }
      LSM_SYNC();
      if (k > 0) {   // embed layer k - 1: weight [hd][hd], then bias [hd]
        const int base = net.o_el + (k - 1) * (hd * hd + hd);
        // the weight: a lane takes W entries of one row at a time (one dz and W inputs per staged row feed W
        // independent chains; each entry's own chain is the same whatever W)
        if ((hd & 7) == 0) tile_chains<8>(accS + base, sD, sN, hd, E, S, tid, nt);
        else if ((hd & 3) == 0) tile_chains<4>(accS + base, sD, sN, hd, E, S, tid, nt);
        else tile_chains<1>(accS + base, sD, sN, hd, E, S, tid, nt);
        for (int j = tid; j < hd; j += nt) {   // the bias
          const int idx = base + hd * hd + j;
          float a = accS[idx], lo = accC[idx];
#pragma unroll 4
          for (int r = 0; r < E; ++r) add2(a, lo, sD[r * S + j]);
          accS[idx] = a;
          accC[idx] = lo;
        }
      } else {   // lin1's edge column, gamma, beta
        const int nv = net.ln ? 3 * hd : hd;
        for (int t = tid; t < nv; t += nt) {
          const int which = t / hd, i = t - which * hd;
          const int idx = which == 0 ? net.o_w1 + i * K + K - 1 : which == 1 ? net.o_gamma + i : net.o_beta + i;
          const float* src = which == 0 ? sD : which == 1 ? sN : sX;
          float a = accS[idx], lo = accC[idx];
          if (which == 0) {
#pragma unroll 4
            for (int r = 0; r < E; ++r) add2(a, lo, sE[r] * src[r * S + i]);
          } else {
#pragma unroll 4
            for (int r = 0; r < E; ++r) add2(a, lo, src[r * S + i]);
          }
          accS[idx] = a;
          accC[idx] = lo;
        }
      }
      LSM_SYNC();
    }
  }

  // ---- N: the node-fed entries ---------------------------------------------------------------------------------------
  {
    const int nw = hd * (K - 1), ne = net.NE * ES;
    for (int t = tid; t < nw + hd + ne; t += nt) {
      if (t < nw) {
        const int i = t / (K - 1), f = t - i * (K - 1);
        float a = 0.0f;
        for (int r = 0; r < E; ++r) {
          if (!outf[r]) continue;
          const float v = f < F - 1 ? xg[r * F + f] : (ty[r] >= 0 ? w[net.o_emb + ty[r] * ES + (f - (F - 1))] : 0.0f);
          a = fma_(sDP[r * S + i], v, a);
        }
        accS[net.o_w1 + i * K + f] = a;
      } else if (t < nw + hd) {
        const int i = t - nw;
        float a = 0.0f, lo = 0.0f;
        for (int r = 0; r < E; ++r)
          if (outf[r]) add2(a, lo, sDP[r * S + i]);
        accS[net.o_b1 + i] = a;
        accC[net.o_b1 + i] = lo;
      } else {
        const int q = t - nw - hd;
        const int tt = q / ES, sc = q - tt * ES;
        float a = 0.0f, lo = 0.0f;
        for (int r = 0; r < E; ++r) {
          if (!outf[r] || ty[r] != tt) continue;
          float u = 0.0f;
          for (int i = 0; i < hd; ++i) u = fma_(w[net.o_w1 + i * K + F - 1 + sc], sDP[r * S + i], u);
          add2(a, lo, u);
        }
        accS[net.o_emb + q] = a;
        accC[net.o_emb + q] = lo;
      }
    }
  }
  LSM_SYNC();
}

// the slab's float64 accumulators take the group's graphs, ascending
LSM_HD void slab_add(const Emb& b, double* slab, const float* acc0, int64_t acc_stride, int nvalid, bool first, int wtid,
                     int wnt) {
  for (int t = wtid; t < b.n; t += wnt) {
    double a = first ? 0.0 : slab[t];
    for (int i = 0; i < nvalid; ++i) {
      const float* p = acc0 + i * acc_stride;
      a += (double)(p[t] + p[b.n4 + t]);
    }
    slab[t] = a;
  }
}

template <int HP>
__global__ __launch_bounds__(BLOCK) void gnn_embed_backward_kernel(Emb b) {
  extern __shared__ float4 lds4[];
  const Net& net = b.net;
  float* lds0 = reinterpret_cast<float*>(lds4);
  const int team = (int)threadIdx.x >> net.ts_shift;
  const int tid = (int)threadIdx.x & (net.TS - 1);
  const int64_t first_g = (int64_t)blockIdx.x * SLAB;
  const int64_t left = net.B - first_g;
  const int count = left < SLAB ? (int)left : SLAB;   // the slab's graphs: uniform in the workgroup
  double* slab = b.ws + (int64_t)blockIdx.x * b.n;
  float* acc0 = b.acc_lds ? lds0 + b.o_acc : b.wsacc + (int64_t)blockIdx.x * net.G * 2 * b.n4;
  const int64_t acc_stride = b.acc_lds ? net.per_graph : 2 * b.n4;
  EdgeState<(HP ? HP : MAX_DIM)> state;
  for (int at = 0; at < count; at += net.G) {
    const bool live = at + team < count;
    const int64_t g = live ? first_g + at + team : net.B - 1;
    const int nvalid = count - at < net.G ? count - at : net.G;
    graph_embed_backward<HP>(b, g, tid, net.TS, lds0 + (int64_t)team * net.per_graph, acc0 + team * acc_stride, live,
                             &state);
    slab_add(b, slab, acc0, acc_stride, nvalid, at == 0, (int)threadIdx.x, (int)blockDim.x);
    __syncthreads();
  }
}

// dembed: the slabs' partials added in ascending order
__global__ __launch_bounds__(BLOCK) void gnn_embed_backward_reduce(Emb b) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= b.n) return;
  double a = 0.0;
  for (int64_t s = 0; s < b.slabs; ++s) a += b.ws[s * b.n + t];
  b.dembed[t] = (float)a;
}

thread_local char g_err[320];

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "gnn embed backward: %s", msg);
  return 1;
}

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

size_t ws_bytes(const Emb& b) {
  return (size_t)b.slabs * ((size_t)b.n * 8 + (b.acc_lds ? 0 : (size_t)b.net.G * 2 * b.n4 * 4));
}

// the config's and the sizes' checks and the launch plan (plan: no pointer is looked at, masked standing for
// masks != NULL); 0 when fine
int make_emb(const lsm_gnn_config& c, const float* weights, const lsm_gnn_embed_bwd_io* io, bool plan, bool masked,
             int64_t B, int32_t E, int32_t N, Emb* b) {
  Net* n = &b->net;
  const char* why = "";
  const size_t total = gnn_layout(c, n, &why);
  if (total == 0) return fail(why);
  if (!plan && !io) return fail("io is null");
  if (!plan) masked = io->masks != nullptr;
  if (!plan && !weights) return fail("weights is null");
  if (B < 0) return fail("B < 0");
  if (B > INT32_MAX) return fail("B exceeds INT32_MAX graphs; split the batch");
  if (E < 1 || E > 256) return fail("E must be in [1, 256]");
  if (masked && (N < 1 || B % N != 0)) return fail("compact layout: B must be a multiple of N > 0");
  n->B = B;
  n->E = E;
  n->N = masked ? N : 1;
  n->W = (E + 63) / 64;
  n->SA = n->SK = 0;
  b->S = pad(n->Hd);
  b->n = n->o_conv[0];
  b->n4 = (b->n + 3) & ~3;
  b->slabs = (B + SLAB - 1) / SLAB;
  const int E4 = (E + 3) & ~3, EE4 = (E * E + 3) & ~3, ES6 = E * b->S;
  const int64_t base = 6 * (int64_t)ES6 + 4 * E4;
  if (base * 4 > LDS_BYTES) {
    char text[220];
    snprintf(text, sizeof text,
             "E = %d nodes need %lld bytes of LDS per graph (%d per node and 16 per four nodes), a workgroup has %d "
             "(see lsm_gnn_embed_backward.h)",
             E, (long long)(base * 4), 6 * b->S * 4, LDS_BYTES);
    return fail(text);
  }
  int ts = 32, sh = 5;
  while (ts < E) ts *= 2, ++sh;
  n->TS = ts;
  n->ts_shift = sh;
  int G = BLOCK / ts;
  const int fit = (int)(LDS_BYTES / (base * 4));
  if (G > fit) G = fit;
  n->G = G;
  n->adj_lds = (int64_t)G * (base + EE4) * 4 <= LDS_BYTES;
  const int64_t with_adj = base + (n->adj_lds ? EE4 : 0);
  b->acc_lds = (int64_t)G * (with_adj + 2 * b->n4) * 4 <= LDS_BYTES;
  b->o_dh = ES6;
  b->o_dp = 2 * ES6;
  b->o_d = 3 * ES6;
  b->o_n = 4 * ES6;
  b->o_x = 5 * ES6;
  b->o_dis = 6 * ES6;
  b->o_ty = b->o_dis + E4;
  b->o_out = b->o_ty + E4;
  b->o_e = b->o_out + E4;
  b->o_adjT = b->o_e + E4;
  b->o_acc = (int32_t)with_adj;
  n->per_graph = (int32_t)(with_adj + (b->acc_lds ? 2 * b->n4 : 0));
  if (plan) return 0;

  if (!io->dembed || !io->workspace) return fail("dembed / workspace is null");
  if (B > 0 && (!io->node_obs || !io->adj || !io->dh0)) return fail("node_obs / adj / dh0 is null");
  if (((uintptr_t)weights & 3) || ((uintptr_t)io->node_obs & 3) || ((uintptr_t)io->adj & 3) ||
      ((uintptr_t)io->dh0 & 3) || ((uintptr_t)io->dembed & 3) || ((uintptr_t)io->masks & 7) ||
      ((uintptr_t)io->bad & 7) || ((uintptr_t)io->workspace & 7))
    return fail("misaligned pointer");
  {
    const size_t nB = (size_t)B;
    const void* in[5] = {weights, io->node_obs, io->adj, io->masks, io->dh0};
    const size_t in_n[5] = {total * 4, nB * E * n->F * 4, (nB / n->N) * E * E * 4, masked ? nB * n->W * 8 : 0,
                            nB * E * n->Hd * 4};
    const void* out[3] = {io->dembed, io->workspace, io->bad};
    const size_t out_n[3] = {(size_t)b->n * 4, ws_bytes(*b), 8};
    for (int i = 0; i < 3; ++i) {
      for (int k = 0; k < 5; ++k)
        if (overlap(out[i], out_n[i], in[k], in_n[k])) return fail("an output overlaps an input");
      for (int k = i + 1; k < 3; ++k)
        if (overlap(out[i], out_n[i], out[k], out_n[k])) return fail("two outputs overlap");
    }
  }
  n->w = weights;
  n->x = io->node_obs;
  n->adj = io->adj;
  n->masks = io->masks;
  n->agent = nullptr;
  n->out = nullptr;
  n->bad = io->bad;
  b->dh0 = io->dh0;
  b->dembed = io->dembed;
  b->ws = static_cast<double*>(io->workspace);
  b->wsacc = reinterpret_cast<float*>(b->ws + b->slabs * b->n);
  return 0;
}

bool fast(const Net& n) { return n.Hd == 16; }

size_t lds_bytes(const Net& n) { return (size_t)n.G * n.per_graph * sizeof(float); }

template <int HP>
void host_run(const Emb& b) {
  const Net& net = b.net;
  std::vector<float4> scratch((size_t)net.per_graph / 4 + 1), accv((size_t)b.n4 / 2 + 1);
  std::vector<EdgeState<(HP ? HP : MAX_DIM)>> states((size_t)net.E);
  float* lds = reinterpret_cast<float*>(scratch.data());
  float* acc = reinterpret_cast<float*>(accv.data());
  for (int64_t g = 0; g < net.B; ++g) {
    graph_embed_backward<HP>(b, g, 0, 1, lds, acc, true, states.data());
    slab_add(b, b.ws + (g / SLAB) * b.n, acc, 0, 1, g % SLAB == 0, 0, 1);
  }
  for (int t = 0; t < b.n; ++t) {
    double a = 0.0;
    for (int64_t s = 0; s < b.slabs; ++s) a += b.ws[s * b.n + t];
    b.dembed[t] = (float)a;
  }
}

}  // namespace

extern "C" {

const char* lsm_gnn_embed_backward_last_error(void) { return g_err; }

size_t lsm_gnn_embed_floats(lsm_gnn_config cfg) {
  Net n;
  const char* why = "";
  if (gnn_layout(cfg, &n, &why) == 0) {
    fail(why);
    return 0;
  }
  return (size_t)n.o_conv[0];
}

size_t lsm_gnn_embed_backward_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E) {
  Emb b;
  if (make_emb(cfg, nullptr, nullptr, true, false, B, E, 1, &b)) return 0;
  return ws_bytes(b);
}

int lsm_gnn_embed_backward_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked,
                                lsm_gnn_embed_bwd_launch_plan* out) {
  Emb b;
  if (!out) return fail("plan: out is null");
  if (make_emb(cfg, nullptr, nullptr, true, masked != 0, B, E, N, &b)) return 1;
  out->TS = b.net.TS;
  out->G = b.net.G;
  out->fast = fast(b.net);
  out->adj_lds = b.net.adj_lds;
  out->acc_lds = b.acc_lds;
  out->S = b.S;
  out->per_graph = b.net.per_graph;
  out->entries = b.n;
  out->lds_bytes = (int64_t)lds_bytes(b.net);
  out->slabs = b.slabs;
  out->ws_bytes = (int64_t)ws_bytes(b);
  return 0;
}

int lsm_gnn_embed_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_embed_bwd_io* io, int64_t B,
                           int32_t E, int32_t N, void* hip_stream) {
  Emb b;
  if (make_emb(cfg, weights, io, false, false, B, E, N, &b)) return 1;
  if (B == 0) return 0;
  const size_t lds = lds_bytes(b.net);
  const dim3 grid((unsigned)b.slabs), block((unsigned)(b.net.G * b.net.TS));
  auto kernel = fast(b.net) ? gnn_embed_backward_kernel<16> : gnn_embed_backward_kernel<0>;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail("could not reserve the workgroup's LDS");
  kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(b);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  gnn_embed_backward_reduce<<<dim3((unsigned)((b.n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)hip_stream>>>(b);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_host_gnn_embed_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_embed_bwd_io* io, int64_t B,
                                int32_t E, int32_t N) {
  Emb b;
  if (make_emb(cfg, weights, io, false, false, B, E, N, &b)) return 1;
  if (B == 0) return 0;
  // a team of one lane and one graph at a time: its accumulators are the host's own
  b.net.G = 1;
  if (fast(b.net)) host_run<16>(b);
  else host_run<0>(b);
  return 0;
}

}  // extern "C"
