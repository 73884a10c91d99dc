// lsm_gnn_backward.hip -- the backward pass through the graph encoder's readout and TransformerConv layers
// (include/lsm_gnn_backward.h states the formulas and the sum order): from dout to the gradient of every
// conv-layer weight and to dh0, the gradient at EmbedConv's output.
//
// Ownership is the forward's (lsm_gnn.hip): a team of TS lanes per graph, lane c owns node c, G graphs per
// workgroup, phases separated by workgroup barriers. One workgroup owns one slab of LSM_GNN_BWD_SLAB graphs and
// walks it G graphs at a time, so that the slab's float64 accumulators (its own row of the workspace) take
// the graphs' terms in ascending order without atomics. Per group of G graphs:
//   F   graph_forward (lsm_gnn_tile.h, the forward's own text) with a save hook: every layer's input rows and
//       per (node, head) the running maximum and 1 / (den + 1e-16)
//   R   the readout's gradient dY, lane c its own row
//   per layer l = L .. 0:
//   0   lane c: g_c = dY_c act'(y_c) in place, dO_c (a copy / H under the mean), q_c, k_c, v_c
//   1   the target pass: lane c walks its incoming edges twice (s_c, sum alpha e; then dq_c, sum da e)
//   2   the source pass: lane r walks its outgoing edges, recomputes a, alpha, da and sums dk_r, dv_r in
//       registers, then writes them over its own k_r, v_r (no other lane reads those rows in this pass)
//   3   the weight terms: the workgroup's threads split the layer's entries; per entry and graph an FMA chain
//       over the nodes, added to the slab's float64 accumulator in graph order
//   4   lane c: dh_c = W_q^T dq_c + W_k^T dk_c + W_v^T dv_c + W_s^T g_c, the next dY (after layer 0: dh0)
// A second kernel adds the slabs' partials in float64 and writes dweights (0 over the EmbedConv entries).
//
// LDS per graph: graph_forward's own region (two activation buffers, reused for dY and dO; k, v; dis; the
// adjacency), then the transposed adjacency (lane r's outgoing edges at stride 1 across lanes), the saved rows
// h_0 .. h_{L+1}, q, dq and the statistics [E][ST] (ST odd: lane c's row does not share a bank group).
// Teams past the slab's end recompute graph B - 1 and write nothing.
//
// The spilled tier (include/lsm_gnn_backward_large.h) is the same per-graph text with a compile-time level SP:
// level 0 is the layout above; levels 1 .. 4 move the saved rows, dq, the statistics and q, in that order, out
// of LDS into the workgroup's own scratch in the workspace (one region per team, after the slab accumulators),
// so that only graph_forward's region has to fit. Which base a region hangs from is decided at compile time:
// every access keeps a known address space. A team writes and reads its own scratch region; the weight phase
// reads the regions of the workgroup's other teams. The __syncthreads() between the phases, which already
// orders one lane's LDS stores before another lane's loads, is also what orders one lane's global stores to the
// scratch before another lane's loads of them: it waits for the workgroup's outstanding stores and fences at
// workgroup scope, and a workgroup's lanes share one L1. Nothing is read across workgroups. Teams past the
// slab's end recompute graph B - 1 into their own scratch region.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_gnn_backward.h"
#include "../../include/lsm_gnn_backward_large.h"
#include "lsm_gnn_tile.h"

namespace {

constexpr int SLAB = LSM_GNN_BWD_SLAB;

struct Bwd {
  Net net;              // the forward's view (ego_only off, out unused)
  const float* dout;
  float* dh0;
  float* dweights;
  double* ws;           // [slabs][nconv]
  int32_t ST;           // the statistics' row stride
  int32_t o_adjT, o_H, o_Q, o_DQ, o_st;   // float offsets inside a graph's LDS region (a spilled one's: inside its scratch region)
  int32_t conv0, nconv; // the blob's first conv entry and the number of conv entries
  int32_t total;        // the blob's length
  int64_t slabs;
};

// the spilled tier's launch: the level-0 view, the scratch after the slab accumulators and a team's floats in it
struct BwdLarge {
  Bwd b;
  float* scratch;       // [slabs][G][spilled]
  int32_t spilled;
};

// the base a region hangs from at level SP: the team's LDS region, or its scratch region from level AT on
template <int SP, int AT>
LSM_HD float* region(float* lds, float* sp) {
  if constexpr (SP >= AT) return sp;
  else return lds;
}
template <int SP, int AT>
LSM_HD const float* region(const float* lds, const float* sp) {
  if constexpr (SP >= AT) return sp;
  else return lds;
}

// graph_forward's save hook: lane c keeps its own rows
struct Saver {
  float* Hs;
  float* st;
  int E, SA, ST, H;
  LSM_HD void row(int l, int c, const float* p, int n) const {
    float* d = Hs + (l * E + c) * SA;
    for (int i = 0; i < n; ++i) d[i] = p[i];
  }
  LSM_HD void stat(int l, int c, int hh, float mx, float inv) const {
    float* s = st + c * ST + (l * H + hh) * 2;
    s[0] = mx;
    s[1] = inv;
  }
};

// s += x with the addition's rounding collected in c (two-sum): a vector entry's terms may cancel to far below
// their size (sum_r da_rc is 0 up to rounding, so the key bias's gradient is), and a plain chain's roundings,
// each of the size of a partial sum, would then be the whole result
LSM_HD void add2(float& s, float& c, float x) {
  const float t = s + x;
  const float b = t - s;
  c += (s - (t - b)) + (x - b);
  s = t;
}

// A bias's (t >= nout * Din) or a matrix entry's chain over the nodes, delta [E][stride] against h [E][SA]
LSM_HD float entry_chain(const float* delta, int stride, const float* hl, int E, int SA, int Din, int nout, int t) {
  float a = 0.0f;
  if (t >= nout * Din) {
    const int j = t - nout * Din;
    float lo = 0.0f;
    for (int n = 0; n < E; ++n) add2(a, lo, delta[n * stride + j]);
    a += lo;
  } else {
    const int j = t / Din, i = t - j * Din;
    for (int n = 0; n < E; ++n) a = fma_(delta[n * stride + j], hl[n * SA + i], a);
  }
  return a;
}

// One entry's term of one graph: the FMA chain over the nodes (include/lsm_gnn_backward.h, "within a graph").
// t indexes conv layer l's entries in the blob's order. sp: the graph's scratch region (levels 1 .. 4).
template <int SP>
LSM_HD float weight_term(const Bwd& b, const float* lds, const float* sp, const float* dcur, const float* dO, int l,
                         int Din, int t) {
  const Net& net = b.net;
  const int E = net.E, SA = net.SA, SK = net.SK, HC = net.HC, D = net.D, H = net.H;
  const float* hl = region<SP, 1>(lds, sp) + b.o_H + l * E * SA;
  const int nW = HC * Din;
  int m = 0;   // 0 query, 1 key, 2 value (weight [HC][Din], bias [HC] each), 3 what follows them
  for (; m < 3 && t >= nW + HC; ++m) t -= nW + HC;
  // (every arm an LDS address: from level 2 on the first one is not used, see below)
  const float* delta = m == 0 ? lds + b.o_DQ : m == 1 ? lds + 2 * E * SA : m == 2 ? lds + 2 * E * SA + E * SK : dcur;
  const int stride = m < 3 ? SK : SA;
  int nout = HC;
  if (m == 3) {
    if (t < HC) {   // the edge weight: targets ascending
      const int hh = t / net.C;
      const float* sQ = region<SP, 4>(lds, sp) + b.o_Q;
      const float* st = region<SP, 3>(lds, sp) + b.o_st + 2 * H * (net.L + 1) + 5 * hh;
      const int jo = net.concat ? t : t - hh * net.C;
      float a = 0.0f, lo = 0.0f;
      for (int c = 0; c < E; ++c) {
        const float* sc = st + c * b.ST;
        add2(a, lo, fma_(dO[c * SA + jo], sc[1], sQ[c * SK + t] * net.inv_sqrt_c * sc[2]));
      }
      return a + lo;
    }
    t -= HC;   // lin_skip: weight [D][Din], bias [D], delta = g
    nout = D;
  }
  // from level 2 on dq is in the scratch and k, v, g are in LDS: the query entries take a branch of their own
  // (the same chain), so that no load's base is chosen between the two at run time
  if constexpr (SP >= 2) {
    if (m == 0) return entry_chain(sp + b.o_DQ, stride, hl, E, SA, Din, nout, t);
  }
  return entry_chain(delta, stride, hl, E, SA, Din, nout, t);
}

// One graph of one group: lanes tid = 0 .. nt-1 of its team (1 on the host). live: the team's graph exists
// (g is B - 1 otherwise and nothing is written). The weight phase is the workgroup's: thread wtid of wnt adds
// the terms of the group's first nvalid graphs (regions lds0 + i * per_graph) to acc[], from 0 when first.
// SP: the spill level; from level 1 on sp is the team's scratch region and sp0 + i * sp_stride graph i's.
template <int HP, int CP, int SP = 0>
LSM_HD void graph_backward(const Bwd& b, int64_t g, int tid, int nt, float* lds, bool live, int wtid, int wnt,
                           float* lds0, int nvalid, double* acc, bool first, float* sp = nullptr,
                           float* sp0 = nullptr, int sp_stride = 0) {
  constexpr int CN = CP ? CP : MAX_DIM;
  const Net& net = b.net;
  const int E = net.E, SA = net.SA, SK = net.SK, H = net.H, HC = net.HC, D = net.D, L = net.L, ST = b.ST;
  const int cc = CP ? CP : net.C;
  const float* __restrict__ w = net.w;
  float* bufA = lds;
  float* bufB = bufA + E * SA;
  float* sK = bufB + E * SA;
  float* sV = sK + E * SK;
  const int32_t* dis = reinterpret_cast<const int32_t*>(sV + E * SK);
  const float* sAdj = reinterpret_cast<const float*>(dis) + ((E + 3) & ~3);
  float* sAdjT = lds + b.o_adjT;
  float* Hs = region<SP, 1>(lds, sp) + b.o_H;
  float* sQ = region<SP, 4>(lds, sp) + b.o_Q;
  float* sDQ = region<SP, 2>(lds, sp) + b.o_DQ;
  float* st = region<SP, 3>(lds, sp) + b.o_st;
  const float* ag = net.adj + (net.masks ? g / net.N : g) * ((int64_t)E * E);
  const int cur0 = 2 * H * (L + 1);   // the current layer's statistics inside a row

  // ---- F: the forward, with saves --------------------------------------------------------------------------
  const Saver sv{Hs, st, E, SA, ST, H};
  graph_forward<HP, CP, Saver>(net, g, tid, nt, lds, false, sv);
  if (net.adj_lds)
    for (int k = tid; k < E * E; k += nt) {
      const int r = k / E, c = k - r * E;
      sAdjT[c * E + r] = sAdj[k];
    }

  // ---- R: the readout's gradient -----------------------------------------------------------------------------
  int ego = -1;
  if (net.aggr == LSM_GNN_NODE) {
    const int64_t id = net.agent[g];
    if (id >= 0 && id < E) ego = (int)id;
    else if (live && tid == 0 && net.bad) *net.bad = 1;
  }
  float* dcur = bufA;
  float* dnxt = bufB;
  {
    const float* yL = Hs + (L + 1) * E * SA;
    const float* dout = b.dout + g * (int64_t)D;
    for (int c = tid; c < E; c += nt) {
      float* d = dcur + c * SA;
      for (int j = 0; j < D; ++j) {
        float v;
        if (net.aggr == LSM_GNN_NODE) {
          v = c == ego ? dout[j] : 0.0f;
        } else if (net.aggr == LSM_GNN_GLOBAL_MAX) {
          float a = yL[j];
          int win = 0;
          for (int n = 1; n < E; ++n) {
            const float y = yL[n * SA + j];
            if (y > a || y != y) a = y, win = n;
          }
          v = win == c ? dout[j] : 0.0f;
        } else {
          v = net.aggr == LSM_GNN_GLOBAL_MEAN ? dout[j] / (float)E : dout[j];
        }
        d[j] = v;
      }
    }
  }

  for (int l = L; l >= 0; --l) {
    const int Din = l == 0 ? net.Hd : D;
    const float* wq = w + net.o_conv[l];
    const float* bq = wq + HC * Din;
    const float* wk = bq + HC;
    const float* bk = wk + HC * Din;
    const float* wv = bk + HC;
    const float* bv = wv + HC * Din;
    const float* we = bv + HC;
    const float* ws = we + HC;
    const float* hl = Hs + l * E * SA;
    const float* yl = Hs + (l + 1) * E * SA;
    // dO: g's own rows under concat, a copy divided by H under the mean
    const float* dO = net.concat ? dcur : dnxt;

    // ---- 0: g, dO, q, k, v per node --------------------------------------------------------------------------
    for (int c = tid; c < E; c += nt) {
      float* d = dcur + c * SA;
      const float* y = yl + c * SA;
      if (net.relu_g) {
        for (int j = 0; j < D; ++j) d[j] = y[j] <= 0.0f ? 0.0f : d[j];
      } else {
        for (int j = 0; j < D; ++j) d[j] *= 1.0f - y[j] * y[j];
      }
      if (!net.concat)
        for (int j = 0; j < D; ++j) dnxt[c * SA + j] = d[j] / (float)H;
      const float* row = hl + c * SA;
      for (int j = 0; j < HC; ++j) {
        sQ[c * SK + j] = dotw(wq + j * Din, row, Din, bq[j]);
        sK[c * SK + j] = dotw(wk + j * Din, row, Din, bk[j]);
        sV[c * SK + j] = dotw(wv + j * Din, row, Din, bv[j]);
      }
    }
    LSM_SYNC();

    // ---- 1: the target pass ----------------------------------------------------------------------------------
    for (int c = tid; c < E; c += nt) {
      const int disc = dis[c];
      for (int hh = 0; hh < H; ++hh) {
        float q[CN], o[CN], dq[CN];
        float qe = 0.0f, oe = 0.0f;
        const float* qrow = sQ + c * SK + hh * cc;
        const float* orow = dO + c * SA + (net.concat ? hh * cc : 0);
#pragma unroll
        for (int j = 0; j < cc; ++j) {
          q[j] = qrow[j];
          o[j] = orow[j];
          qe = fma_(q[j], we[hh * cc + j], qe);
          oe = fma_(o[j], we[hh * cc + j], oe);
          dq[j] = 0.0f;
        }
        float* sc = st + c * ST;
        // the forward's maximum; the denominator is summed again, of exp(a - max) against the final maximum (the
        // forward's own den carries the roundings of its rescales, and sum_r alpha_rc would miss 1 by them)
        const float mx = sc[(l * H + hh) * 2];
        float den = 0.0f;
        double den2 = 0.0, spd = 0.0, spe = 0.0, sde = 0.0;
        bool any = false;
        for (int r = 0; r < E; ++r) {
          const float e = LSM_ADJ(r, c, disc);
          if (e == 0.0f) continue;
          any = true;
          const float* kr = sK + r * SK + hh * cc;
          const float* vr = sV + r * SK + hh * cc;
          float dot = 0.0f, ov = 0.0f;
#pragma unroll
          for (int j = 0; j < cc; ++j) {
            dot = fma_(q[j], kr[j], dot);
            ov = fma_(o[j], vr[j], ov);
          }
          const float p = expf(fma_(e, qe, dot) * net.inv_sqrt_c - mx);
          den += p;
          den2 += (double)p;
          spd += (double)p * (double)fma_(e, oe, ov);
          spe += (double)p * (double)e;
        }
        const float inv = any ? 1.0f / (den + 1e-16f) : 0.0f;
        const float s = any ? (float)(spd / (den2 + 1e-16)) : 0.0f, sae = any ? (float)(spe / (den2 + 1e-16)) : 0.0f;
        sc[(l * H + hh) * 2 + 1] = inv;
        for (int r = 0; r < E; ++r) {
          const float e = LSM_ADJ(r, c, disc);
          if (e == 0.0f) continue;
          const float* kr = sK + r * SK + hh * cc;
          const float* vr = sV + r * SK + hh * cc;
          float dot = 0.0f, ov = 0.0f;
#pragma unroll
          for (int j = 0; j < cc; ++j) {
            dot = fma_(q[j], kr[j], dot);
            ov = fma_(o[j], vr[j], ov);
          }
          const float al = expf(fma_(e, qe, dot) * net.inv_sqrt_c - mx) * inv;
          const float da = al * (fma_(e, oe, ov) - s);
          sde += (double)da * (double)e;
#pragma unroll
          for (int j = 0; j < cc; ++j) dq[j] = fma_(da, kr[j], dq[j]);
        }
        float* dqrow = sDQ + c * SK + hh * cc;
#pragma unroll
        for (int j = 0; j < cc; ++j) dqrow[j] = fma_((float)sde, we[hh * cc + j], dq[j]) * net.inv_sqrt_c;
        float* cs = sc + cur0 + 5 * hh;
        cs[0] = s;
        cs[1] = sae;
        cs[2] = (float)sde;
        cs[3] = qe;
        cs[4] = oe;
      }
    }
    LSM_SYNC();

    // ---- 2: the source pass ----------------------------------------------------------------------------------
    for (int r = tid; r < E; r += nt) {
      const int disr = dis[r];
      for (int hh = 0; hh < H; ++hh) {
        float kr[CN], vr[CN], dk[CN], dv[CN];
        float* krow = sK + r * SK + hh * cc;
        float* vrow = sV + r * SK + hh * cc;
#pragma unroll
        for (int j = 0; j < cc; ++j) {
          kr[j] = krow[j];
          vr[j] = vrow[j];
          dk[j] = 0.0f;
          dv[j] = 0.0f;
        }
        for (int c = 0; c < E; ++c) {
          const float e = net.adj_lds ? sAdjT[c * E + r] : ((disr | dis[c]) ? 0.0f : ag[r * E + c]);
          if (e == 0.0f) continue;
          const float* sc = st + c * ST;
          const float mx = sc[(l * H + hh) * 2], inv = sc[(l * H + hh) * 2 + 1];
          const float* cs = sc + cur0 + 5 * hh;
          const float* qc = sQ + c * SK + hh * cc;
          const float* oc = dO + c * SA + (net.concat ? hh * cc : 0);
          float dot = 0.0f, ov = 0.0f;
#pragma unroll
          for (int j = 0; j < cc; ++j) {
            dot = fma_(qc[j], kr[j], dot);
            ov = fma_(oc[j], vr[j], ov);
          }
          const float al = expf(fma_(e, cs[3], dot) * net.inv_sqrt_c - mx) * inv;
          const float da = al * (fma_(e, cs[4], ov) - cs[0]);
#pragma unroll
          for (int j = 0; j < cc; ++j) {
            dv[j] = fma_(al, oc[j], dv[j]);
            dk[j] = fma_(da, qc[j], dk[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < cc; ++j) {
          krow[j] = dk[j] * net.inv_sqrt_c;
          vrow[j] = dv[j];
        }
      }
    }
    LSM_SYNC();

    // ---- 3: the layer's weight terms into the slab's accumulators -----------------------------------------------
    {
      const int nl = 3 * (HC * Din + HC) + HC + D * Din + D;
      double* al = acc + (net.o_conv[l] - b.conv0);
      const int off_cur = (int)(dcur - lds), off_dO = (int)(dO - lds);
      for (int t = wtid; t < nl; t += wnt) {
        double a = first ? 0.0 : al[t];
        for (int i = 0; i < nvalid; ++i) {
          const float* base = lds0 + (int64_t)i * net.per_graph;
          a += (double)weight_term<SP>(b, base, sp0 + (int64_t)i * sp_stride, base + off_cur, base + off_dO, l, Din, t);
        }
        al[t] = a;
      }
    }
    LSM_SYNC();

    // ---- 4: dh per node, 16 columns at a time ---------------------------------------------------------------------
    for (int c = tid; c < E; c += nt) {
      const float* dqr = sDQ + c * SK;
      const float* dkr = sK + c * SK;
      const float* dvr = sV + c * SK;
      const float* gr = dcur + c * SA;
      float* out = dnxt + c * SA;
      for (int i0 = 0; i0 < Din; i0 += 16) {
        float a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = 0.0f;
        const int ni = Din - i0 < 16 ? Din - i0 : 16;
        if (ni == 16) {
          for (int j = 0; j < HC; ++j) {
            const float x = dqr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = fma_(wq[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < HC; ++j) {
            const float x = dkr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = fma_(wk[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < HC; ++j) {
            const float x = dvr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = fma_(wv[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < D; ++j) {
            const float x = gr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = fma_(ws[j * Din + i0 + i], x, a[i]);
          }
        } else {
          for (int j = 0; j < HC; ++j) {
            const float x = dqr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (i < ni) a[i] = fma_(wq[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < HC; ++j) {
            const float x = dkr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (i < ni) a[i] = fma_(wk[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < HC; ++j) {
            const float x = dvr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (i < ni) a[i] = fma_(wv[j * Din + i0 + i], x, a[i]);
          }
          for (int j = 0; j < D; ++j) {
            const float x = gr[j];
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (i < ni) a[i] = fma_(ws[j * Din + i0 + i], x, a[i]);
          }
        }
#pragma unroll
        for (int i = 0; i < 16; ++i)
          if (i < ni) out[i0 + i] = a[i];
      }
      if (l == 0 && b.dh0 && live) {
        float* dst = b.dh0 + (g * E + c) * (int64_t)Din;
        for (int i = 0; i < Din; ++i) dst[i] = out[i];
      }
    }
    float* t = dcur;
    dcur = dnxt;
    dnxt = t;
  }
  LSM_SYNC();   // keeps the groups apart
}

template <int HP, int CP>
__global__ __launch_bounds__(BLOCK) void gnn_backward_kernel(Bwd b) {
  extern __shared__ float4 lds4[];
  const Net& net = b.net;
  float* lds0 = reinterpret_cast<float*>(lds4);
  const int team = (int)threadIdx.x >> net.ts_shift;
  const int tid = (int)threadIdx.x & (net.TS - 1);
  const int64_t first_g = (int64_t)blockIdx.x * SLAB;
  const int64_t left = net.B - first_g;
  const int count = left < SLAB ? (int)left : SLAB;   // the slab's graphs: uniform in the workgroup
  double* acc = b.ws + (int64_t)blockIdx.x * b.nconv;
  for (int at = 0; at < count; at += net.G) {
    const bool live = at + team < count;
    const int64_t g = live ? first_g + at + team : net.B - 1;
    const int nvalid = count - at < net.G ? count - at : net.G;
    graph_backward<HP, CP>(b, g, tid, net.TS, lds0 + (int64_t)team * net.per_graph, live, (int)threadIdx.x,
                           (int)blockDim.x, lds0, nvalid, acc, at == 0);
  }
}

// The spilled tier, SP = 1 .. 4: the same walk; team i of workgroup s owns scratch region s * G + i.
template <int HP, int CP, int SP>
__global__ __launch_bounds__(BLOCK) void gnn_backward_large_kernel(BwdLarge a) {
  extern __shared__ float4 lds4[];
  const Bwd& b = a.b;
  const Net& net = b.net;
  float* lds0 = reinterpret_cast<float*>(lds4);
  const int team = (int)threadIdx.x >> net.ts_shift;
  const int tid = (int)threadIdx.x & (net.TS - 1);
  const int64_t first_g = (int64_t)blockIdx.x * SLAB;
  const int64_t left = net.B - first_g;
  const int count = left < SLAB ? (int)left : SLAB;
  double* acc = b.ws + (int64_t)blockIdx.x * b.nconv;
  float* sp0 = a.scratch + (int64_t)blockIdx.x * net.G * a.spilled;
  for (int at = 0; at < count; at += net.G) {
    const bool live = at + team < count;
    const int64_t g = live ? first_g + at + team : net.B - 1;
    const int nvalid = count - at < net.G ? count - at : net.G;
    graph_backward<HP, CP, SP>(b, g, tid, net.TS, lds0 + (int64_t)team * net.per_graph, live, (int)threadIdx.x,
                               (int)blockDim.x, lds0, nvalid, acc, at == 0, sp0 + (int64_t)team * a.spilled, sp0,
                               a.spilled);
  }
}

// dweights: 0 over the EmbedConv entries, the slabs' partials added in ascending order over the conv entries
__global__ __launch_bounds__(BLOCK) void gnn_backward_reduce(Bwd b) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= b.total) return;
  double a = 0.0;
  if (t >= b.conv0)
    for (int64_t s = 0; s < b.slabs; ++s) a += b.ws[s * b.nconv + (t - b.conv0)];
  b.dweights[t] = (float)a;
}

thread_local char g_err[320];
thread_local char g_err_large[320];
thread_local bool g_large;   // the running entry point is lsm_gnn_backward_large.h's: its own text and prefix

int fail(const char* msg) {
  if (g_large) snprintf(g_err_large, sizeof g_err_large, "gnn backward large: %s", msg);
  else snprintf(g_err, sizeof g_err, "gnn backward: %s", msg);
  return 1;
}

// which sizes make_bwd accepts and where the five regions go
constexpr int TIER_LDS = -1;    // lsm_gnn_backward.h: level 0 or a refusal
constexpr int TIER_HOST = -2;   // the host entry points of the large header: level 0's layout, no LDS to fit
                                // (0 .. 4: the large header's min_spill)
struct Tier {
  int32_t spill;            // the level
  int32_t spilled;          // floats per graph in the scratch, a multiple of 4
  int64_t acc_bytes;        // the slab accumulators
  int64_t scratch_bytes;    // the scratch behind them, with the 8 bytes that align its start to 16
};

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  if (!a || !b || na == 0 || nb == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + nb && y < x + na;
}

// the config's and the sizes' checks and the launch plan (io == nullptr: lsm_gnn_backward_plan and
// lsm_gnn_backward_workspace_bytes, masked standing for masks != NULL); 0 when fine. tier: TIER_LDS, TIER_HOST
// or the large header's min_spill; *t is what was chosen.
int make_bwd(const lsm_gnn_config& c, const float* weights, const lsm_gnn_bwd_io* io, bool plan, bool masked,
             int64_t B, int32_t E, int32_t N, Bwd* b, int tier = TIER_LDS, Tier* t = nullptr) {
  Net* n = &b->net;
  const char* why = "";
  const size_t total = gnn_layout(c, n, &why);
  if (total == 0) return fail(why);
  if (tier > 4 || tier < TIER_HOST) return fail("min_spill must be in [0, 4]");
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
  n->ego_only = 0;
  n->SA = pad(n->Hd > n->D ? n->Hd : n->D);
  n->SK = pad(n->Hd > n->HC ? n->Hd : n->HC);
  b->ST = (2 * n->H * (n->L + 1) + 5 * n->H) | 1;
  b->conv0 = n->o_conv[0];
  b->nconv = (int32_t)total - b->conv0;
  b->total = (int32_t)total;
  b->slabs = (B + SLAB - 1) / SLAB;
  const int E4 = (E + 3) & ~3, EE4 = (E * E + 3) & ~3;
  // the LDS floats of a graph at level s: graph_forward's region and what the level keeps beside it
  const auto kept = [&](int s) {
    return (int64_t)E * (2 * n->SA + 2 * n->SK + (s < 1 ? (n->L + 2) * n->SA : 0) + (s < 2 ? n->SK : 0) +
                         (s < 3 ? b->ST : 0) + (s < 4 ? n->SK : 0)) + E4;
  };
  int spill = tier > 0 ? tier : 0;
  if (tier == TIER_LDS) {
    const int64_t base = kept(0);
    if (base * 4 > LDS_BYTES) {
      char text[200];
      snprintf(text, sizeof text,
               "E = %d nodes need %lld bytes of LDS per graph (%lld per node), a workgroup has %d (see lsm_gnn_backward.h)",
               E, (long long)(base * 4), (long long)((base - E4) * 4 / E), LDS_BYTES);
      return fail(text);
    }
  } else {
    if (kept(4) * 4 > LDS_BYTES) {   // lsm_gnn_forward's own limit
      char text[240];
      snprintf(text, sizeof text,
               "E = %d nodes need %lld bytes of LDS per graph for the forward's region alone (%lld per node), a "
               "workgroup has %d: lsm_gnn_forward refuses this size too (see lsm_gnn.h)",
               E, (long long)(kept(4) * 4), (long long)((kept(4) - E4) * 4 / E), LDS_BYTES);
      return fail(text);
    }
    if (tier != TIER_HOST)
      while (kept(spill) * 4 > LDS_BYTES) ++spill;   // ends at 4 at the latest
  }
  const int64_t base = kept(spill);
  n->adj_lds = (base + 2 * EE4) * 4 <= LDS_BYTES;
  const int fwd = E * (2 * n->SA + 2 * n->SK) + E4 + (n->adj_lds ? EE4 : 0);
  b->o_adjT = fwd;
  // the five regions in one order, h, q, dq, st (the odd-sized one last: the others stay 16-byte aligned), each
  // behind the last one of its own space
  int o = fwd + (n->adj_lds ? EE4 : 0), q = 0;
  const auto place = [&](int at, int floats) {
    int& where = spill >= at ? q : o;
    const int r = where;
    where += floats;
    return r;
  };
  b->o_H = place(1, (n->L + 2) * E * n->SA);
  b->o_Q = place(4, E * n->SK);
  b->o_DQ = place(2, E * n->SK);
  b->o_st = place(3, E * b->ST);
  n->per_graph = (o + 3) & ~3;
  int ts = 32, sh = 5;
  while (ts < E) ts *= 2, ++sh;
  n->TS = ts;
  n->ts_shift = sh;
  int G = BLOCK / ts;
  const int fit = LDS_BYTES / (n->per_graph * 4);
  if (G > fit) G = fit;
  if (tier == TIER_HOST && G < 1) G = 1;   // host memory: one graph at a time, whatever its size
  if (G < 1) return fail("a graph's LDS region does not fit");   // per_graph's rounding: not reached
  n->G = G;
  Tier tt;
  tt.spill = spill;
  tt.spilled = (q + 3) & ~3;
  tt.acc_bytes = b->slabs * b->nconv * (int64_t)sizeof(double);
  tt.scratch_bytes = spill && B > 0 ? b->slabs * G * tt.spilled * (int64_t)sizeof(float) + 8 : 0;
  if (t) *t = tt;
  if (plan) return 0;

  if (!io->dweights || !io->workspace) return fail("dweights / workspace is null");
  if (B > 0 && (!io->node_obs || !io->adj || !io->dout)) return fail("node_obs / adj / dout is null");
  if (c.aggr == LSM_GNN_NODE && !io->agent_id) return fail("node aggregation needs agent_id");
  if (((uintptr_t)weights & 3) || ((uintptr_t)io->node_obs & 3) || ((uintptr_t)io->adj & 3) ||
      ((uintptr_t)io->dout & 3) || ((uintptr_t)io->dweights & 3) || ((uintptr_t)io->dh0 & 3) ||
      ((uintptr_t)io->masks & 7) || ((uintptr_t)io->agent_id & 7) || ((uintptr_t)io->bad & 7) ||
      ((uintptr_t)io->workspace & 7))
    return fail("misaligned pointer");
  {
    const size_t nB = (size_t)B;
    const void* in[6] = {weights, io->node_obs, io->adj, io->masks, io->agent_id, io->dout};
    const size_t in_n[6] = {total * 4, nB * E * n->F * 4, (nB / n->N) * E * E * 4, masked ? nB * n->W * 8 : 0, nB * 8,
                            nB * n->D * 4};
    const void* out[4] = {io->dweights, io->dh0, io->workspace, io->bad};
    const size_t out_n[4] = {total * 4, nB * E * n->Hd * 4, (size_t)(tt.acc_bytes + tt.scratch_bytes), 8};
    for (int i = 0; i < 4; ++i) {
      for (int k = 0; k < 6; ++k)
        if (overlap(out[i], out_n[i], in[k], in_n[k])) return fail("an output overlaps an input");
      for (int k = i + 1; k < 4; ++k)
        if (overlap(out[i], out_n[i], out[k], out_n[k])) return fail("two outputs overlap");
    }
  }
  n->w = weights;
  n->x = io->node_obs;
  n->adj = io->adj;
  n->masks = io->masks;
  n->agent = io->agent_id;
  n->out = nullptr;
  n->bad = io->bad;
  b->dout = io->dout;
  b->dh0 = io->dh0;
  b->dweights = io->dweights;
  b->ws = static_cast<double*>(io->workspace);
  return 0;
}

bool fast(const Net& n) { return n.Hd == 16 && n.C == 16; }

size_t lds_bytes(const Net& n) { return (size_t)n.G * n.per_graph * sizeof(float); }

// lsm_gnn_backward's two launches, and lsm_gnn_backward_large's at level 0
int launch_level0(const Bwd& b, void* hip_stream) {
  const size_t lds = lds_bytes(b.net);
  const dim3 grid((unsigned)b.slabs), block((unsigned)(b.net.G * b.net.TS));
  auto kernel = fast(b.net) ? gnn_backward_kernel<16, 16> : gnn_backward_kernel<0, 0>;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail("could not reserve the workgroup's LDS");
  kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(b);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  gnn_backward_reduce<<<dim3((unsigned)((b.total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)hip_stream>>>(b);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

// the host entry points' walk: a team of one lane, the level-0 layout in host memory
void host_backward(const Bwd& b) {
  const int64_t B = b.net.B;
  std::vector<float4> scratch((size_t)b.net.per_graph / 4 + 1);
  float* lds = reinterpret_cast<float*>(scratch.data());
  for (int64_t g = 0; g < B; ++g) {
    double* acc = b.ws + (g / SLAB) * b.nconv;
    if (fast(b.net)) graph_backward<16, 16>(b, g, 0, 1, lds, true, 0, 1, lds, 1, acc, g % SLAB == 0);
    else graph_backward<0, 0>(b, g, 0, 1, lds, true, 0, 1, lds, 1, acc, g % SLAB == 0);
  }
  for (int t = 0; t < b.total; ++t) {
    double a = 0.0;
    if (t >= b.conv0)
      for (int64_t s = 0; s < b.slabs; ++s) a += b.ws[s * b.nconv + (t - b.conv0)];
    b.dweights[t] = (float)a;
  }
}

}  // namespace

extern "C" {

const char* lsm_gnn_backward_last_error(void) { return g_err; }

size_t lsm_gnn_backward_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E) {
  g_large = false;
  Bwd b;
  if (make_bwd(cfg, nullptr, nullptr, true, false, B, E, 1, &b)) return 0;
  return (size_t)b.slabs * b.nconv * sizeof(double);
}

int lsm_gnn_backward_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked,
                          lsm_gnn_bwd_launch_plan* out) {
  g_large = false;
  Bwd b;
  if (!out) return fail("plan: out is null");
  if (make_bwd(cfg, nullptr, nullptr, true, masked != 0, B, E, N, &b)) return 1;
  out->TS = b.net.TS;
  out->G = b.net.G;
  out->fast = fast(b.net);
  out->adj_lds = b.net.adj_lds;
  out->acc_lds = 0;
  out->SA = b.net.SA;
  out->SK = b.net.SK;
  out->ST = b.ST;
  out->lds_bytes = (int64_t)lds_bytes(b.net);
  out->slabs = b.slabs;
  out->ws_bytes = b.slabs * b.nconv * (int64_t)sizeof(double);
  return 0;
}

int lsm_gnn_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B, int32_t E, int32_t N,
                     void* hip_stream) {
  g_large = false;
  Bwd b;
  if (make_bwd(cfg, weights, io, false, false, B, E, N, &b)) return 1;
  if (B == 0) return 0;
  return launch_level0(b, hip_stream);
}

int lsm_host_gnn_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B, int32_t E,
                          int32_t N) {
  g_large = false;
  Bwd b;
  if (make_bwd(cfg, weights, io, false, false, B, E, N, &b)) return 1;
  if (B == 0) return 0;
  host_backward(b);
  return 0;
}

// ---- include/lsm_gnn_backward_large.h ------------------------------------------------------------------------------

const char* lsm_gnn_backward_large_last_error(void) { return g_err_large; }

size_t lsm_gnn_backward_large_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t min_spill) {
  g_large = true;
  Bwd b;
  Tier t;
  if (min_spill < 0) return fail("min_spill must be in [0, 4]"), (size_t)0;
  if (make_bwd(cfg, nullptr, nullptr, true, false, B, E, 1, &b, min_spill, &t)) return 0;
  return (size_t)(t.acc_bytes + t.scratch_bytes);
}

int lsm_gnn_backward_large_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked, int32_t min_spill,
                                lsm_gnn_bwd_large_launch_plan* out) {
  g_large = true;
  Bwd b;
  Tier t;
  if (!out) return fail("plan: out is null");
  if (min_spill < 0) return fail("min_spill must be in [0, 4]");
  if (make_bwd(cfg, nullptr, nullptr, true, masked != 0, B, E, N, &b, min_spill, &t)) return 1;
  out->TS = b.net.TS;
  out->G = b.net.G;
  out->fast = fast(b.net);
  out->adj_lds = b.net.adj_lds;
  out->acc_lds = 0;
  out->SA = b.net.SA;
  out->SK = b.net.SK;
  out->ST = b.ST;
  out->spill = t.spill;
  out->spilled_floats = t.spilled;
  out->lds_bytes = (int64_t)lds_bytes(b.net);
  out->slabs = b.slabs;
  out->ws_bytes = t.acc_bytes + t.scratch_bytes;
  out->scratch_bytes = t.scratch_bytes;
  return 0;
}

int lsm_gnn_backward_large(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B, int32_t E,
                           int32_t N, int32_t min_spill, void* hip_stream) {
  g_large = true;
  Bwd b;
  Tier t;
  if (min_spill < 0) return fail("min_spill must be in [0, 4]");
  if (make_bwd(cfg, weights, io, false, false, B, E, N, &b, min_spill, &t)) return 1;
  if (B == 0) return 0;
  if (t.spill == 0) return launch_level0(b, hip_stream);
  BwdLarge a;
  a.b = b;
  a.scratch = reinterpret_cast<float*>(((uintptr_t)io->workspace + (uintptr_t)t.acc_bytes + 15) & ~(uintptr_t)15);
  a.spilled = t.spilled;
  using Kernel = void (*)(BwdLarge);
  static const Kernel table[2][4] = {
      {gnn_backward_large_kernel<0, 0, 1>, gnn_backward_large_kernel<0, 0, 2>, gnn_backward_large_kernel<0, 0, 3>,
       gnn_backward_large_kernel<0, 0, 4>},
      {gnn_backward_large_kernel<16, 16, 1>, gnn_backward_large_kernel<16, 16, 2>, gnn_backward_large_kernel<16, 16, 3>,
       gnn_backward_large_kernel<16, 16, 4>}};
  const Kernel kernel = table[fast(b.net) ? 1 : 0][t.spill - 1];
  const size_t lds = lds_bytes(b.net);
  const dim3 grid((unsigned)b.slabs), block((unsigned)(b.net.G * b.net.TS));
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail("could not reserve the workgroup's LDS");
  kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(a);
  if (hipGetLastError() != hipSuccess) return fail("launch failed");
  gnn_backward_reduce<<<dim3((unsigned)((b.total + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, (hipStream_t)hip_stream>>>(b);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_host_gnn_backward_large(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B,
                                int32_t E, int32_t N) {
  g_large = true;
  Bwd b;
  if (make_bwd(cfg, weights, io, false, false, B, E, N, &b, TIER_HOST)) return 1;
  if (B == 0) return 0;
  host_backward(b);
  return 0;
}

}  // extern "C"
