// lsm_gnn_tile.h -- the graph encoder's per-graph forward text and what it needs, shared by the forward
// unit (lsm_gnn.hip) and the backward unit (lsm_gnn_backward.hip), which recomputes the forward with a save
// hook. Everything here has internal linkage: each unit compiles its own copy.
//
// graph_forward is ONE __host__ __device__ text: lanes tid = 0 .. nt-1 of a team run one graph, lane c owns
// node c in every phase, every activation lives in the team's LDS region (layout: lsm_gnn.hip's comment).
// The Saves hook is called by the lane that owns node c, with what the backward pass needs per node:
//   row(l, c, p, n)            p[0..n) = h_l of node c: l = 0 EmbedConv's output, l + 1 conv layer l's output
//   stat(l, c, hh, mx, inv)    conv layer l, head hh: the running maximum of the logits of c's incoming edges
//                              and 1 / (den + 1e-16) (-inf and 0 for a target without an incoming edge)
// NoSaves, the default, compiles to nothing.
#ifndef LSM_GNN_TILE_H
#define LSM_GNN_TILE_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/lsm_gnn.h"

// the <0, 0> instance's loops have runtime bounds: their "#pragma unroll" is meant for <16, 16>
#pragma clang diagnostic ignored "-Wpass-failed"

namespace {

#define LSM_HD __host__ __device__ __forceinline__
#if defined(__HIP_DEVICE_COMPILE__)
#define LSM_SYNC() __syncthreads()
#else
#define LSM_SYNC() ((void)0)
#endif

constexpr int LDS_BYTES = 163840;   // one workgroup may use all of a CU's LDS
constexpr int BLOCK = 256;
constexpr int MAX_DIM = 64;         // embed_hidden, C
constexpr int MAX_LAYERS = 4;

struct Net {
  const float* w;
  const float* x;
  const float* adj;
  const uint64_t* masks;
  const int64_t* agent;
  float* out;
  int64_t* bad;
  int64_t B;
  int32_t E, F, NE, ES, Hd, EL, C, H, HC, D, L, K, N, W;
  int32_t relu_e, ln, relu_g, concat, aggr, ego_only;
  int32_t SA, SK;          // padded row strides of the activation and the k / v buffers
  int32_t per_graph;       // LDS floats per graph
  int32_t adj_lds;         // the adjacency is staged in LDS
  int32_t TS, ts_shift, G; // team size (a power of two), its log2, graphs per workgroup
  int32_t o_emb, o_w1, o_b1, o_gamma, o_beta, o_el, o_conv[MAX_LAYERS + 1];
  float inv_sqrt_c;
};

struct NoSaves {
  LSM_HD void row(int, int, const float*, int) const {}
  LSM_HD void stat(int, int, int, float, float) const {}
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

// The activation over a vector, ReLU (as torch's: NaN stays NaN) or Tanh. The choice is lane-uniform and
// made once per vector, around the loop: as a per-element select the compiler evaluates tanhf for every
// element of a ReLU net too (some fifty instructions each, several times the per-edge FMAs).
LSM_HD void act_n(float* m, int n, int relu) {
  if (relu) {
#pragma unroll
    for (int i = 0; i < n; ++i) m[i] = m[i] < 0.0f ? 0.0f : m[i];
  } else {
#pragma unroll
    for (int i = 0; i < n; ++i) m[i] = tanhf(m[i]);
  }
}

// acc + <w[0..n), row[0..n)>, row a 16-byte aligned LDS row
LSM_HD float dotw(const float* __restrict__ w, const float* row, int n, float acc) {
  int i = 0;
  for (; i + 4 <= n; i += 4) {
    const float4 h = *reinterpret_cast<const float4*>(row + i);
    acc = fma_(w[i], h.x, acc);
    acc = fma_(w[i + 1], h.y, acc);
    acc = fma_(w[i + 2], h.z, acc);
    acc = fma_(w[i + 3], h.w, acc);
  }
  for (; i < n; ++i) acc = fma_(w[i], row[i], acc);
  return acc;
}

// the shared nn.LayerNorm(n): biased variance, eps 1e-5
template <int NN>
LSM_HD void layer_norm(float (&m)[NN], int n, const float* __restrict__ gamma, const float* __restrict__ beta) {
  float s = 0.0f;
#pragma unroll
  for (int i = 0; i < n; ++i) s += m[i];
  const float mean = s / (float)n;
  float q = 0.0f;
#pragma unroll
  for (int i = 0; i < n; ++i) {
    const float d = m[i] - mean;
    q = fma_(d, d, q);
  }
  const float rs = rsq_(q / (float)n + 1e-5f);
#pragma unroll
  for (int i = 0; i < n; ++i) m[i] = fma_((m[i] - mean) * rs, gamma[i], beta[i]);
}

// the graph's entry [r][c] for a lane that knows dis[c] (disc); sAdj, dis, ag, E and net are the caller's
#define LSM_ADJ(r, c, disc) (net.adj_lds ? sAdj[(r) * E + (c)] : ((dis[r] | (disc)) ? 0.0f : ag[(r) * E + (c)]))

// One graph, run by lanes tid = 0 .. nt-1 of its team (nt >= E on the device, 1 on the host).
// HP / CP: embed_hidden / C as compile-time sizes, or 0 for runtime sizes up to MAX_DIM.
template <int HP, int CP, class Saves = NoSaves>
LSM_HD void graph_forward(const Net& net, int64_t g, int tid, int nt, float* lds, bool write,
                          const Saves& sv = Saves()) {
  constexpr int HN = HP ? HP : MAX_DIM;
  constexpr int CN = CP ? CP : MAX_DIM;
  const int E = net.E, F = net.F, K = net.K, SA = net.SA, SK = net.SK, H = net.H, HC = net.HC, D = net.D;
  const int hd = HP ? HP : net.Hd;
  const int cc = CP ? CP : net.C;
  const float* __restrict__ w = net.w;
  float* bufA = lds;
  float* bufB = bufA + E * SA;
  float* sK = bufB + E * SA;
  float* sV = sK + E * SK;
  int32_t* dis = reinterpret_cast<int32_t*>(sV + E * SK);
  float* sAdj = reinterpret_cast<float*>(dis) + ((E + 3) & ~3);
  const float* ag = net.adj + (net.masks ? g / net.N : g) * ((int64_t)E * E);
  const float* xg = net.x + g * ((int64_t)E * F);

  // ---- phase 0: disconnect bits and lin1's node part P (in the k buffer) ----------------------------
  for (int r = tid; r < E; r += nt) {
    dis[r] = net.masks ? (int32_t)((net.masks[g * net.W + (r >> 6)] >> (r & 63)) & 1ull) : 0;
    const float* xr = xg + (int64_t)r * F;
    const float t = xr[F - 1];
    const bool okt = t > -1.0f && t < (float)net.NE;   // trunc(t) in [0, NE); NaN and inf fail
    const int ti = okt ? (int)t : 0;
    if (!okt && net.bad) *net.bad = 1;
    float* P = sK + r * SK;
    for (int i = 0; i < hd; ++i) {
      const float* wi = w + net.o_w1 + i * K;
      float a = w[net.o_b1 + i];
      for (int f = 0; f < F - 1; ++f) a = fma_(wi[f], xr[f], a);
      if (okt)
        for (int s = 0; s < net.ES; ++s) a = fma_(wi[F - 1 + s], w[net.o_emb + ti * net.ES + s], a);
      P[i] = a;
    }
  }
  LSM_SYNC();
  if (net.adj_lds) {
    for (int k = tid; k < E * E; k += nt) {
      const int r = k / E, c = k - r * E;
      const float v = ag[k];
      sAdj[k] = (dis[r] | dis[c]) ? 0.0f : v;
    }
    LSM_SYNC();
  }

  // ---- phase 1: EmbedConv, aggr = add -----------------------------------------------------------------
  for (int c = tid; c < E; c += nt) {
    const int disc = dis[c];
    float h0[HN];
#pragma unroll
    for (int i = 0; i < hd; ++i) h0[i] = 0.0f;
    for (int r = 0; r < E; ++r) {
      const float e = LSM_ADJ(r, c, disc);
      if (e == 0.0f) continue;   // NaN is an edge, -0.0 is not
      const float* P = sK + r * SK;
      float m[HN], t[HN];
#pragma unroll
      for (int i = 0; i < hd; ++i) m[i] = fma_(e, w[net.o_w1 + i * K + K - 1], P[i]);
      act_n(m, hd, net.relu_e);
      if (net.ln) layer_norm<HN>(m, hd, w + net.o_gamma, w + net.o_beta);
      for (int k = 0; k < net.EL; ++k) {
        const float* wl = w + net.o_el + k * (hd * hd + hd);
#pragma unroll
        for (int j = 0; j < hd; ++j) {
          float a = wl[hd * hd + j];
#pragma unroll
          for (int i = 0; i < hd; ++i) a = fma_(wl[j * hd + i], m[i], a);
          t[j] = a;
        }
#pragma unroll
        for (int j = 0; j < hd; ++j) m[j] = t[j];
        act_n(m, hd, net.relu_e);
        if (net.ln) layer_norm<HN>(m, hd, w + net.o_gamma, w + net.o_beta);
      }
#pragma unroll
      for (int i = 0; i < hd; ++i) h0[i] += m[i];
    }
#pragma unroll
    for (int i = 0; i < hd; ++i) bufA[c * SA + i] = h0[i];
    sv.row(0, c, bufA + c * SA, hd);
  }
  LSM_SYNC();

  // the ego node: read once, range-checked; no address is formed from a bad one
  int ego = -1;
  if (net.aggr == LSM_GNN_NODE) {
    const int64_t id = net.agent[g];
    if (id >= 0 && id < E) ego = (int)id;
  }

  // ---- phase 2: TransformerConv layers ----------------------------------------------------------------
  float* cur = bufA;
  float* nxt = bufB;
  for (int l = 0; l <= net.L; ++l) {
    const int Din = l == 0 ? net.Hd : D;
    const float* wq = w + net.o_conv[l];
    const float* bq = wq + HC * Din;
    const float* wk = bq + HC;
    const float* bk = wk + HC * Din;
    const float* wv = bk + HC;
    const float* bv = wv + HC * Din;
    const float* we = bv + HC;
    const float* ws = we + HC;
    const float* bs = ws + D * Din;
    // (a) keys and values of every node
    for (int n = tid; n < E; n += nt) {
      const float* row = cur + n * SA;
      for (int j = 0; j < HC; ++j) {
        sK[n * SK + j] = dotw(wk + j * Din, row, Din, bk[j]);
        sV[n * SK + j] = dotw(wv + j * Din, row, Din, bv[j]);
      }
    }
    LSM_SYNC();
    // (b) attention over the incoming edges of c, head merge, root term, activation
    const bool only_ego = net.ego_only && l == net.L && net.aggr == LSM_GNN_NODE;
    for (int c = tid; c < E; c += nt) {
      if (only_ego && c != ego) continue;
      const int disc = dis[c];
      const float* row = cur + c * SA;
      float* o = nxt + c * SA;
      for (int hh = 0; hh < H; ++hh) {
        float q[CN], acc[CN];
        float qe = 0.0f;
#pragma unroll
        for (int j = 0; j < cc; ++j) {
          q[j] = dotw(wq + (hh * cc + j) * Din, row, Din, bq[hh * cc + j]);
          qe = fma_(q[j], we[hh * cc + j], qe);
          acc[j] = 0.0f;
        }
        float mx = -INFINITY, den = 0.0f, se = 0.0f;
        bool any = false;
        for (int r = 0; r < E; ++r) {
          const float e = LSM_ADJ(r, c, disc);
          if (e == 0.0f) continue;
          any = true;
          const float* kr = sK + r * SK + hh * cc;
          const float* vr = sV + r * SK + hh * cc;
          float dot = 0.0f;
#pragma unroll
          for (int j = 0; j < cc; ++j) dot = fma_(q[j], kr[j], dot);
          const float a = fma_(e, qe, dot) * net.inv_sqrt_c;
          float p;
          if (a > mx) {   // a new running maximum: rescale what has been summed
            const float s = expf(mx - a);
            den *= s;
            se *= s;
#pragma unroll
            for (int j = 0; j < cc; ++j) acc[j] *= s;
            mx = a;
            p = 1.0f;
          } else {
            p = expf(a - mx);
          }
          den += p;
          se = fma_(p, e, se);
#pragma unroll
          for (int j = 0; j < cc; ++j) acc[j] = fma_(p, vr[j], acc[j]);
        }
        const float inv = any ? 1.0f / (den + 1e-16f) : 0.0f;
        sv.stat(l, c, hh, mx, inv);
#pragma unroll
        for (int j = 0; j < cc; ++j) {
          const float v = any ? fma_(se, we[hh * cc + j], acc[j]) * inv : 0.0f;
          if (net.concat) o[hh * cc + j] = v;
          else o[j] = hh == 0 ? v : o[j] + v;
        }
      }
      for (int j = 0; j < D; ++j) {
        const float merged = net.concat ? o[j] : o[j] / (float)H;
        o[j] = merged + dotw(ws + j * Din, row, Din, bs[j]);
      }
      act_n(o, D, net.relu_g);
      sv.row(l + 1, c, o, D);
    }
    LSM_SYNC();
    float* t = cur;
    cur = nxt;
    nxt = t;
  }

  // ---- phase 3: readout ---------------------------------------------------------------------------------
  if (!write) return;
  float* og = net.out + g * (int64_t)D;
  if (net.aggr == LSM_GNN_NODE) {
    if (ego < 0 && tid == 0 && net.bad) *net.bad = 1;
    for (int j = tid; j < D; j += nt) og[j] = ego >= 0 ? cur[ego * SA + j] : 0.0f;
    return;
  }
  for (int j = tid; j < D; j += nt) {
    float a = cur[j];
    for (int n = 1; n < E; ++n) {
      const float v = cur[n * SA + j];
      if (net.aggr == LSM_GNN_GLOBAL_MAX) a = (v > a || v != v) ? v : a;
      else a += v;
    }
    og[j] = net.aggr == LSM_GNN_GLOBAL_MEAN ? a / (float)E : a;
  }
}

inline int pad(int w) { return ((w + 3) & ~3) + 4; }

inline bool in_range(int v, int lo, int hi) { return v >= lo && v <= hi; }

// the config's checks and the blob's offsets; returns the blob's length in floats, or 0 with *why the reason
inline size_t gnn_layout(const lsm_gnn_config& c, Net* n, const char** why) {
#define LSM_REFUSE(text) return *why = (text), (size_t)0
  if (!in_range(c.F, 2, 64)) LSM_REFUSE("F must be in [2, 64]");
  if (!in_range(c.num_embeddings, 1, 64) || !in_range(c.embedding_size, 1, 64))
    LSM_REFUSE("num_embeddings and embedding_size must be in [1, 64]");
  if (!in_range(c.embed_hidden, 1, MAX_DIM) || !in_range(c.C, 1, MAX_DIM)) LSM_REFUSE("embed_hidden and C must be in [1, 64]");
  if (!in_range(c.H, 1, 4)) LSM_REFUSE("H must be in [1, 4]");
  if (c.H * c.C > 256) LSM_REFUSE("H * C must be <= 256");
  if (!in_range(c.embed_layer_N, 0, MAX_LAYERS) || !in_range(c.layer_N, 0, MAX_LAYERS))
    LSM_REFUSE("embed_layer_N and layer_N must be in [0, 4]");
  if (!in_range(c.aggr, LSM_GNN_NODE, LSM_GNN_GLOBAL_ADD)) LSM_REFUSE("unknown aggregation");
#undef LSM_REFUSE
  n->F = c.F;
  n->NE = c.num_embeddings;
  n->ES = c.embedding_size;
  n->Hd = c.embed_hidden;
  n->EL = c.embed_layer_N;
  n->C = c.C;
  n->H = c.H;
  n->HC = c.H * c.C;
  n->D = c.concat ? n->HC : c.C;
  n->L = c.layer_N;
  n->K = c.F - 1 + c.embedding_size + 1;
  n->relu_e = c.embed_relu != 0;
  n->ln = c.layer_norm != 0;
  n->relu_g = c.relu != 0;
  n->concat = c.concat != 0;
  n->aggr = c.aggr;
  n->ego_only = c.ego_only != 0;
  n->inv_sqrt_c = 1.0f / sqrtf((float)c.C);
  int o = 0;
  n->o_emb = o, o += n->NE * n->ES;
  n->o_w1 = o, o += n->Hd * n->K;
  n->o_b1 = o, o += n->Hd;
  n->o_gamma = o, o += n->Hd;
  n->o_beta = o, o += n->Hd;
  n->o_el = o, o += n->EL * (n->Hd * n->Hd + n->Hd);
  for (int l = 0; l <= MAX_LAYERS; ++l) {
    n->o_conv[l] = o;
    if (l > n->L) continue;
    const int Din = l == 0 ? n->Hd : n->D;
    o += 3 * (n->HC * Din + n->HC) + n->HC + n->D * Din + n->D;
  }
  return (size_t)o;
}

}  // namespace

#endif
