// lsm_gnn.hip -- the forward pass of the reference's graph encoder in one launch (include/lsm_gnn.h).
//
// Reference: GNNBase.forward (onpolicy/algorithms/utils/gnn.py:545-564) runs process_adj, then EmbedConv
// (gnn.py:21-148), gnn_layer_N + 1 torch_geometric TransformerConv layers (gnn.py:246-290) and the
// readout, on an edge list: per-edge gathers of [nnz, hidden] and [nnz, H * C] tensors and atomic
// scatters. Here a graph never leaves its workgroup: node_obs and the adjacency (either layout, the
// compact one expanded on the fly by a select) are read once, every activation lives in LDS, and the
// only thing written is the [out_dim] row.
//
// Work split. A team of TS lanes owns one graph, TS the power of two >= E (at least 32); a 256-thread
// workgroup packs G = 256 / TS graphs (fewer when their LDS does not fit), so a 24-node graph takes half
// a wave and not a whole group. Lane c of a team owns node c in every phase:
//   0   dis[c] (the compact layout's disconnect bit), P_c = lin1's node part W . [x_c, emb_c] + b (only
//       the e column of lin1 depends on the edge); then the team stages the expanded adjacency in LDS
//   1   EmbedConv: lane c walks its incoming edges r = 0 .. E-1, runs the per-edge MLP in registers
//       (m = act(P_r + e * w_e), layer norm, the embed layers) and sums into h0_c
//   2   per conv layer: (a) k_c, v_c; (b) q_c per head, then the incoming edges of c with an online
//       softmax (running max, one exp per edge), the head merge, lin_skip and the activation
//   3   readout
// with a workgroup barrier between phases (every team runs the same phase sequence: the loops are
// bounded by E and the config alone; a team past B recomputes graph B - 1 and writes nothing).
// Each target's reduction is sequential in one lane, sources ascending: no atomics, no cross-lane
// reduction, bit-reproducible. The logit is split as (<q_c, k_r> + e <q_c, w_e>) / sqrt(C) and the
// output as (sum p v_r + (sum p e) w_e) / (sum p + 1e-16), so an edge costs 2 C FMAs per head.
// Reading lane-uniform weights through the scalar cache, the FMAs take them as scalar operands.
//
// LDS per graph (floats): two activation buffers [E][SA] (ping-pong), k and v [E][SK] (P lives in k
// during phase 1), dis [E], and the adjacency [E][E] when it fits. Row strides are padded to
// round_up(w, 4) + 4 floats: 16-byte aligned rows for 16-byte reads, and lane c's row c * stride does
// not land every lane on the same banks (stride 16 or 48 would: 4 distinct bank groups for 64 lanes).
//
// Two instances: <16, 16> (embed_hidden == 16 and C == 16, the reference's sizes: the per-edge vectors
// are register arrays, every loop over them unrolled) and <0, 0> (any size up to 64, runtime loops).
// graph_forward is ONE __host__ __device__ text; lsm_host_gnn_forward runs it with a team of one lane.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/lsm_gnn.h"
#include "lsm_gnn_tile.h"   // graph_forward and its helpers, shared with lsm_gnn_backward.hip

namespace {

template <int HP, int CP>
__global__ __launch_bounds__(BLOCK) void gnn_kernel(Net net) {
  extern __shared__ float4 lds4[];
  const int team = (int)threadIdx.x >> net.ts_shift;
  const int tid = (int)threadIdx.x & (net.TS - 1);
  int64_t g = (int64_t)blockIdx.x * net.G + team;
  const bool write = g < net.B;
  if (!write) g = net.B - 1;   // keeps the workgroup's barriers uniform; nothing is written
  graph_forward<HP, CP>(net, g, tid, net.TS, reinterpret_cast<float*>(lds4) + (int64_t)team * net.per_graph, write);
}

thread_local char g_err[256];

int fail(const char* msg) {
  snprintf(g_err, sizeof g_err, "gnn: %s", msg);
  return 1;
}

// the config's checks and the blob's offsets (lsm_gnn_tile.h); returns the blob's length in floats, 0 with a text on refusal
size_t layout(const lsm_gnn_config& c, Net* n) {
  const char* why = "";
  const size_t floats = gnn_layout(c, n, &why);
  if (floats == 0) fail(why);
  return floats;
}

// every check of one call, shared by the device and the host entry point; fills n; 0 when fine
int make_net(const lsm_gnn_config& c, const float* weights, const float* node_obs, const float* adj,
             const uint64_t* masks, int64_t B, int32_t E, int32_t N, const int64_t* agent_id, float* out,
             int64_t* bad, Net* n, int plan_masked = -1) {
  // lsm_gnn_plan: plan_masked >= 0 stands for masks != NULL, and the pointers are neither given nor checked
  const bool plan = plan_masked >= 0;
  const bool masked = plan ? plan_masked != 0 : masks != nullptr;
  if (layout(c, n) == 0) return 1;
  if (!plan && !weights) return fail("weights is null");
  if (B < 0) return fail("B < 0");
  if (B > INT32_MAX) return fail("B exceeds INT32_MAX graphs; split the batch");
  if (E < 1 || E > 256) return fail("E must be in [1, 256]");
  if (masked && (N < 1 || B % N != 0)) return fail("compact layout: B must be a multiple of N > 0");
  if (!plan && B > 0 && (!node_obs || !adj || !out)) return fail("node_obs / adj / out is null");
  if (!plan && c.aggr == LSM_GNN_NODE && !agent_id) return fail("node aggregation needs agent_id");
  if (((uintptr_t)weights & 3) || ((uintptr_t)node_obs & 3) || ((uintptr_t)adj & 3) || ((uintptr_t)out & 3) ||
      ((uintptr_t)masks & 7) || ((uintptr_t)agent_id & 7) || ((uintptr_t)bad & 7))
    return fail("misaligned pointer");
  n->w = weights;
  n->x = node_obs;
  n->adj = adj;
  n->masks = masks;
  n->agent = agent_id;
  n->out = out;
  n->bad = bad;
  n->B = B;
  n->E = E;
  n->N = masked ? N : 1;
  n->W = (E + 63) / 64;
  n->SA = pad(n->Hd > n->D ? n->Hd : n->D);
  n->SK = pad(n->Hd > n->HC ? n->Hd : n->HC);
  const int act = E * (2 * n->SA + 2 * n->SK) + ((E + 3) & ~3);
  if ((int64_t)act * 4 > LDS_BYTES) return fail("E * layer widths exceed the LDS of one workgroup (see lsm_gnn.h)");
  const int with_adj = act + ((E * E + 3) & ~3);
  n->adj_lds = (int64_t)with_adj * 4 <= LDS_BYTES;
  n->per_graph = n->adj_lds ? with_adj : act;
  int ts = 32, sh = 5;
  while (ts < E) ts *= 2, ++sh;
  n->TS = ts;
  n->ts_shift = sh;
  int G = BLOCK / ts;
  const int fit = LDS_BYTES / (n->per_graph * 4);
  if (G > fit) G = fit;
  n->G = G;
  return 0;
}

bool fast(const Net& n) { return n.Hd == 16 && n.C == 16; }

// the workgroup's dynamic LDS
size_t lds_bytes(const Net& n) { return (size_t)n.G * n.per_graph * sizeof(float); }

}  // namespace

extern "C" {

const char* lsm_gnn_last_error(void) { return g_err; }

size_t lsm_gnn_weights_floats(lsm_gnn_config cfg) {
  Net n;
  return layout(cfg, &n);
}

int lsm_gnn_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked, lsm_gnn_launch_plan* out) {
  Net n;
  if (!out) return fail("plan: out is null");
  if (make_net(cfg, nullptr, nullptr, nullptr, nullptr, B, E, N, nullptr, nullptr, nullptr, &n, masked != 0)) return 1;
  out->TS = n.TS;
  out->G = n.G;
  out->adj_lds = n.adj_lds;
  out->fast = fast(n);
  out->SA = n.SA;
  out->SK = n.SK;
  out->lds_bytes = (int64_t)lds_bytes(n);
  return 0;
}

int lsm_gnn_forward(lsm_gnn_config cfg, const float* weights, const float* node_obs, const float* adj,
                    const uint64_t* masks, int64_t B, int32_t E, int32_t N, const int64_t* agent_id, float* out,
                    int64_t* bad, void* hip_stream) {
  Net n;
  if (make_net(cfg, weights, node_obs, adj, masks, B, E, N, agent_id, out, bad, &n)) return 1;
  if (B == 0) return 0;
  const size_t lds = lds_bytes(n);
  const dim3 grid((unsigned)((B + n.G - 1) / n.G)), block((unsigned)(n.G * n.TS));
  auto kernel = fast(n) ? gnn_kernel<16, 16> : gnn_kernel<0, 0>;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return fail("could not reserve the workgroup's LDS");
  kernel<<<grid, block, lds, (hipStream_t)hip_stream>>>(n);
  return hipGetLastError() == hipSuccess ? 0 : fail("launch failed");
}

int lsm_host_gnn_forward(lsm_gnn_config cfg, const float* weights, const float* node_obs, const float* adj,
                         const uint64_t* masks, int64_t B, int32_t E, int32_t N, const int64_t* agent_id, float* out,
                         int64_t* bad) {
  Net n;
  if (make_net(cfg, weights, node_obs, adj, masks, B, E, N, agent_id, out, bad, &n)) return 1;
  std::vector<float4> scratch((size_t)n.per_graph / 4 + 1);
  for (int64_t g = 0; g < B; ++g) {
    if (fast(n)) graph_forward<16, 16>(n, g, 0, 1, reinterpret_cast<float*>(scratch.data()), true);
    else graph_forward<0, 0>(n, g, 0, 1, reinterpret_cast<float*>(scratch.data()), true);
  }
  return 0;
}

}  // extern "C"
