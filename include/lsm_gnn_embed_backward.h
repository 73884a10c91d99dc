/*
 * lsm_gnn_embed_backward.h -- C ABI of EmbedConv's backward pass: from dh0, the gradient at EmbedConv's output
 * (lsm_gnn_backward.h ends there), to the gradient of the blob's EmbedConv entries: the entity embedding, lin1,
 * the shared LayerNorm and the embed layers, [0, lsm_gnn_embed_floats(cfg)) of the packed blob, in the blob's
 * own layout and order. The config, the blob, the two adjacency layouts, the edge set, the attribute e, the
 * disconnect bits and the entity-type rule are lsm_gnn.h's. The call needs (weights, node_obs, adj, dh0) only: it
 * does not run the conv layers. The gradient norm, the clipping and the optimiser are lsm_optim.h's.
 *
 * All arithmetic float32 unless stated. Per graph, with E nodes, Hd = embed_hidden, EL = embed_layer_N,
 * K = F - 1 + embedding_size + 1, x_r node r's features, t_r = trunc(x_r[F-1]) its entity type, emb the entity
 * embedding, w1 / b1 lin1, W_k / b_k embed layer k, gamma / beta the one shared LayerNorm:
 *
 * Forward, recomputed per edge r -> c (attribute e = e_rc) with the forward's own expressions:
 *     P_r     = b1 + w1[:, :F-1] x_r[:F-1] + w1[:, F-1 : F-1+ES] emb[t_r]     (lin1's node part: one FMA chain per
 *               output from the bias, the features ascending, then the embedding's columns ascending; a node
 *               with an invalid type has no embedding term)
 *     z_0     = fma(e, w1[:, K-1], P_r)
 *     a_k     = act(z_k)                              ReLU (a NaN stays NaN) or Tanh
 *     n_k     = LN(a_k) = fma(xh_k, gamma, beta), xh_k = (a_k - mean) * rstd, biased variance, eps 1e-5; n_k = a_k
 *               when layer_norm == 0
 *     z_{k+1} = W_k n_k + b_k, k = 0 .. EL-1          (an FMA chain per output from the bias, inputs ascending)
 *     m       = n_EL,  h0_c = sum of m over c's incoming edges
 * Backward, per edge, dn_EL = dh0_c, then for k = EL .. 0:
 *     through LayerNorm   ggamma += dn_k (.) xh_k,  gbeta += dn_k     (per edge: FMA / addition chains from 0 in
 *                         this order, k descending)
 *                         g = dn_k (.) gamma,  da_k = rstd * ((g - mean(g)) - xh_k * mean(g (.) xh_k)); both
 *                         means are chains over the columns ascending, divided by Hd
 *     through act         ReLU: dz_k = a_k <= 0 ? 0 : da_k (a NaN a_k passes da_k, as torch's); Tanh:
 *                         dz_k = da_k * (1 - a_k^2)
 *     through Linear      k > 0:  dW_{k-1} += dz_k (x) n_{k-1},  db_{k-1} += dz_k,
 *                                 dn_{k-1}[i] = sum_j W_{k-1}[j][i] dz_k[j]   (an FMA chain from 0, j ascending)
 *     at lin1 (k = 0)     dw1[:, K-1] += e * dz_0,  dP_r += dz_0,  dgamma += ggamma,  dbeta += gbeta
 * and then per node r that has an outgoing edge, with dP_r the sum of dz_0 over r's outgoing edges:
 *     dw1[:, :F-1] += dP_r (x) x_r[:F-1];  dw1[:, F-1 : F-1+ES] += dP_r (x) emb[t_r];  db1 += dP_r;
 *     d emb[t_r][s] += u_r[s],  u_r[s] = sum_i w1[i][F-1+s] dP_r[i]      (an FMA chain from 0, i ascending)
 * Rules that follow: a node with an invalid entity type contributes nothing to emb's gradient and a zero
 * embedding to lin1's columns, and sets *bad = 1; no address is formed from data (the type is range-checked
 * first, and emb's rows are matched by comparison). A node without an outgoing edge contributes nothing at all,
 * whatever its features; a target without an incoming edge contributes nothing, whatever its dh0 row. With
 * layer_norm == 0 the gamma and beta entries are written as 0. node_obs and adj are data: no gradient is taken
 * at them. Non-finite inputs give non-finite outputs and a clean finish.
 *
 * SUM ORDER (the contract; independent of the launch plan, the grid and the device):
 *   within a graph    entries fed per edge (dW_k, db_k, dw1[:, K-1], dgamma, dbeta): the edges in the order
 *                     targets c ascending and, within a target, sources r ascending. A matrix entry (dW_k) is one
 *                     float32 FMA chain from 0 in that order. A vector entry (db_k, dw1[:, K-1] whose term is the
 *                     rounded product e * dz_0, dgamma and dbeta whose terms are the edge's ggamma and gbeta) is
 *                     a chain of float32 additions in that order that also collects each addition's rounding
 *                     (two-sum) and adds their sum back at the end, as lsm_gnn_backward.h's vector entries.
 *                     dP_r is a plain float32 addition chain over r's outgoing edges, c ascending, in the lane that
 *                     owns r. Entries fed per node: nodes r ascending, skipping a node without an outgoing edge;
 *                     dw1's node columns are FMA chains from 0, db1 and emb's entries are two-sum chains (emb's
 *                     over the nodes of that type).
 *   within a slab     graphs are grouped into slabs of LSM_GNN_BWD_SLAB consecutive graphs; a slab's entry is a
 *                     float64 accumulator that starts at 0 and takes the per-graph float32 terms, graphs ascending.
 *   across slabs      the slabs' float64 partials are added in ascending order in float64, starting from 0, and
 *                     rounded to float32 once.
 * No atomics and no last-block-done counter: a call is bit-reproducible, and the host entry point runs the same
 * text with a team of one lane.
 *
 * Work split. One workgroup owns one slab and walks it G graphs at a time; a team of TS lanes (the power of two
 * >= E, at least 32) owns one graph and lane r owns SOURCE r. Per group: P_r and the graph's dh0 rows into LDS;
 * then the team walks the targets c = 0 .. E-1 uniformly: lane r, where the edge r -> c exists, recomputes the
 * MLP in registers and back-propagates, adding dz_0 to dP_r in its own LDS row; per Linear it stages its dz_k and
 * n_{k-1} rows (at lin1: dz_0, e, ggamma, gbeta) in LDS, a lane without that edge stages zeros in both, and after
 * a barrier the team's lanes split the layer's entries and run each entry's chain over the E rows into the
 * graph's float32 accumulators. (A zero row leaves a finite FMA chain and a finite two-sum chain from +0 unchanged
 * to the bit, so the E rows give the order above; a non-finite sum stays non-finite.) After the walk the node-fed entries follow, once per graph; then the
 * workgroup's threads add the group's graphs, ascending, into the slab's float64 accumulators. A second launch
 * adds the slabs' partials and writes dembed.
 *
 * LDS per graph, in floats, S = pad(embed_hidden), pad(w) = round_up(w, 4) + 4:
 *   E * 6 * S + 4 * round_up(E, 4)
 * (P, dh0, dP and three staged rows per node; per node the disconnect bit, the entity type, the outgoing-edge
 * flag and the staged e), plus round_up(E * E, 4) for the transposed adjacency, and then 2 * round_up(n, 4),
 * n = lsm_gnn_embed_floats(cfg), for the graph's float32 accumulators (sum and collected roundings), each when it
 * still fits in the 163840 bytes of a workgroup at the G the rest allows; otherwise the adjacency is read from
 * memory and the accumulators live in the workspace (the plan reports adj_lds and acc_lds). A size whose single
 * graph does not fit is refused, with the figures in the text (reference defaults: 480 bytes per node and 16 per
 * four nodes, every E <= 256 accepted; embed_hidden = 64: 1632 bytes per node, accepted up to E = 99). Every
 * (config, E) that lsm_gnn_backward accepts is accepted here: that call needs at least 8 rows of this width per
 * node. G = min(256 / TS, what fits in LDS without the two optional parts).
 *
 * Workspace: per slab one float64 row of n entries and, when acc_lds == 0, G rows of 2 * n floats:
 *   ceil(B / LSM_GNN_BWD_SLAB) * (8 * n + (acc_lds ? 0 : 8 * G * n)) bytes.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_gnn_embed_backward_last_error() (thread-local, prefix "gnn embed backward: "). Refused: lsm_gnn.h's limits
 * and the LDS need above; a null io, weights, dembed or workspace; with B > 0 a null node_obs, adj or dh0; the
 * compact layout with N < 1 or B % N != 0; B < 0 or B > INT32_MAX; misaligned pointers (4 bytes; masks, bad and
 * workspace: 8); an output (dembed, workspace, bad) overlapping an input or another output. B == 0 is legal and
 * writes nothing. lsm_gnn_embed_backward is stream-ordered and asynchronous: two launches, no host
 * synchronisation, no allocation.
 */
#ifndef LSM_GNN_EMBED_BACKWARD_H
#define LSM_GNN_EMBED_BACKWARD_H

#include <stddef.h>
#include <stdint.h>

#include "lsm_gnn.h"
#include "lsm_gnn_backward.h" /* LSM_GNN_BWD_SLAB */

#ifdef __cplusplus
extern "C" {
#endif

/* The number of EmbedConv entries of the blob = the blob offset of conv layer 0's query weight; 0 for a config
 * outside lsm_gnn.h's limits. */
size_t lsm_gnn_embed_floats(lsm_gnn_config cfg);

/* One call's tensors: device pointers for lsm_gnn_embed_backward, host pointers for the host entry point. */
typedef struct lsm_gnn_embed_bwd_io {
  const float* node_obs;   /* [B][E][F] */
  const float* adj;        /* either layout, as lsm_gnn_forward */
  const uint64_t* masks;   /* NULL = reference layout */
  const float* dh0;        /* [B][E][embed_hidden]: INPUT, the gradient at EmbedConv's output */
  float* dembed;           /* [lsm_gnn_embed_floats(cfg)], the blob's own layout and order, overwritten */
  void* workspace;         /* lsm_gnn_embed_backward_workspace_bytes(cfg, B, E) bytes, 8-byte aligned */
  int64_t* bad;            /* [1], nullable, only ever set */
} lsm_gnn_embed_bwd_io;

/* Bytes of workspace for B graphs of E nodes; 0 for B == 0 and for a config or sizes the call refuses. */
size_t lsm_gnn_embed_backward_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E);

int lsm_gnn_embed_backward(lsm_gnn_config cfg, const float* weights /* device blob */, const lsm_gnn_embed_bwd_io* io,
                           int64_t B, int32_t E, int32_t N, void* hip_stream);

/* The same routine on host memory (all pointers host pointers): the same per-graph text with a team of one lane,
 * the same slabs, the same sum order. */
int lsm_host_gnn_embed_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_embed_bwd_io* io, int64_t B,
                                int32_t E, int32_t N);

/* The launch plan lsm_gnn_embed_backward would use, filled on the host by the launch's own code. */
typedef struct lsm_gnn_embed_bwd_launch_plan {
  int32_t TS;        /* lanes per graph: the power of two >= E, at least 32 */
  int32_t G;         /* graphs per workgroup at a time: 256 / TS, fewer when their LDS does not fit */
  int32_t fast;      /* 1: the embed_hidden == 16 instance, 0: the generic one */
  int32_t adj_lds;   /* 1: the transposed adjacency is staged in LDS, 0: read from memory */
  int32_t acc_lds;   /* 1: the graphs' float32 accumulators live in LDS, 0: in the workspace */
  int32_t S;         /* row stride (floats) of P, dh0 and the staged rows */
  int32_t per_graph; /* LDS floats per graph */
  int32_t entries;   /* lsm_gnn_embed_floats */
  int64_t lds_bytes; /* the workgroup's dynamic LDS */
  int64_t slabs;     /* ceil(B / LSM_GNN_BWD_SLAB): the grid of the first launch */
  int64_t ws_bytes;  /* lsm_gnn_embed_backward_workspace_bytes */
} lsm_gnn_embed_bwd_launch_plan;

/* masked != 0: the compact layout. Returns 0, or nonzero with the refusal of these sizes in
 * lsm_gnn_embed_backward_last_error() (the pointer checks are not made); *out is written on success only. */
int lsm_gnn_embed_backward_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked,
                                lsm_gnn_embed_bwd_launch_plan* out);

const char* lsm_gnn_embed_backward_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
