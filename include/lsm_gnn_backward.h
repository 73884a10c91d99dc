/*
 * lsm_gnn_backward.h -- C ABI of the backward pass through the graph encoder's readout and its layer_N + 1
 * TransformerConv layers: from dout, the gradient at lsm_gnn_forward's out (lsm_backward.h's dx1), to the
 * gradient of every conv-layer weight of the packed blob and to dh0, the gradient at EmbedConv's output. The
 * config, the weight blob, the two adjacency layouts and the forward's formulas are lsm_gnn.h's. EmbedConv's
 * own backward is NOT here: the blob's EmbedConv entries, [0, offset of conv layer 0's query weight), are
 * written as 0 in this version; their gradient follows from dh0 (a sum over the edges of a per-edge MLP) and is
 * the next piece. The gradient norm and the optimiser are lsm_optim.h's.
 *
 * The call is self-contained: it recomputes the forward from the same inputs with the forward's own per-graph
 * text (csrc/lsm_gnn_tile.h), so the gradient is that of the function lsm_gnn_forward computes. No edge list and
 * no per-edge tensor is built. All arithmetic float32 unless stated. Per graph b, with E nodes:
 *
 * - Readout, dY = the gradient at the last layer's output [E][out_dim]:
 *     LSM_GNN_NODE         dY[agent_id[b]] = dout[b], every other node 0; an agent_id outside [0, E)
 *                          contributes nothing (dY = 0) and sets *bad = 1
 *     LSM_GNN_GLOBAL_ADD   dY[n] = dout[b] for every node
 *     LSM_GNN_GLOBAL_MEAN  dY[n] = dout[b] / E
 *     LSM_GNN_GLOBAL_MAX   per column, dout[b] goes to the lowest-index node that attains the maximum under the
 *                          forward's comparison (a later node replaces the running one when it is greater or
 *                          NaN), every other node gets 0
 *   cfg.ego_only is ignored (the recompute runs every node) and gives the same bytes.
 * - Per conv layer l = layer_N .. 0, with h the layer's input, y its output, q, k, v, alpha the forward's, w_e
 *   the edge weight, e = e_rc the attribute of edge r -> c, C the head width and H the heads:
 *     g_c = dY_c * act'(y_c): ReLU passes dY where y > 0 and gives 0 where y <= 0 (a NaN y passes it, as
 *           torch's); Tanh multiplies by 1 - y^2. g_c is the pre-activation gradient of lin_skip.
 *     dO_c = per head, g_c's slice [hh * C, hh * C + C) under concat, g_c / H under the mean
 *     per incoming edge r -> c and head:
 *       dalpha_rc = <dO_c, v_r> + e <dO_c, w_e>          (= <dO_c, v_r + e w_e>)
 *       s_c       = sum_r alpha_rc dalpha_rc
 *       da_rc     = alpha_rc (dalpha_rc - s_c)
 *     with alpha_rc = exp(a_rc - max_c) / (sum_r exp(a_rc - max_c) + 1e-16) as the forward defines it: a_rc is
 *     recomputed by the forward's expression (the same bits) and max_c is the forward's running maximum at its
 *     end; the denominator is summed again, r ascending, of the exponentials against that final maximum (the
 *     forward's own sum carries the roundings of its rescales, and sum_r alpha_rc would miss 1 by them). The
 *     running maximum is a constant of the differentiation; differentiating through it would change the result
 *     by O(1e-16 * s_c), since the softmax is shift-invariant up to the 1e-16 term.
 *     Per target and head, four sums over the incoming edges are float64 sums of float32 factors, r ascending:
 *     sum p, sum p dalpha, sum p e (p = exp(a - max)) and sum da e; s_c = sum p dalpha / (sum p + 1e-16) and
 *     sum_r alpha_rc e likewise, rounded to float32 once. sum_r da_rc is 0 up to rounding, and a float32 s_c
 *     would leave s_c times a few 2^-24 in it, which is the whole of the key bias's gradient.
 *       dv_r  = sum_c alpha_rc dO_c
 *       dq_c  = (sum_r da_rc k_r + (sum_r da_rc e) w_e) / sqrt(C)
 *       dk_r  = sum_c da_rc q_c / sqrt(C)
 *       dw_e  = sum_c ( dO_c (sum_r alpha_rc e) + q_c (sum_r da_rc e) / sqrt(C) )
 *       dh_c  = W_q^T dq_c + W_k^T dk_c + W_v^T dv_c + W_s^T g_c
 *     dh is the dY of layer l - 1 and, after layer 0, dh0. A target without an incoming edge keeps only the skip
 *     path; a node without an outgoing edge has dk = dv = 0.
 * - Weights, per conv layer: dW_q[j][i] = sum_{b,n} dq[b,n][j] h[b,n][i], and the same with dk, dv and (for
 *   lin_skip) g; each bias is the column sum of its delta; dw_e as above, summed over the graphs.
 * - node_obs and adj are data: no gradient is taken at them. Non-finite inputs give non-finite gradients. No
 *   address is ever formed from data.
 *
 * SUM ORDER (the contract; independent of the launch plan, the grid and the device):
 *   within a graph    every matrix entry's term is one float32 FMA chain over the nodes n = 0 .. E-1 ascending,
 *                     starting from 0. A vector entry's (a bias's, the edge weight's) is a chain of float32
 *                     additions in the same order that also collects each addition's rounding (two-sum) and
 *                     adds their sum back at the end: its terms may cancel to far below their size. Inside a
 *                     node, every sum over incoming
 *                     edges runs r ascending and every sum over outgoing edges c ascending, each in one lane;
 *                     dw_e's term sums over the targets c ascending what each target summed over its sources r
 *                     ascending.
 *   within a slab     graphs are grouped into slabs of LSM_GNN_BWD_SLAB consecutive graphs; a slab's entry is a
 *                     float64 accumulator that starts at 0 and takes the per-graph float32 terms, graphs
 *                     ascending.
 *   across slabs      the slabs' float64 partials are added in ascending order in float64, starting from 0, and
 *                     rounded to float32 once.
 * There are no atomics and no last-block-done counter: a call is bit-reproducible, and the host entry point and
 * the kernel run the same text in the same order.
 *
 * Work split. One workgroup owns one slab and walks it G graphs at a time; a team of TS lanes (the power of two
 * >= E, at least 32) owns one graph and lane c owns node c, as in the forward. Per group of G graphs: the forward
 * with saves; the readout's dY; then per layer (0) g, q, k, v per node, (1) the target pass, lane c over its
 * incoming edges twice (s_c, then dq_c), (2) the source pass, lane r over its outgoing edges c ascending,
 * recomputing a_rc, alpha_rc and da_rc from q_c, c's statistics and its own k_r, v_r (the edge work is paid twice
 * for a fixed order and no atomics), (3) the weight terms: the workgroup's threads split the layer's entries, and
 * the thread that owns an entry adds the G graphs' terms to the slab's accumulator in graph order, (4) dh per
 * node. A second launch adds the slabs' partials and writes dweights.
 *
 * LDS per graph, in floats, pad(w) = round_up(w, 4) + 4, SA = pad(max(embed_hidden, out_dim)),
 * SK = pad(max(embed_hidden, HC)):
 *   E * ((layer_N + 4) * SA + 4 * SK + ST) + round_up(E, 4),  ST = (2 * H * (layer_N + 1) + 5 * H) | 1
 * (the forward's two activation buffers, reused for dY; every layer's input and the last output; k, v, q, dq;
 * per node and head the forward's maximum and 1 / (den + 1e-16) of every layer and s, sum alpha e, sum da e,
 * <q, w_e>, <dO, w_e> of the current one), plus 2 * round_up(E * E, 4) for the adjacency and its transpose when
 * that still fits in the 163840 bytes of a workgroup. Nothing is stored per edge. A size whose single graph
 * does not fit is refused (reference defaults: 1444 bytes per node, accepted up to E = 113; the forward accepts
 * sizes this call refuses, and lsm_gnn_backward_large.h runs this pass at them). G = min(256 / TS, what fits).
 *
 * Workspace: 0 bytes per graph; per slab one float64 row of the conv layers' entries,
 *   8 * ceil(B / LSM_GNN_BWD_SLAB) * (lsm_gnn_weights_floats(cfg) - offset of conv layer 0) bytes
 * (reference defaults: 8304 entries, 66432 bytes per slab). The slab accumulators always live there (each
 * workgroup reads and writes its own row only), never in LDS; the plan reports acc_lds = 0.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_gnn_backward_last_error() (thread-local, prefix "gnn backward: "). Refused: lsm_gnn.h's limits and the LDS
 * need above (with the figures in the text); a null io, weights, dweights or workspace; with B > 0 a null
 * node_obs, adj or dout; LSM_GNN_NODE with a null agent_id; the compact layout with N < 1 or B % N != 0; B < 0
 * or B > INT32_MAX; misaligned pointers (4 bytes; masks, agent_id, bad and workspace: 8); an output (dweights,
 * dh0, workspace, bad) overlapping an input or another output. B == 0 is legal and writes nothing.
 * lsm_gnn_backward is stream-ordered and asynchronous: two launches, no host synchronisation, no allocation.
 */
#ifndef LSM_GNN_BACKWARD_H
#define LSM_GNN_BACKWARD_H

#include <stddef.h>
#include <stdint.h>

#include "lsm_gnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Graphs per slab of the weight-gradient reduction. */
#define LSM_GNN_BWD_SLAB 256

/* One call's tensors: device pointers for lsm_gnn_backward, host pointers for lsm_host_gnn_backward. */
typedef struct lsm_gnn_bwd_io {
  const float* node_obs;   /* [B][E][F] */
  const float* adj;        /* either layout, as lsm_gnn_forward */
  const uint64_t* masks;   /* NULL = reference layout */
  const int64_t* agent_id; /* [B], LSM_GNN_NODE */
  const float* dout;       /* [B][out_dim]: the gradient at lsm_gnn_forward's out */
  float* dweights;         /* [lsm_gnn_weights_floats(cfg)], the blob's own layout, overwritten */
  float* dh0;              /* [B][E][embed_hidden], nullable */
  void* workspace;         /* lsm_gnn_backward_workspace_bytes(cfg, B, E) bytes, 8-byte aligned */
  int64_t* bad;            /* [1], nullable, only ever set */
} lsm_gnn_bwd_io;

/* Bytes of workspace for B graphs of E nodes; 0 for B == 0 and for a config or sizes the call refuses. */
size_t lsm_gnn_backward_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E);

int lsm_gnn_backward(lsm_gnn_config cfg, const float* weights /* device blob */, const lsm_gnn_bwd_io* io, int64_t B,
                     int32_t E, int32_t N, void* hip_stream);

/* The same routine on host memory (all pointers host pointers): the same per-graph text with a team of one
 * lane, the same slabs, the same sum order. */
int lsm_host_gnn_backward(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B, int32_t E,
                          int32_t N);

/* The launch plan lsm_gnn_backward would use, filled on the host by the launch's own code. */
typedef struct lsm_gnn_bwd_launch_plan {
  int32_t TS;         /* lanes per graph: the power of two >= E, at least 32 */
  int32_t G;          /* graphs per workgroup at a time: 256 / TS, fewer when their LDS does not fit */
  int32_t fast;       /* 1: the <16, 16> instance, 0: the generic one */
  int32_t adj_lds;    /* 1: the adjacency and its transpose are staged in LDS, 0: read from memory */
  int32_t acc_lds;    /* where the slab accumulators live: always 0, the workspace */
  int32_t SA, SK, ST; /* row strides (floats) of the activation, the k / v / q / dq and the statistics buffers */
  int64_t lds_bytes;  /* the workgroup's dynamic LDS */
  int64_t slabs;      /* ceil(B / LSM_GNN_BWD_SLAB): the grid of the first launch */
  int64_t ws_bytes;   /* lsm_gnn_backward_workspace_bytes */
} lsm_gnn_bwd_launch_plan;

/* masked != 0: the compact layout. Returns 0, or nonzero with lsm_gnn_backward's refusal of these sizes in
 * lsm_gnn_backward_last_error() (the pointer checks are not made); *out is written on success only. */
int lsm_gnn_backward_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked,
                          lsm_gnn_bwd_launch_plan* out);

const char* lsm_gnn_backward_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
