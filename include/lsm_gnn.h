/*
 * lsm_gnn.h -- C ABI of the fused forward pass of the reference's graph encoder, GNNBase.forward
 * (onpolicy/algorithms/utils/gnn.py:545-564): EmbedConv, gnn_layer_N + 1 TransformerConv layers and the
 * readout, for B graphs of E nodes, in one launch. The input is a step's node_obs and its adjacency in
 * either layout; no edge list and no per-edge tensor is built, and nothing synchronises with the host.
 * This is the forward alone (GMPERunner.collect and evaluation, under torch.no_grad()); the backward pass
 * through the readout and the conv layers is lsm_gnn_backward.h's, which recomputes this forward itself.
 *
 * What is computed (all arithmetic float32). Graph b has nodes x = node_obs[b] [E][F]; the last column is
 * the entity type. Edge (r -> c) exists when the graph's matrix entry [r][c] is nonzero (NaN counts as
 * nonzero, -0.0 does not: process_adj); its attribute e is that entry; messages flow from r to c.
 *   reference layout (masks == NULL)  adj[b][r][c]                              adj = [B][E][E]
 *   compact layout                    (bit r | bit c of masks[b]) ? +0 : A[b / N][r][c]   (a select)
 *                                     adj = A [B / N][E][E], masks = [B][W], W = ceil(E / 64)
 * 1. EmbedConv (aggr = add): m = lin1([x_r[:F-1], entity_embed[trunc(x_r[F-1])], e]), act, layer_norm,
 *    then embed_layer_N times (Linear, act, layer_norm); h0_c = sum of m over the incoming edges of c
 *    (0 without one). layer_norm is ONE LayerNorm(embed_hidden) (eps 1e-5, biased variance) used at every
 *    position, the identity when cfg.layer_norm == 0. embed_add_self_loop has no effect in the reference
 *    (edge_attr is never None there, gnn.py:112) and has no field here.
 * 2. TransformerConv (beta off, dropout 0, edge_dim 1, root_weight on), layer_N + 1 times: per node
 *    q, k, v = lin_query / lin_key / lin_value (h) as [H][C]; per edge ee = lin_edge(e) (no bias);
 *    a = <q_c, k_r + ee> / sqrt(C) per head; softmax over the incoming edges of c,
 *    exp(a - max) / (sum exp(a - max) + 1e-16); out_c = sum alpha (v_r + ee); heads concatenated to
 *    [H * C] or averaged to [C]; out_c += lin_skip(h_c) (alone when c has no incoming edge); then the
 *    net's activation.
 * 3. Readout: LSM_GNN_NODE: row b is node agent_id[b]'s features; LSM_GNN_GLOBAL_MEAN / _MAX / _ADD:
 *    over the E nodes. out is [B][out_dim], out_dim = C * (concat ? H : 1).
 *
 * The packed weight blob (float32, lsm_gnn_weights_floats(cfg) values, torch's [out][in] row-major
 * Linear weights), in this order, with K = F - 1 + embedding_size + 1, HC = H * C, out_dim as above and
 * Din = embed_hidden for conv layer 0, out_dim for the others:
 *   entity_embed [num_embeddings][embedding_size]
 *   lin1 weight [embed_hidden][K], bias [embed_hidden]
 *   layer_norm gamma [embed_hidden], beta [embed_hidden]        (present, unread, when layer_norm == 0)
 *   embed layer k = 0 .. embed_layer_N - 1: weight [embed_hidden][embed_hidden], bias [embed_hidden]
 *   conv layer l = 0 .. layer_N (gnn1, then gnn2[l - 1]):
 *     query weight [HC][Din], bias [HC]; key weight, bias; value weight, bias (same shapes);
 *     edge weight [HC]; skip weight [out_dim][Din], bias [out_dim]
 *
 * Limits (refused beyond them): F in [2, 64]; num_embeddings, embedding_size in [1, 64]; embed_hidden and
 * C in [1, 64]; H in [1, 4]; H * C <= 256; embed_layer_N and layer_N in [0, 4]; E in [1, 256]. All of a
 * graph's activations stay in the workgroup's LDS, so additionally
 *   4 * E * (2 * pad(max(embed_hidden, out_dim)) + 2 * pad(max(embed_hidden, HC)) + 1) <= 163840 bytes,
 *   pad(w) = round_up(w, 4) + 4
 * (reference defaults: every E <= 256 fits; H * C = 256 fits up to E = 39). The adjacency is staged in
 * LDS as well when E * E more floats fit, and read from memory in each layer otherwise.
 *
 * Bad inputs: an entity type that is not finite or outside [0, num_embeddings) after truncation
 * contributes a zero embedding and sets *bad = 1; an agent_id outside [0, E) gives a zero output row and
 * sets *bad = 1. No address is formed from either. *bad is only ever set: the caller clears it.
 *
 * lsm_gnn_forward is stream-ordered and asynchronous: one kernel launch, no host synchronisation, no
 * allocation, no atomics (each target's incoming edges are reduced by the one lane that owns the target,
 * sources ascending, so the output is bit-reproducible from run to run). Return value: 0 on success;
 * nonzero on an argument error, before any launch or write, with the text in lsm_gnn_last_error()
 * (thread-local, prefix "gnn: "). Refused: a null weights / node_obs / adj / out (when B > 0 for the
 * last three), a size outside the limits above, the compact layout with N < 1 or B % N != 0, B < 0 or
 * B > INT32_MAX, an unknown aggregation, LSM_GNN_NODE with a null agent_id, misaligned pointers.
 * B == 0 is legal and does nothing.
 *
 * The declarations live apart from lsm_rollout.h (part of the rollout's build id), lsm_learner.h,
 * lsm_recurrent.h and lsm_minibatch_edges.h.
 */
#ifndef LSM_GNN_H
#define LSM_GNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LSM_GNN_NODE = 0, LSM_GNN_GLOBAL_MEAN = 1, LSM_GNN_GLOBAL_MAX = 2, LSM_GNN_GLOBAL_ADD = 3 };

/* The network's shape, passed by value (the reference's argument names in brackets). */
typedef struct lsm_gnn_config {
  int32_t F;              /* node_obs columns, the entity type last */
  int32_t num_embeddings; /* [num_embeddings] */
  int32_t embedding_size; /* [embedding_size] */
  int32_t embed_hidden;   /* [embed_hidden_size] */
  int32_t embed_layer_N;  /* [embed_layer_N] */
  int32_t embed_relu;     /* [embed_use_ReLU]: 1 ReLU, 0 Tanh */
  int32_t layer_norm;     /* [use_feature_normalization] */
  int32_t C;              /* [gnn_hidden_size] */
  int32_t H;              /* [gnn_num_heads] */
  int32_t concat;         /* [gnn_concat_heads] */
  int32_t layer_N;        /* [gnn_layer_N]: gnn2's layers; layer_N + 1 convolutions in all */
  int32_t relu;           /* [gnn_use_ReLU] */
  int32_t aggr;           /* LSM_GNN_NODE / LSM_GNN_GLOBAL_* */
  int32_t ego_only;       /* LSM_GNN_NODE only, a timing knob: 1 = the last layer's attention runs for
                             the ego node alone (same output). 0 is the default. */
} lsm_gnn_config;

/* Length of the packed weight blob in floats; 0 for a config outside the limits. */
size_t lsm_gnn_weights_floats(lsm_gnn_config cfg);

int lsm_gnn_forward(lsm_gnn_config cfg, const float* weights /* device blob */,
                    const float* node_obs /* device [B][E][F] */, const float* adj,
                    const uint64_t* masks /* NULL = reference layout */, int64_t B, int32_t E, int32_t N,
                    const int64_t* agent_id /* device [B], nullable for global */,
                    float* out /* device [B][out_dim] */, int64_t* bad /* device [1], nullable */,
                    void* hip_stream);

/* The same routine on host memory (all pointers host pointers), through the same per-graph code. */
int lsm_host_gnn_forward(lsm_gnn_config cfg, const float* weights, const float* node_obs, const float* adj,
                         const uint64_t* masks, int64_t B, int32_t E, int32_t N, const int64_t* agent_id,
                         float* out, int64_t* bad);

const char* lsm_gnn_last_error(void);

/* The launch plan lsm_gnn_forward would use for these sizes (what lsm_kernel_name is for the step kernels):
 * filled on the host by the launch's own code, nothing is launched and no pointer is needed. */
typedef struct lsm_gnn_launch_plan {
  int32_t TS;        /* lanes per graph: the power of two >= E, at least 32 */
  int32_t G;         /* graphs per workgroup: 256 / TS, fewer when their LDS does not fit; G * TS threads */
  int32_t adj_lds;   /* 1: the adjacency is staged in LDS */
  int32_t fast;      /* 1: the <16, 16> instance, 0: the generic one */
  int32_t SA, SK;    /* padded row strides (floats) of the activation and the k / v buffers */
  int64_t lds_bytes; /* the workgroup's dynamic LDS */
} lsm_gnn_launch_plan;

/* masked != 0: the compact layout (masks != NULL). Returns 0, or nonzero with lsm_gnn_forward's refusal of
 * these sizes in lsm_gnn_last_error() (the pointer checks are not made); *out is written on success only. */
int lsm_gnn_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked, lsm_gnn_launch_plan* out);

#ifdef __cplusplus
}
#endif
#endif
