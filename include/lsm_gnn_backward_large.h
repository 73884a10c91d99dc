/*
 * lsm_gnn_backward_large.h -- lsm_gnn_backward.h's backward pass (the readout and the TransformerConv layers) for
 * every size lsm_gnn_forward accepts. The tensors (lsm_gnn_bwd_io), the formulas, the ownership, the work split
 * and the SUM ORDER are lsm_gnn_backward.h's, by reference and unchanged: the result does not depend on anything
 * below, and where lsm_gnn_backward accepts a size, these entry points give its bytes.
 *
 * lsm_gnn_backward keeps everything a graph needs in LDS and refuses a size whose single graph does not fit.
 * Of a graph's LDS only the forward's region has to be there: per node 2 * SA + 2 * SK floats (the two activation
 * buffers, k and v) and the disconnect word, which is exactly what lsm_gnn_forward requires to fit. The other
 * regions can live in global memory, in a scratch the workgroup owns. The spill level, 0 to 4, says which do;
 * each level moves one more region out of LDS:
 *
 *   level   moves to the workgroup's scratch, on top of the previous level      floats per node
 *   0       nothing: lsm_gnn_backward's kernel and LDS layout
 *   1       the saved rows h_0 .. h_{layer_N + 1}                               (layer_N + 2) * SA
 *   2       dq                                                                  SK
 *   3       the statistics                                                      ST
 *   4       q; only the forward's region is left in LDS                         SK
 *
 * (the largest region first, the one read most across lanes last: a saved row is written by the lane that owns
 * it and read by it and the weight phase, q is read by every lane for every edge of the source pass).
 *
 * The plan. LDS per graph at level s, in floats, with lsm_gnn_backward.h's SA, SK, ST:
 *   kept(s) = E * (2 * SA + 2 * SK + [s < 1] (layer_N + 2) * SA + [s < 2] SK + [s < 3] ST + [s < 4] SK)
 *             + round_up(E, 4)
 * The level is the lowest s >= min_spill with 4 * kept(s) <= 163840. The adjacency and its transpose are staged
 * in LDS as lsm_gnn_backward does: both or neither, when 4 * (kept(s) + 2 * round_up(E * E, 4)) still fits. TS is
 * the power of two >= E, at least 32; G = min(256 / TS, what fits). A size lsm_gnn_forward accepts is accepted
 * at some level <= 4; one it refuses is refused here, with the forward's figures in the text. The level is a
 * compile-time parameter of the kernels of levels 1 to 4 (the <16, 16> and the generic instance of each), so
 * every access keeps a known address space; at level 0 the call launches the very kernel lsm_gnn_backward
 * launches.
 *
 * Workspace: [slabs][nconv] float64, lsm_gnn_backward's slab accumulators, then from level 1 on the scratch,
 * [slabs][G][spilled_floats] float32 from the first 16-byte boundary behind the accumulators. spilled_floats is
 * a graph's spilled regions (in the order h, q, dq, statistics) rounded up to 16 bytes;
 *   scratch_bytes = 4 * slabs * G * spilled_floats + 8   (the 8: room for that boundary; 0 at level 0)
 *   ws_bytes      = lsm_gnn_backward's figure + scratch_bytes
 * Team i of the workgroup of slab s reads and writes region [s][i] only, except in the weight phase, where the
 * workgroup's threads read all G regions of their own slab; the workgroup barrier between the phases orders a
 * lane's stores to the scratch before another lane's loads. Teams past the slab's end recompute graph B - 1
 * into their own region. Nothing is read across workgroups; offsets into the scratch are 64-bit. No atomics, no
 * host synchronisation, no allocation: two launches, stream-ordered, bit-reproducible.
 *
 * Return value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_gnn_backward_large_last_error() (thread-local, prefix "gnn backward large: "). Refused: min_spill outside
 * [0, 4]; a size lsm_gnn_forward refuses; and everything lsm_gnn_backward refuses except its LDS limit (null and
 * misaligned pointers, B, E, N, overlaps -- the workspace's checks cover the scratch). B == 0 is legal and
 * writes nothing.
 */
#ifndef LSM_GNN_BACKWARD_LARGE_H
#define LSM_GNN_BACKWARD_LARGE_H

#include <stddef.h>
#include <stdint.h>

#include "lsm_gnn_backward.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for B graphs of E nodes at the level the plan takes for min_spill; 0 for B == 0 and for a
 * config, sizes or min_spill the call refuses. */
size_t lsm_gnn_backward_large_workspace_bytes(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t min_spill);

/* io->workspace: lsm_gnn_backward_large_workspace_bytes(cfg, B, E, min_spill) bytes, 8-byte aligned. */
int lsm_gnn_backward_large(lsm_gnn_config cfg, const float* weights /* device blob */, const lsm_gnn_bwd_io* io,
                           int64_t B, int32_t E, int32_t N, int32_t min_spill, void* hip_stream);

/* The same routine on host memory, for every size lsm_gnn_forward accepts: the same per-graph text with a team
 * of one lane, the same slabs, the same sum order. There is no LDS on the host and so no level: the workspace it
 * writes is lsm_gnn_backward's, 8 * slabs * nconv bytes (lsm_gnn_backward_large_workspace_bytes at any level is
 * enough). Bit-equal to lsm_host_gnn_backward wherever that accepts. */
int lsm_host_gnn_backward_large(lsm_gnn_config cfg, const float* weights, const lsm_gnn_bwd_io* io, int64_t B,
                                int32_t E, int32_t N);

/* The launch plan lsm_gnn_backward_large would use: lsm_gnn_bwd_launch_plan's fields and the level's. */
typedef struct lsm_gnn_bwd_large_launch_plan {
  int32_t TS;         /* lanes per graph: the power of two >= E, at least 32 */
  int32_t G;          /* graphs per workgroup at a time: 256 / TS, fewer when their LDS does not fit */
  int32_t fast;       /* 1: the <16, 16> instance, 0: the generic one */
  int32_t adj_lds;    /* 1: the adjacency and its transpose are staged in LDS, 0: read from memory */
  int32_t acc_lds;    /* where the slab accumulators live: always 0, the workspace */
  int32_t SA, SK, ST; /* row strides (floats) of the activation, the k / v / q / dq and the statistics buffers */
  int32_t spill;      /* the level, 0 .. 4 */
  int32_t spilled_floats; /* a graph's floats in the scratch (a multiple of 4; 0 at level 0) */
  int64_t lds_bytes;  /* the workgroup's dynamic LDS */
  int64_t slabs;      /* ceil(B / LSM_GNN_BWD_SLAB): the grid of the first launch */
  int64_t ws_bytes;   /* lsm_gnn_backward_large_workspace_bytes: the accumulators and the scratch */
  int64_t scratch_bytes; /* the scratch's share of ws_bytes */
} lsm_gnn_bwd_large_launch_plan;

/* masked != 0: the compact layout. Returns 0, or nonzero with lsm_gnn_backward_large's refusal of these sizes in
 * lsm_gnn_backward_large_last_error() (the pointer checks are not made); *out is written on success only. */
int lsm_gnn_backward_large_plan(lsm_gnn_config cfg, int64_t B, int32_t E, int32_t N, int32_t masked,
                                int32_t min_spill, lsm_gnn_bwd_large_launch_plan* out);

const char* lsm_gnn_backward_large_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
