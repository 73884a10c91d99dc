/*
 * lsm_minibatch_edges.h -- C ABI of the minibatch edge lists taken straight from the device replay buffer.
 *
 * In the reference a minibatch's adjacency has one consumer: GNNBase.forward
 * (onpolicy/algorithms/utils/gnn.py:545-564) hands it to process_adj (gnn.py:376-407) and keeps only
 * edge_index / edge_attr. These entry points give that pair for a minibatch whose graphs are named by
 * ids into the buffer's sample rows; the dense [G][E][E] minibatch is never built.
 *
 * A minibatch has G graphs. Graph g has a source row i(g) in the buffer's [T][M] sample rows
 * (rows = T * M, M = n * N, column = env * N + agent):
 *   LSM_MB_INDICES  ids = int64 [count] sample rows, G = count, i(g) = ids[g]
 *                   (the samples of GraphReplayBuffer.feed_forward_generator)
 *   LSM_MB_CHUNKS   ids = int64 [count] chunk ids, G = L * count, g = l * count + b,
 *                   i(g) = row(ids[b], l) with row(c, l) of include/lsm_recurrent.h:
 *                   f = c * L + l, row (f % T) * M + f / T (recurrent_generator's time-major order,
 *                   chunks that run from one column's series into the next included)
 * The matrix of graph g is
 *   reference layout (masks == NULL)  adj[i]                                    adj = [rows][E][E]
 *   compact layout                    (bit r | bit c of masks[i]) ? +0 : A[i / N][r][c]   (a select)
 *                                     adj = A [rows / N][E][E], masks = [rows][W], W = ceil(E / 64)
 * and the result is process_adj of the stacked [G][E][E] matrices: edge_index int64 [2][nnz] holding
 * (g * E + r, g * E + c), edge_attr float32 [nnz][1], in nonzero() order over (g, r, c); NaN counts as
 * nonzero, -0.0 does not. Duplicate ids are allowed.
 *
 * An id outside its range ([0, rows), or [0, rows / L) for chunks) gives its graph (for a chunk, its L
 * graphs) zero edges and sets *bad = 1 when bad is given; no address is formed from it. *bad is only
 * ever set: the caller clears it.
 *
 * The device entry points are stream-ordered and asynchronous, with no host synchronisation. Return
 * value: 0 on success; nonzero on an argument error, before any launch or write, with the text in
 * lsm_mb_edges_last_error() (thread-local, prefix "mb_edges: "). Refused: null adj / offsets /
 * workspace / outputs (ids only when count > 0), E outside [1, 256], the compact layout with N < 1 or
 * rows % N != 0, count < 0, rows < 0 or >= 2^32, G > INT32_MAX, an unknown kind, chunks with L < 1,
 * L > rows, T < 1, M < 1 or T * M != rows, a workspace smaller than lsm_mb_edges_workspace_bytes(G),
 * and cap < 0 where cap is read. G == 0 is legal and gives nnz = 0.
 *
 * The declarations live apart from lsm_rollout.h (part of the rollout's build id), lsm_learner.h and
 * lsm_recurrent.h.
 */
#ifndef LSM_MINIBATCH_EDGES_H
#define LSM_MINIBATCH_EDGES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { LSM_MB_INDICES = 0, LSM_MB_CHUNKS = 1 };

/* The graphs of one minibatch, passed by value. */
typedef struct lsm_mb_graphs {
  const float* adj;      /* reference: [rows][E][E]; compact: A [rows / N][E][E] */
  const uint64_t* masks; /* compact: [rows][W] disconnect words; NULL selects the reference layout */
  int32_t E, N;          /* N: agents per env (compact only; ignored for the reference layout) */
  int64_t rows;          /* T * M sample rows */
  int32_t kind;          /* LSM_MB_INDICES / LSM_MB_CHUNKS */
  const int64_t* ids;    /* [count] */
  int64_t count;
  int64_t L, T, M;       /* LSM_MB_CHUNKS only */
} lsm_mb_graphs;

/* Bytes of the count pass's workspace (per-graph counts + the scan's temporary storage) for G graphs. */
size_t lsm_mb_edges_workspace_bytes(int64_t G);

/* Count kernel (one wave per graph), then an inclusive scan: offsets[0] = 0, offsets[g + 1] = edges of
 * graphs 0 .. g, offsets[G] = nnz. */
int lsm_mb_edges_count(lsm_mb_graphs graphs, int64_t* offsets /* device [G + 1] */, void* workspace,
                       size_t workspace_bytes, int64_t* bad /* device [1], nullable */, void* hip_stream);

/* Emit kernel: graph g's edges at offsets[g].
 *   nnz >= 0  the host knows nnz = offsets[G]: edge_index is [2][nnz], edge_attr [nnz]; cap is ignored.
 *   nnz <  0  nnz is read from offsets[G] on the device and the outputs hold cap edges
 *             (edge_index [2 * cap] words, of which the first 2 * nnz are [2][nnz]); nothing is written
 *             when nnz > cap. */
int lsm_mb_edges_emit(lsm_mb_graphs graphs, const int64_t* offsets /* device [G + 1] */, int64_t nnz,
                      int64_t cap, int64_t* edge_index, float* edge_attr, void* hip_stream);

/* The same routine on host memory (all pointers host pointers): *nnz_out = nnz; the outputs hold cap
 * edges and get [2][nnz] / [nnz] when nnz <= cap, nothing otherwise. */
int lsm_host_mb_edges(lsm_mb_graphs graphs, int64_t cap, int64_t* edge_index, float* edge_attr,
                      int64_t* nnz_out, int64_t* bad /* nullable */);

const char* lsm_mb_edges_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
