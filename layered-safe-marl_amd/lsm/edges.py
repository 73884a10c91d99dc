"""Device-side ``GNNBase.process_adj`` (``onpolicy/algorithms/utils/gnn.py:376-407``).

``process_adj(adj)`` takes the rollout's adjacency (a CUDA float32 tensor ``(B, E, E)`` or
``(E, E)``, e.g. ``GpuGraphVecEnv.t_adj`` viewed as ``(n*N, E, E)``) and returns
``(edge_index int64 [2, nnz], edge_attr float32 [nnz, 1])`` in ``nonzero()`` order, the pair the
reference's GNN consumes. ``process_adj_compact(A, masks, N)`` does the same for the compact layout
(``LSM_ADJ_COMPACT``: one ``[n, E, E]`` table + per-ego disconnect masks), expanding each ego's
matrix on the fly instead of materialising ``(n, N, E, E)``.

Like ``torch.nonzero`` the call synchronises once (the edge count sizes the outputs): after both
kernels when the upper bound B*E*E of the outputs fits BOUNDED_OUTPUT_BYTES (the results are then
contiguous views of those buffers, copied to exact size when they would hold more than twice the
edges), else between them. ``counts`` (int64 [B], the step kernel's LSM_OUT_ADJ_NNZ for this
adjacency) skips the count pass: the call is then a scan and one emit pass over the adjacency
(``lsm_edges_scan_emit``), and a count that does not match its graph raises. All work runs in
``lsm_edges.hip`` through the C ABI; there is no torch/CPU fallback.

``minibatch_edges(buffer_adj, masks, N, ids, chunks=None)`` is ``process_adj`` of a PPO minibatch named
by sample or chunk ids into a replay buffer's adjacency (either layout), without the dense minibatch
(``lsm_mb_edges.hip``); ``DeviceGraphBuffer``'s generators call it with ``edges=True``.
"""
from __future__ import annotations

import ctypes as C

from . import capi
from ._device import _torch


class EdgeError(RuntimeError):
    pass


def _check(rc, lib):
    if rc != 0:
        raise EdgeError(lib.lsm_edges_last_error().decode())


# outputs sized by the edge-count upper bound B*E*E up to this many bytes: count and emit then run back
# to back and the call synchronises once, after both (the returned tensors are views of the
# bounded buffers); above it the count is read first and the outputs are sized exactly
BOUNDED_OUTPUT_BYTES = 1 << 30
# a bounded result holding fewer than cap / SHRINK_RATIO edges is copied to exact size, so what the
# caller keeps is O(nnz) (at most SHRINK_RATIO x the exact storage), not O(B*E*E)
SHRINK_RATIO = 2


# offsets + scan workspace of the last few (device, stream, B): reused by the next call with the same
# key (stream-ordered: that call's count kernel runs after this call's emit kernel has read them), so a
# call's host prologue before its first launch -- GPU idle time after the previous call's sync -- is
# two ctypes launches instead of two allocations and a workspace query more
_SCRATCH = {}


def _scratch(lib, dev, stream_handle, B):
    torch = _torch()
    key = (dev.index, stream_handle, B)
    hit = _SCRATCH.get(key)
    if hit is None:
        ws_bytes = int(lib.lsm_edges_workspace_bytes(B))
        hit = (torch.empty(B + 2, dtype=torch.int64, device=dev),   # offsets[B + 1]: counts-path error word
               torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev), ws_bytes)
        if len(_SCRATCH) >= 8:
            _SCRATCH.clear()
        _SCRATCH[key] = hit
    return hit


def _bounded(ebuf, abuf, nnz, cap):
    """The [2, nnz] / [nnz, 1] results as views of the bounded buffers, or exact-size copies when the
    buffers are more than SHRINK_RATIO x what they hold (a kept view pins B*E*E*20 B)."""
    ei, ea = ebuf[:2 * nnz].view(2, nnz), abuf[:nnz].view(nnz, 1)
    if nnz * SHRINK_RATIO < cap:
        ei, ea = ei.clone(), ea.clone()
    return ei, ea


def _run(adj, masks, B, E, N, counts=None):
    torch = _torch()
    lib = capi.load_library()
    dev = adj.device
    if dev.type != "cuda":
        raise EdgeError("process_adj needs a CUDA (HIP) tensor; the edge list is built on the GPU")
    sh = torch.cuda.current_stream(dev).cuda_stream
    stream = C.c_void_p(sh)
    offsets, ws, ws_bytes = _scratch(lib, dev, sh, B)
    mp = C.c_void_p(masks.data_ptr()) if masks is not None else None
    ap = C.c_void_p(adj.data_ptr())
    cap = B * E * E
    if counts is not None:
        # one adjacency pass: the step kernel's per-graph counts -> scan -> emit (one ctypes call)
        if counts.dtype != torch.int64 or counts.numel() != B or counts.device != dev:
            raise EdgeError("counts must be int64 [B] on the adjacency's device (LSM_OUT_ADJ_NNZ)")
        counts = counts.contiguous()
        ebuf = torch.empty(2 * max(cap, 1), dtype=torch.int64, device=dev)
        abuf = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
        host = (C.c_int64 * 2)()   # nnz, mismatched graphs: read back by the call itself (the one sync)
        _check(lib.lsm_edges_scan_emit(ap, mp, B, E, N, C.c_void_p(counts.data_ptr()),
                                       C.c_void_p(offsets.data_ptr()), C.c_void_p(ws.data_ptr()), ws_bytes, cap,
                                       C.c_void_p(ebuf.data_ptr()), C.c_void_p(abuf.data_ptr()), host, stream), lib)
        nnz, bad = int(host[0]), int(host[1])
        if nnz > cap:
            raise EdgeError("edge count %d exceeds B*E*E = %d" % (nnz, cap))
        if bad:
            raise EdgeError("%d graphs' nonzeros differ from the given counts (counts of another adjacency?)" % bad)
        return _bounded(ebuf, abuf, nnz, cap)
    _check(lib.lsm_edges_count(ap, mp, B, E, N, C.c_void_p(offsets.data_ptr()), C.c_void_p(ws.data_ptr()),
                               ws_bytes, stream), lib)
    if 0 < cap * 20 <= BOUNDED_OUTPUT_BYTES:
        ebuf = torch.empty(2 * cap, dtype=torch.int64, device=dev)
        abuf = torch.empty(cap, dtype=torch.float32, device=dev)
        _check(lib.lsm_edges_emit_dev(ap, mp, B, E, N, C.c_void_p(offsets.data_ptr()), cap,
                                      C.c_void_p(ebuf.data_ptr()), C.c_void_p(abuf.data_ptr()), stream), lib)
        nnz = int(offsets[B].item())   # the one sync, as in torch.nonzero (after both kernels)
        if nnz > cap:
            raise EdgeError("edge count %d exceeds B*E*E = %d" % (nnz, cap))
        return _bounded(ebuf, abuf, nnz, cap)
    nnz = int(offsets[B].item())   # the one sync, as in torch.nonzero
    edge_index = torch.empty((2, nnz), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((nnz, 1), dtype=torch.float32, device=dev)
    if nnz:
        _check(lib.lsm_edges_emit(ap, mp, B, E, N, C.c_void_p(offsets.data_ptr()), nnz,
                                  C.c_void_p(edge_index.data_ptr()), C.c_void_p(edge_attr.data_ptr()), stream), lib)
    return edge_index, edge_attr


def _mb_check(rc, lib):
    if rc != 0:
        raise EdgeError(lib.lsm_mb_edges_last_error().decode())


# offsets (+ the bad-id word, cleared here and after every report) and workspace of the last few
# (device, stream, G) of minibatch_edges, reused like _SCRATCH
_MB_SCRATCH = {}


def _mb_scratch(lib, dev, stream_handle, G):
    torch = _torch()
    key = (dev.index, stream_handle, G)
    hit = _MB_SCRATCH.get(key)
    if hit is None:
        ws_bytes = int(lib.lsm_mb_edges_workspace_bytes(G))
        hit = (torch.zeros(G + 2, dtype=torch.int64, device=dev),   # offsets[G + 1]: the bad-id word
               torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev), ws_bytes)
        if len(_MB_SCRATCH) >= 8:
            _MB_SCRATCH.clear()
        _MB_SCRATCH[key] = hit
    return hit


def minibatch_edges(buffer_adj, masks, N, ids, *, chunks=None):
    """``process_adj`` of a minibatch whose graphs are named by ids into a replay buffer's sample rows
    (``include/lsm_minibatch_edges.h``, ``csrc/lsm_mb_edges.hip``); the dense ``[G, E, E]`` minibatch is
    not built.

    ``buffer_adj``: the buffer's adjacency over its ``rows = T * n * N`` sample rows, a contiguous
    float32 CUDA tensor ``[..., E, E]``: ``rows`` matrices in the reference layout (``masks`` None), or
    the ``rows / N`` per-env tables of the compact layout with ``masks`` int64 ``[..., ceil(E/64)]``, one
    row of disconnect words per sample. ``ids`` int64: sample rows (``chunks`` None, the samples of
    ``feed_forward_generator``; graph g = ``ids[g]``), or chunk ids with ``chunks = (L, T, M)`` (the
    minibatch of ``recurrent_generator``: graph ``l * len(ids) + b`` is step l of chunk ``ids[b]``).
    Returns ``(edge_index int64 [2, nnz], edge_attr float32 [nnz, 1])`` with node numbers ``g * E + r``,
    equal to ``process_adj`` of the gathered minibatch adjacency. An id outside its range raises.

    The call follows ``process_adj``'s policy: one synchronisation, after both kernels when the bound
    ``G * E * E`` of the outputs fits BOUNDED_OUTPUT_BYTES (results are views of the bounded buffers,
    copied to exact size below 1 / SHRINK_RATIO of it), else between them."""
    torch = _torch()
    lib = capi.load_library()
    dev = buffer_adj.device
    if dev.type != "cuda":
        raise EdgeError("minibatch_edges needs CUDA (HIP) tensors; the edge list is built on the GPU")
    if buffer_adj.dtype != torch.float32 or buffer_adj.dim() < 3 or buffer_adj.size(-1) != buffer_adj.size(-2):
        raise EdgeError("buffer_adj must be float32 [..., E, E]")
    if not buffer_adj.is_contiguous():
        raise EdgeError("buffer_adj must be contiguous (a slice of leading rows is)")
    if ids.dtype != torch.int64 or ids.dim() != 1 or ids.device != dev:
        raise EdgeError("ids must be int64 [count] on the adjacency's device")
    ids = ids.contiguous()
    E = buffer_adj.size(-1)
    graphs = buffer_adj.numel() // (E * E)
    if masks is None:
        rows, mp = graphs, None
    else:
        W = (E + 63) // 64
        if masks.dtype != torch.int64 or masks.device != dev or masks.size(-1) != W or not masks.is_contiguous():
            raise EdgeError("masks must be contiguous int64 [..., ceil(E/64)] on the adjacency's device")
        rows = masks.numel() // W
        if N < 1 or rows != graphs * N:
            raise EdgeError("compact layout: %d mask rows for %d tables of N = %d agents" % (rows, graphs, N))
        mp = masks.data_ptr()
    d = capi.LsmMbGraphs(adj=buffer_adj.data_ptr(), masks=mp, E=E, N=int(N), rows=rows, kind=capi.LSM_MB_INDICES,
                         ids=ids.data_ptr() or None, count=ids.numel())
    G = ids.numel()
    if chunks is not None:
        d.kind = capi.LSM_MB_CHUNKS
        d.L, d.T, d.M = (int(x) for x in chunks)
        if d.L < 1:
            raise EdgeError("chunks: L < 1")
        G *= d.L
    if G > 2 ** 31 - 1:
        raise EdgeError("more than 2^31 - 1 graphs in one call; split the minibatch")
    sh = torch.cuda.current_stream(dev).cuda_stream
    stream = C.c_void_p(sh)
    offsets, ws, ws_bytes = _mb_scratch(lib, dev, sh, G)
    op = offsets.data_ptr()
    _mb_check(lib.lsm_mb_edges_count(d, C.c_void_p(op), C.c_void_p(ws.data_ptr()), ws_bytes,
                                     C.c_void_p(op + 8 * (G + 1)), stream), lib)
    cap = G * E * E

    def read_nnz():   # the one sync, as in torch.nonzero: offsets[G] and the bad-id word behind it
        nnz, bad = offsets[G:].tolist()
        if bad:
            offsets[G + 1] = 0
            raise EdgeError("an id is outside the buffer's %s" % ("chunks" if chunks is not None else "sample rows"))
        if nnz > cap:
            raise EdgeError("edge count %d exceeds G*E*E = %d" % (nnz, cap))
        return nnz

    if 0 < cap * 20 <= BOUNDED_OUTPUT_BYTES:
        ebuf = torch.empty(2 * cap, dtype=torch.int64, device=dev)
        abuf = torch.empty(cap, dtype=torch.float32, device=dev)
        _mb_check(lib.lsm_mb_edges_emit(d, C.c_void_p(op), -1, cap, C.c_void_p(ebuf.data_ptr()),
                                        C.c_void_p(abuf.data_ptr()), stream), lib)
        return _bounded(ebuf, abuf, read_nnz(), cap)   # after both kernels
    nnz = read_nnz()
    edge_index = torch.empty((2, nnz), dtype=torch.int64, device=dev)
    edge_attr = torch.empty((nnz, 1), dtype=torch.float32, device=dev)
    if nnz:
        _mb_check(lib.lsm_mb_edges_emit(d, C.c_void_p(op), nnz, nnz, C.c_void_p(edge_index.data_ptr()),
                                        C.c_void_p(edge_attr.data_ptr()), stream), lib)
    return edge_index, edge_attr


def process_adj(adj, counts=None):
    """gnn.py:376-407 on a (B, E, E) or (E, E) float32 CUDA tensor; counts: optional int64 [B]
    per-graph nonzeros (LSM_OUT_ADJ_NNZ of the step that wrote adj)."""
    torch = _torch()
    if not (2 <= adj.dim() <= 3) or adj.size(-1) != adj.size(-2):
        raise EdgeError("adj must be (B, E, E) or (E, E)")   # the reference asserts the same
    if adj.dtype != torch.float32:
        raise EdgeError("adj must be float32 (the runner's buffer dtype, graph_buffer.py:95-104)")
    a = adj.contiguous()
    E = a.size(-1)
    B = a.size(0) if a.dim() == 3 else 1
    return _run(a, None, B, E, 1, None if counts is None else counts.reshape(-1))


def process_adj_compact(table, masks, num_agents: int, counts=None):
    """Edges of the per-ego graphs of a compact-layout adjacency: ``table`` [n, E, E] float32,
    ``masks`` [n, N, ceil(E/64)] int64 (bit r of ego e = entity r disconnected). Graph b = env*N +
    ego, so the result equals ``process_adj(expand_compact_adj(table, masks, E).view(-1, E, E))``."""
    torch = _torch()
    n, E = table.size(0), table.size(-1)
    W = (E + 63) // 64
    if table.dtype != torch.float32 or tuple(table.shape) != (n, E, E):
        raise EdgeError("table must be float32 [n, E, E]")
    if tuple(masks.shape) != (n, num_agents, W) or masks.dtype != torch.int64:
        raise EdgeError("masks must be int64 [n, N, ceil(E/64)]")
    return _run(table.contiguous(), masks.contiguous(), n * num_agents, E, num_agents,
                None if counts is None else counts.reshape(-1))
