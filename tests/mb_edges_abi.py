"""ctypes helpers shared by the minibatch-edges tests (include/lsm_minibatch_edges.h): buffer-shaped
adjacency sources in both layouts on the host or on a torch device, canaried destinations, the entry
points, and the expected value -- oracle/process_adj.py on dense matrices built in numpy from
tests/recurrent_model.py's row function and the oracle's expand_compact. Nothing here comes from the
code under test."""
import ctypes as C

import numpy as np

import recurrent_abi as ra
import recurrent_model as rcm
from lsm import capi
from oracle.process_adj import expand_compact, process_adj

CANARY64 = np.array([ra.CANARY, ra.CANARY], np.int32).view(np.int64)[0]


def graph_rows(ids, rows, chunks):
    """Source row of every graph of the minibatch, in graph order; -1 for an id outside its range."""
    if chunks is not None:
        L, T, M = chunks
        assert T * M == rows
        return rcm.chunk_rows(ids, L, T, M)
    return np.array([int(x) if 0 <= int(x) < rows else -1 for x in ids], dtype=np.int64)


def dense(full, idx):
    """[G, E, E]: full[idx], zero where idx is -1."""
    out = full[np.where(idx >= 0, idx, 0)].copy()
    out[idx < 0] = 0
    return out


def expected(full, ids, chunks):
    """(edge_index [2, nnz], edge_attr [nnz, 1], offsets [G + 1]) of the minibatch: the oracle on the
    dense matrices."""
    d = dense(full, graph_rows(ids, full.shape[0], chunks))
    ei, ea = process_adj(d)
    per = (d != 0).reshape(d.shape[0], -1).sum(axis=1)   # NaN != 0, -0.0 == 0, as nonzero()
    off = np.concatenate([[0], np.cumsum(per)]).astype(np.int64)
    assert off[-1] == ea.shape[0]
    return ei, ea.astype(np.float32), off


class Source:
    """A buffer's adjacency placed once. Reference layout: adj [rows, E, E]. Compact: A [rows / N, E, E]
    and masks [rows, W] uint64. `full` is the [rows, E, E] matrix the layout stands for."""

    def __init__(self, adj, masks=None, N=1, device=None):
        self.device, self.N = device, N
        self.E = adj.shape[-1]
        adj = np.ascontiguousarray(adj, dtype=np.float32)
        self.adj = ra.Placed(adj.view(np.int32), 0, device)
        if masks is None:
            self.masks, self.rows, self.full = None, adj.shape[0], adj
        else:
            masks = np.ascontiguousarray(masks, dtype=np.uint64)
            self.masks = ra.Placed(masks.view(np.int32), 0, device)
            self.rows = masks.shape[0]
            assert self.rows == adj.shape[0] * N
            self.full = expand_compact(adj, masks.reshape(adj.shape[0], N, -1)).reshape(self.rows, self.E, self.E)
            self.full = self.full.astype(np.float32)

    def desc(self, ids_ptr, count, chunks, /, **over):
        d = capi.LsmMbGraphs(adj=self.adj.ptr, masks=self.masks.ptr if self.masks else None, E=self.E, N=self.N,
                             rows=self.rows, kind=capi.LSM_MB_INDICES, ids=ids_ptr, count=count)
        if chunks is not None:
            d.kind = capi.LSM_MB_CHUNKS
            d.L, d.T, d.M = chunks
        for k, v in over.items():
            setattr(d, k, v)
        return d


def graph_count(ids, chunks):
    return len(ids) * (chunks[0] if chunks is not None else 1)


def _outputs(cap, device):
    return ra.destination(4 * cap, 0, device), ra.destination(cap, 0, device)


def _read(ei_dst, ea_dst, nnz, written, what):
    """The destinations' [2, nnz] / [nnz, 1] heads; every word behind the written part is the canary."""
    ei = ra.read_destination(ei_dst, what)
    ea = ra.read_destination(ea_dst, what)
    n = nnz if written else 0
    assert (ei[4 * n:] == ra.CANARY).all() and (ea[n:] == ra.CANARY).all(), "written past nnz: %s" % (what,)
    return ei[:4 * n].view(np.int64).reshape(2, n), ea[:n].view(np.float32).reshape(n, 1)


def run_host(lib, src, ids, chunks=None, cap=None):
    """lsm_host_mb_edges with outputs of cap edges between canaries. Returns (edge_index, edge_attr,
    nnz, bad); the first two are empty when nnz > cap (nothing may be written then)."""
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    idp = ra.Placed(ids.view(np.int32), 0) if len(ids) else None
    if cap is None:
        cap = graph_count(ids, chunks) * src.E * src.E
    ei_dst, ea_dst = _outputs(cap, None)
    tail = np.array([-7, 0], dtype=np.int64)   # nnz_out, bad
    rc = lib.lsm_host_mb_edges(src.desc(idp.ptr if idp else None, len(ids), chunks), cap,
                               C.c_void_p(ei_dst[0].ptr + 4 * ra.PRE), C.c_void_p(ea_dst[0].ptr + 4 * ra.PRE),
                               C.c_void_p(tail.ctypes.data), C.c_void_p(tail.ctypes.data + 8))
    assert rc == 0, lib.lsm_mb_edges_last_error()
    nnz, bad = int(tail[0]), int(tail[1])
    ei, ea = _read(ei_dst, ea_dst, nnz, nnz <= cap, "host")
    return ei, ea, nnz, bad


def run_device(lib, src, ids, chunks=None, dev_nnz=False, cap=None):
    """lsm_mb_edges_count + lsm_mb_edges_emit on src.device. Outputs hold exactly nnz edges (cap edges
    with dev_nnz, the path that reads nnz on the device) and sit between canaries, as do the offsets.
    Returns (edge_index, edge_attr, offsets [G + 1], bad)."""
    import torch
    dev = src.device
    ids = np.ascontiguousarray(ids, dtype=np.int64)
    G = graph_count(ids, chunks)
    idp = ra.Placed(ids.view(np.int32), 0, dev) if len(ids) else None
    d = src.desc(idp.ptr if idp else None, len(ids), chunks)
    off_dst = ra.destination(2 * (G + 1), 0, dev)
    bad = ra.Placed(np.zeros(2, np.int32), 0, dev)
    nbytes = int(lib.lsm_mb_edges_workspace_bytes(G))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    op = C.c_void_p(off_dst[0].ptr + 4 * ra.PRE)
    rc = lib.lsm_mb_edges_count(d, op, C.c_void_p(ws.data_ptr()), nbytes, C.c_void_p(bad.ptr), stream)
    assert rc == 0, lib.lsm_mb_edges_last_error()
    torch.cuda.synchronize()
    offsets = ra.read_destination(off_dst, "offsets").view(np.int64)
    nnz = int(offsets[G])
    if cap is None:
        cap = nnz
    ei_dst, ea_dst = _outputs(cap, dev)
    rc = lib.lsm_mb_edges_emit(d, op, -1 if dev_nnz else nnz, cap, C.c_void_p(ei_dst[0].ptr + 4 * ra.PRE),
                               C.c_void_p(ea_dst[0].ptr + 4 * ra.PRE), stream)
    assert rc == 0, lib.lsm_mb_edges_last_error()
    torch.cuda.synchronize()
    ei, ea = _read(ei_dst, ea_dst, nnz, nnz <= cap, "device")
    np.testing.assert_array_equal(ra.read_destination(off_dst, "offsets after emit").view(np.int64), offsets)
    return ei, ea, offsets, int(bad.read().view(np.int64)[0])


def assert_edges(got_ei, got_ea, want_ei, want_ea, what=""):
    """Bit for bit (NaN attributes compare by their words)."""
    assert got_ei.shape == want_ei.shape and got_ea.shape == want_ea.shape, (what, got_ei.shape, want_ei.shape)
    np.testing.assert_array_equal(got_ei, want_ei, err_msg=str(what))
    np.testing.assert_array_equal(got_ea.view(np.int32), want_ea.view(np.int32), err_msg=str(what))


# ---- the fixtures' two statements of the buffer adjacency -------------------------------------------

def fixture_sources(z, device=None):
    """{"reference": in_adj rows 0 .. T-1, "compact": recurrent_abi.fixture_specs' poisoned table (inf /
    7.5 under common mask bits: a product instead of a select fails on it) + masks}."""
    T, M, E = z["T"], z["M"], z["E"]
    ref = Source(z["in_adj"][:T].reshape(T * M, E, E), device=device)
    spec = ra.fixture_specs(z)[0][-1]
    assert spec["kind"] == "compact" and np.isinf(spec["A"]).any()
    cmp_ = Source(spec["A"], spec["masks"], spec["N"], device=device)
    np.testing.assert_array_equal(cmp_.full.view(np.int32), ref.full.view(np.int32))
    return {"reference": ref, "compact": cmp_}


# ---- synthetic buffers: the smallest shapes at which each path can go wrong ---------------------------

SYN_T, SYN_n, SYN_N = 3, 2, 2          # rows = 12, M = 4
SYN_E = (5, 24, 66, 130)               # odd (4-B loads); one batch; two mask words, several batches; three
# (kind, ids, L): G = 1, 3, 5, 9 graphs -- partial workgroups; duplicate ids; L = 5 > T straddles columns
SYN_CASES = {
    "idx1": ("indices", [1], None), "idx3": ("indices", [0, 3, 0], None),
    "idx5": ("indices", [11, 2, 2, 7, 4], None), "idx9": ("indices", [5, 1, 0, 3, 3, 10, 2, 8, 11], None),
    "chunk1": ("chunks", [7], 1), "chunk3": ("chunks", [1], 3), "chunk5": ("chunks", [1], 5),
    "chunk9": ("chunks", [3, 0, 3], 3),
}


def synthetic(E, device=None):
    """{"reference", "compact"}: one buffer adjacency in both layouts. Tables: 0 all zero, 1 full (no
    zero entry), the others sparse with NaN, -0.0 and inf entries; sample row 2 has no mask bit (a full
    graph), row 3 every bit (an empty one), the others random bits, with bits 0 / 63 / 64 set where E
    reaches them. Under set bits the tables hold nonzero values, inf among them."""
    rng = np.random.default_rng(E)
    rows, N = SYN_T * SYN_n * SYN_N, SYN_N
    A = rng.normal(0, 1, (rows // N, E, E)).astype(np.float32)
    A[rng.random(A.shape) < 0.5] = 0
    A[rng.random(A.shape) < 0.05] = np.nan
    A[rng.random(A.shape) < 0.05] = -0.0
    A[rng.random(A.shape) < 0.03] = np.inf
    A[0] = 0
    A[1] = np.where(A[1] == 0, np.float32(2.5), A[1])
    bits = rng.random((rows, E)) < 0.2
    bits[2], bits[3] = False, True
    for r, pos in ((4, 0), (5, 63), (6, 64), (7, 0), (7, 63), (7, 64), (8, E - 1)):
        if pos < E:
            bits[r, pos] = True
    bits[9] = False
    under = bits[:, :, None] | bits[:, None, :]
    assert np.isinf(A.repeat(N, axis=0)[under]).any() or E < 6
    cmp_ = Source(A, rcm.pack_bits(bits), N, device)
    full = cmp_.full
    assert not full[3].any() and (full[2] != 0).all() and not full[0].any()
    assert np.isnan(full).any() and (np.signbit(full) & (full == 0)).any()
    return {"reference": Source(full, device=device), "compact": cmp_}


def syn_case(name):
    kind, ids, L = SYN_CASES[name]
    return np.array(ids, dtype=np.int64), (None if kind == "indices" else (L, SYN_T, SYN_n * SYN_N))
