"""ctypes helpers shared by the recurrent hand-off tests (include/lsm_recurrent.h): lay sources and
canaried destinations out on the host or on a torch device, call the entry points and return numpy
arrays, and load the reference fixtures (tests/golden/recurrent/)."""
import ctypes as C
import glob
import os

import numpy as np

import recurrent_model as rcm
from lsm import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recurrent")
CANARY = np.int32(-559038737)  # 0xDEADBEEF
PRE, TAIL = 4, 8               # canary words before (16 B: keeps the alignment) and after a destination


def fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    for k in ("T", "n", "N", "E", "L", "num_mini_batch", "recurrent_N", "use_centralized_V"):
        z[k] = int(z[k])
    z["M"] = z["n"] * z["N"]
    z["mb"] = len(z["perm"]) // z["num_mini_batch"]
    return z


def words(a, rows):
    """[rows, ...] float32 / int32 -> [rows, words] int32 (the bytes, unchanged)."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4
    return a.reshape(rows, -1).view(np.int32)


def aligned_words(nwords):
    """A zeroed int32 array whose first element is 16-byte aligned."""
    raw = np.zeros(nwords + 4, dtype=np.int32)
    skip = (-raw.ctypes.data // 4) % 4
    out = raw[skip:skip + nwords]
    assert out.ctypes.data % 16 == 0
    return out


class Placed:
    """Flat int32 words at `off` words past a 16-byte boundary, on the host or on a torch device."""

    def __init__(self, data, off=0, device=None):
        data = np.ascontiguousarray(data).reshape(-1).view(np.int32)
        self.off, self.size, self.device = off, data.size, device
        host = aligned_words(off + data.size)
        host[off:] = data
        if device is None:
            self.buf = host
            self.ptr = host.ctypes.data + 4 * off
        else:
            import torch
            self.buf = torch.as_tensor(host, device=device)
            self.ptr = self.buf.data_ptr() + 4 * off
        assert self.ptr % 16 == (4 * off) % 16

    def read(self):
        a = self.buf if self.device is None else self.buf.cpu().numpy()
        return a[self.off:]


def destination(nwords, off, device):
    """A destination of nwords behind PRE + off canary words and before TAIL more."""
    return Placed(np.full(PRE + nwords + TAIL, CANARY, dtype=np.int32), off, device), nwords


def read_destination(dst, what=""):
    p, n = dst
    host = p.buf if p.device is None else p.buf.cpu().numpy()
    a = host[p.off:]
    assert (a[:PRE] == CANARY).all() and (a[PRE + n:] == CANARY).all(), "canary overwritten: %s" % (what,)
    assert (host[:p.off] == 0).all(), "bytes before the destination's buffer written: %s" % (what,)
    return a[PRE:PRE + n].copy()


def _sync(device):
    if device is not None:
        import torch
        torch.cuda.synchronize()


def _stream(device):
    if device is None:
        return None
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ChunkSources:
    """Source arrays placed once. specs: dicts with kind 'rows' / 'first' (src: [T * M, words] int32,
    off: words off a 16-byte boundary, for src and dst) or 'compact' (A [T * M / N, E, E] float32, masks
    [T * M, W] uint64, N)."""

    def __init__(self, specs, device=None):
        self.specs, self.device = specs, device
        self.placed = []
        for s in specs:
            if s["kind"] == "compact":
                self.placed.append((Placed(s["A"].view(np.int32), 0, device),
                                    Placed(np.ascontiguousarray(s["masks"]).view(np.int32), 0, device)))
            else:
                self.placed.append((Placed(s["src"], s.get("off", 0), device), None))

    def run(self, lib, chunks, L, T, M, expect_rc=0):
        """One lsm_*_gather_chunks call over all fields. Returns ([dst rows, words] int32 per field, bad)."""
        dev = self.device
        chunks = np.asarray(chunks, dtype=np.int64)
        Cn = len(chunks)
        ch = Placed(chunks.view(np.int32), 0, dev)
        bad = Placed(np.zeros(2, np.int32), 0, dev)
        fields = (capi.LsmChunkField * len(self.specs))()
        dsts = []
        for f, s, (src, masks) in zip(fields, self.specs, self.placed):
            drows = Cn if s["kind"] == "first" else L * Cn
            if s["kind"] == "compact":
                E = s["A"].shape[-1]
                w = E * E
                f.kind, f.E, f.N, f.masks = capi.LSM_CHUNK_COMPACT_ADJ, E, s["N"], masks.ptr
            else:
                w = s["src"].shape[1]
                f.kind = capi.LSM_CHUNK_FIRST_ROW if s["kind"] == "first" else capi.LSM_CHUNK_ROWS
                f.row_bytes = 4 * w
            d = destination(drows * w, s.get("off", 0), dev)
            f.src, f.dst = src.ptr, d[0].ptr + 4 * PRE
            dsts.append((d, drows, w))
        args = [fields, len(self.specs), C.c_void_p(ch.ptr), Cn, L, T, M, C.c_void_p(bad.ptr)]
        if dev is None:
            rc = lib.lsm_host_gather_chunks(*args)
        else:
            rc = lib.lsm_buffer_gather_chunks(*args, _stream(dev))
        assert rc == expect_rc, lib.lsm_recurrent_last_error()
        _sync(dev)
        out = [read_destination(d, s["kind"]).reshape(drows, w) for (d, drows, w), s in zip(dsts, self.specs)]
        return out, int(bad.read().view(np.int64)[0])

    def model(self, chunks, L, T, M):
        want = []
        for s in self.specs:
            if s["kind"] == "rows":
                want.append(rcm.gather_rows(s["src"], chunks, L, T, M))
            elif s["kind"] == "first":
                want.append(rcm.gather_first(s["src"], chunks, L, T, M))
            else:
                g = rcm.gather_compact_adj(s["A"], s["masks"], chunks, L, T, M, s["N"])
                want.append(g.view(np.int32).reshape(g.shape[0], -1))
        return want


def run_fixture(lib, specs, chunks, L, T, M, device=None):
    """The fixture's 17 fields in two calls (16 fields at most per call). Returns (outputs, bad)."""
    out, bad = [], 0
    for part in (specs[:capi.LSM_CHUNK_MAX_FIELDS], specs[capi.LSM_CHUNK_MAX_FIELDS:]):
        got, b = ChunkSources(part, device).run(lib, chunks, L, T, M)
        out += got
        bad |= b
    return out, bad


def fixture_specs(z):
    """The fixture's buffer arrays as gather fields (rows 0 .. T-1 of each), in the generator's yield
    order, plus a compact restatement of adj: the table with inf and non-zero entries wherever every
    agent of the env has the row's or the column's bit set (a select gives 0 there, a product would
    not)."""
    T, M, n, N, E = z["T"], z["M"], z["n"], z["N"], z["E"]
    specs, names = [], []
    for nm in rcm.NAMES:
        src = words(z["in_" + nm][:T], T * M)
        specs.append(dict(kind="first" if nm in rcm.FIRST else "rows", src=src))
        names.append(nm)
    bits = z["adj_bits"][:T]                          # [T, n, N, E]
    common = bits.all(axis=2)                         # [T, n, E]
    under = common[:, :, :, None] | common[:, :, None, :]
    assert under.any()
    poison = np.where((np.arange(E)[:, None] + np.arange(E)[None, :]) % 2 == 0, np.float32(np.inf), np.float32(7.5))
    A = np.where(under, poison, z["adj_table"][:T]).astype(np.float32).reshape(T * n, E, E)
    specs.append(dict(kind="compact", A=A, masks=rcm.pack_bits(bits.reshape(T * M, E)), N=N))
    names.append("adj")
    return specs, names


def fixture_batch(z, i, name):
    """Minibatch i's array `name` as [rows, words] int32."""
    a = z["b%d_%s" % (i, name)]
    return words(a, a.shape[0])


def copy_rows(lib, srcs, dones, flags, M, device, offs=None):
    """One lsm_buffer_copy_rows launch. srcs: [M, words] int32 arrays. Each destination is the middle
    row of a three-row buffer whose neighbours hold the canary. Returns the destinations [M, words]."""
    offs = offs or [0] * len(srcs)
    copies = (capi.LsmRowCopy * len(srcs))()
    keep, dsts = [], []
    dn = None
    if dones is not None:
        d8 = np.zeros((len(dones) + 3) // 4 * 4, np.uint8)
        d8[:len(dones)] = dones
        dn = Placed(d8.view(np.int32), 0, device)
    for c, s, fl, off in zip(copies, srcs, flags, offs):
        src = Placed(s, off, device)
        n = s.size
        buf = Placed(np.full(3 * n, CANARY, dtype=np.int32), off, device)
        c.src, c.dst, c.row_bytes, c.zero_on_done = src.ptr, buf.ptr + 4 * n, 4 * s.shape[1], int(fl)
        keep.append(src)
        dsts.append((buf, n, s.shape))
    rc = lib.lsm_buffer_copy_rows(copies, len(srcs), C.c_void_p(dn.ptr) if dn else None, M, _stream(device))
    assert rc == 0, lib.lsm_recurrent_last_error()
    _sync(device)
    out = []
    for buf, n, shape in dsts:
        a = buf.read()
        assert (a[:n] == CANARY).all() and (a[2 * n:] == CANARY).all(), "a neighbouring buffer row was written"
        out.append(a[n:2 * n].reshape(shape).copy())
    return out
