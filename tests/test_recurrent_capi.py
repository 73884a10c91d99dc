"""CPU tests of the recurrent hand-off ABI (include/lsm_recurrent.h): the header and its exports,
lsm_host_gather_chunks -- the text the kernel runs -- against every minibatch the reference's
recurrent_generator yielded (tests/golden/make_recurrent_golden.py) bit for bit, the numpy model's
addressing against the reference's (env, agent, t) view, out-of-range chunk ids, and the argument
refusals (which return before any launch, so they need no device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import recurrent_abi as ra
import recurrent_model as rcm
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_recurrent.h")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    from lsm import build
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_RECURRENT) and len(declared) == 4
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert not declared & set(capi.EXPORTED)
    assert not declared & set(capi.EXPORTED_LEARNER)
    assert "lsm_chunks.hip" in build.UNITS


def test_fixture_set():
    names = ra.fixtures()
    zs = [ra.load_fixture(n) for n in names]
    assert {(z["T"], z["n"], z["N"], z["E"]) for z in zs} == {(6, 3, 5, 4)}
    assert {z["L"] for z in zs} == {1, 3, 4, 6}
    assert any(not z["use_centralized_V"] for z in zs)
    for z in zs:
        T, M, L, k = z["T"], z["M"], z["L"], z["num_mini_batch"]
        assert len(z["perm"]) == rcm.data_chunks(L, T, M)
        np.testing.assert_array_equal(np.sort(z["perm"]), np.arange(len(z["perm"])))
        assert 0.15 < (z["in_masks"] == 0).mean() < 0.45 and 0.08 < (z["in_active_masks"] == 0).mean() < 0.35
        used = z["perm"][:z["mb"] * k]
        straddles = ((used * L) % T + L > T).any()
        if L == 4 and z["recurrent_N"] == 2:
            assert straddles and (T * M) % L != 0 and z["num_mini_batch"] == 2
            assert z["b0_rnn_states"].shape == (z["mb"], 2, 4)
        if L in (1, 3, 6):
            assert not straddles
        # the compact statement the fixture's adj was built from
        bits = z["adj_bits"]
        drop = bits[..., :, None] | bits[..., None, :]
        np.testing.assert_array_equal(z["in_adj"], np.where(drop, np.float32(0), z["adj_table"][:, :, None]))


@pytest.mark.parametrize("name", ra.fixtures())
def test_model_matches_fixture(name):
    z = ra.load_fixture(name)
    T, M, L, mb = z["T"], z["M"], z["L"], z["mb"]
    specs, names = ra.fixture_specs(z)
    src = ra.ChunkSources(specs)
    for i in range(z["num_mini_batch"]):
        chunks = z["perm"][i * mb:(i + 1) * mb]
        for w, nm in zip(src.model(chunks, L, T, M), names):
            np.testing.assert_array_equal(w, ra.fixture_batch(z, i, nm), err_msg="%s batch %d" % (nm, i))


@pytest.mark.parametrize("name", ra.fixtures())
def test_host_gather_chunks_matches_fixture(lib, name):
    z = ra.load_fixture(name)
    T, M, L, mb = z["T"], z["M"], z["L"], z["mb"]
    specs, names = ra.fixture_specs(z)
    assert names[-1] == "adj" and specs[-1]["kind"] == "compact" and np.isinf(specs[-1]["A"]).any()
    for i in range(z["num_mini_batch"]):
        chunks = z["perm"][i * mb:(i + 1) * mb]
        got, bad = ra.run_fixture(lib, specs, chunks, L, T, M)   # checks the canaries around every destination
        assert bad == 0
        for g, nm, s in zip(got, names, specs):
            want = ra.fixture_batch(z, i, nm)
            assert g.shape == want.shape, nm
            np.testing.assert_array_equal(g, want, err_msg="%s (%s) batch %d" % (nm, s["kind"], i))


def test_model_chunk_rows_is_the_cast_view():
    rng = np.random.default_rng(0)
    shapes = [(6, 15, 4), (6, 15, 3), (5, 7, 9), (3, 4, 12), (1, 6, 4), (7, 1, 3), (4, 5, 1), (4, 5, 20)]
    shapes += [tuple(int(x) for x in rng.integers(1, 12, 3)) for _ in range(30)]
    seen_longer = False
    for T, M, L in shapes:
        L = min(L, T * M)
        seen_longer |= L > T
        nch = rcm.data_chunks(L, T, M)
        src = rng.integers(0, 2 ** 31, (T * M, 3)).astype(np.int32)
        view = rcm.cast_view(src, T, M)            # row f = (column f // T, time f % T)
        chunks = rng.permutation(nch)[:max(1, nch // 2)]
        rows = rcm.chunk_rows(chunks, L, T, M)
        want = np.stack([view[c * L:(c + 1) * L] for c in chunks], axis=1).reshape(L * len(chunks), 3)
        np.testing.assert_array_equal(src[rows], want, err_msg=str((T, M, L)))
        np.testing.assert_array_equal(src[rcm.first_rows(chunks, L, T, M)], view[chunks * L])
    assert seen_longer


def _synthetic(T, M, N, seed=3):
    rng = np.random.default_rng(seed)
    rows = T * M
    specs = []
    for w, kind, off in ((1, "rows", 0), (6, "rows", 0), (4, "rows", 0), (4, "rows", 1), (12, "first", 0),
                         (3, "first", 0)):
        specs.append(dict(kind=kind, off=off, src=rng.integers(-2 ** 31, 2 ** 31, (rows, w)).astype(np.int32)))
    for E in (5, 8):
        A = rng.normal(0, 1, (rows // N, E, E)).astype(np.float32)
        A[A == 0] = 1.0
        A[0, 0, 0] = np.inf
        bits = rng.random((rows, E)) < 0.25
        bits[0, 0] = True
        specs.append(dict(kind="compact", A=A, masks=rcm.pack_bits(bits), N=N))
    return specs


@pytest.mark.parametrize("T,M,N,L,Cn", [(6, 15, 5, 4, 9), (5, 8, 2, 7, 3), (3, 4, 4, 12, 1), (4, 6, 3, 1, 24)])
def test_host_gather_chunks_matches_model(lib, T, M, N, L, Cn):
    rng = np.random.default_rng(L)
    src = ra.ChunkSources(_synthetic(T, M, N))
    chunks = rng.integers(0, rcm.data_chunks(L, T, M), Cn)   # duplicates allowed at the ABI level
    chunks[0] = rcm.data_chunks(L, T, M) - 1
    got, bad = src.run(lib, chunks, L, T, M)
    assert bad == 0
    for g, w, s in zip(got, src.model(chunks, L, T, M), src.specs):
        np.testing.assert_array_equal(g, w, err_msg=s["kind"])


def test_host_gather_chunks_bad_ids(lib):
    T, M, N, L = 6, 15, 5, 4
    nch = rcm.data_chunks(L, T, M)
    src = ra.ChunkSources(_synthetic(T, M, N))
    chunks = np.array([3, -1, 0, nch, 2 ** 40, nch - 1, 5], dtype=np.int64)
    got, bad = src.run(lib, chunks, L, T, M)
    assert bad == 1
    Cn = len(chunks)
    for g, w, s in zip(got, src.model(chunks, L, T, M), src.specs):
        np.testing.assert_array_equal(g, w, err_msg=s["kind"])
        steps = 1 if s["kind"] == "first" else L
        for b in (1, 3, 4):
            assert (g.reshape(steps, Cn, -1)[:, b] == 0).all(), s["kind"]
        assert g.reshape(steps, Cn, -1)[:, [0, 2, 5, 6]].any()
    assert src.run(lib, chunks[[0, 2, 5]], L, T, M)[1] == 0


# ---- argument refusals: nonzero and a text, before any launch or write -----------------------------

def _field(**kw):
    buf = np.zeros(64, np.uint64)
    base = dict(kind=capi.LSM_CHUNK_ROWS, src=buf.ctypes.data, dst=buf.ctypes.data, row_bytes=16,
                masks=buf.ctypes.data, E=4, N=2)
    base.update(kw)
    f = capi.LsmChunkField(**base)
    f._keep = buf
    return f


_COMPACT = capi.LSM_CHUNK_COMPACT_ADJ
CHUNK_REFUSALS = {
    "null fields": dict(fields=None),
    "no fields": dict(nfields=0),
    "17 fields": dict(nfields=17),
    "null chunks": dict(chunks=None),
    "C = 0": dict(C=0),
    "L = 0": dict(L=0),
    "L > T * M": dict(L=7),
    "T = 0": dict(T=0),
    "M = 0": dict(M=0),
    "T * M = 2^32": dict(T=2 ** 16, M=2 ** 16),
    "null src": dict(field=dict(src=None)),
    "null dst": dict(field=dict(dst=None)),
    "src off by 2": dict(field=dict(src=2)),
    "row_bytes = 0": dict(field=dict(row_bytes=0)),
    "row_bytes = 6": dict(field=dict(row_bytes=6)),
    "first row_bytes = 6": dict(field=dict(kind=capi.LSM_CHUNK_FIRST_ROW, row_bytes=6)),
    "unknown kind": dict(field=dict(kind=7)),
    "compact without masks": dict(field=dict(kind=_COMPACT, masks=None)),
    "compact E = 0": dict(field=dict(kind=_COMPACT, E=0)),
    "compact N = 0": dict(field=dict(kind=_COMPACT, N=0)),
    "compact rows % N": dict(field=dict(kind=_COMPACT, N=4)),
    # the kernel counts copy units in 32 bits
    "2^32 destination rows": dict(C=2 ** 31, L=2, T=2 ** 16, M=2 ** 15),
    "2^32 copy units": dict(C=2 ** 20, L=2, T=2 ** 16, M=2 ** 15, field=dict(row_bytes=2 ** 15)),
}


@pytest.mark.parametrize("entry", ["lsm_buffer_gather_chunks", "lsm_host_gather_chunks"])
@pytest.mark.parametrize("what", sorted(CHUNK_REFUSALS))
def test_gather_chunks_refusals(lib, entry, what):
    spec = CHUNK_REFUSALS[what]
    nfields = spec.get("nfields", 2)
    arr = (capi.LsmChunkField * 17)(*([_field()] * 17))
    keep = _field(**dict(spec.get("field", {})))
    if spec.get("field", {}).get("src") == 2:
        keep.src = keep._keep.ctypes.data + 2
    arr[1] = keep
    idx = np.zeros(4, np.int64)
    bad = np.zeros(1, np.int64)
    fields = None if "fields" in spec else arr
    chunks = None if "chunks" in spec else C.c_void_p(idx.ctypes.data)
    args = [fields, nfields, chunks, spec.get("C", 1), spec.get("L", 2), spec.get("T", 2), spec.get("M", 3),
            C.c_void_p(bad.ctypes.data)]
    if entry == "lsm_buffer_gather_chunks":
        args.append(None)
    assert getattr(lib, entry)(*args) != 0
    assert lib.lsm_recurrent_last_error().decode().startswith("gather_chunks: ")
    assert bad[0] == 0 and not keep._keep.any()   # nothing was written


def _copy(**kw):
    buf = np.zeros(64, np.uint64)
    base = dict(src=buf.ctypes.data, dst=buf.ctypes.data + 256, row_bytes=16, zero_on_done=0)
    base.update(kw)
    c = capi.LsmRowCopy(**base)
    c._keep = buf
    return c


COPY_REFUSALS = {
    "null copies": dict(copies=None),
    "no copies": dict(ncopies=0),
    "9 copies": dict(ncopies=9),
    "M = 0": dict(M=0),
    "null src": dict(copy=dict(src=None)),
    "null dst": dict(copy=dict(dst=None)),
    "row_bytes = 0": dict(copy=dict(row_bytes=0)),
    "row_bytes = 10": dict(copy=dict(row_bytes=10)),
    "zero_on_done without dones": dict(copy=dict(zero_on_done=1)),
    "2^32 copy units": dict(M=2 ** 30, copy=dict(row_bytes=64)),
}


@pytest.mark.parametrize("what", sorted(COPY_REFUSALS))
def test_copy_rows_refusals(lib, what):
    spec = COPY_REFUSALS[what]
    arr = (capi.LsmRowCopy * 9)(*([_copy()] * 9))
    keep = _copy(**spec.get("copy", {}))
    arr[1] = keep
    rc = lib.lsm_buffer_copy_rows(None if "copies" in spec else arr, spec.get("ncopies", 2), None, spec.get("M", 4),
                                  None)
    assert rc != 0
    assert lib.lsm_recurrent_last_error().decode().startswith("copy_rows: ")
