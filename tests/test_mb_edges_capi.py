"""CPU tests of the minibatch-edges ABI (include/lsm_minibatch_edges.h): the header and its exports,
lsm_host_mb_edges -- the source-row function and the per-element mask / nonzero text the kernels run --
against oracle/process_adj.py on the adjacency the reference's own recurrent_generator yielded
(tests/golden/recurrent/) and on numpy-built dense matrices, out-of-range ids, and the argument refusals
(which return before any launch or write, so they need no device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mb_edges_abi as mb
import recurrent_abi as ra
from lsm import capi
from oracle.process_adj import process_adj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_minibatch_edges.h")
LAYOUTS = ("reference", "compact")


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
    assert declared == set(capi.EXPORTED_MB_EDGES) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT):
        assert not declared & set(other)
    assert "lsm_mb_edges.hip" in build.UNITS
    for field in ("adj", "masks", "E", "N", "rows", "kind", "ids", "count", "L", "T", "M"):
        assert re.search(r"\b%s\b" % field, hdr[hdr.index("typedef struct lsm_mb_graphs"):hdr.index("} lsm_mb_graphs")])
        assert hasattr(capi.LsmMbGraphs, field)


@pytest.mark.parametrize("name", ra.fixtures())
def test_host_chunks_match_the_reference_generator(lib, name):
    z = ra.load_fixture(name)
    T, M, L, mbs = z["T"], z["M"], z["L"], z["mb"]
    srcs = mb.fixture_sources(z)
    for i in range(z["num_mini_batch"]):
        chunks = z["perm"][i * mbs:(i + 1) * mbs]
        want_ei, want_ea = process_adj(z["b%d_adj" % i])   # what the reference's generator yielded
        assert want_ea.shape[0] > 0
        for layout in LAYOUTS:
            ei, ea, nnz, bad = mb.run_host(lib, srcs[layout], chunks, (L, T, M), cap=want_ea.shape[0])
            assert nnz == want_ea.shape[0] and bad == 0
            mb.assert_edges(ei, ea, want_ei, want_ea, (name, i, layout))
            # the numpy statement of the same minibatch agrees with the fixture
            mei, mea, _ = mb.expected(srcs[layout].full, chunks, (L, T, M))
            mb.assert_edges(mei, mea, want_ei, want_ea, (name, i, "model"))


@pytest.mark.parametrize("name", ra.fixtures())
def test_host_indices_match_numpy(lib, name):
    z = ra.load_fixture(name)
    rows = z["T"] * z["M"]
    srcs = mb.fixture_sources(z)
    perm = np.random.default_rng(rows).permutation(rows)
    size = rows // 4
    for i in range(4):
        ids = perm[i * size:(i + 1) * size]
        want_ei, want_ea = process_adj(srcs["reference"].full[ids])
        for layout in LAYOUTS:
            ei, ea, nnz, bad = mb.run_host(lib, srcs[layout], ids, None, cap=want_ea.shape[0])
            assert nnz == want_ea.shape[0] and bad == 0
            mb.assert_edges(ei, ea, want_ei, want_ea, (name, i, layout))


@pytest.fixture(scope="module")
def synthetic():
    return {E: mb.synthetic(E) for E in mb.SYN_E}


@pytest.mark.parametrize("case", sorted(mb.SYN_CASES))
@pytest.mark.parametrize("E", mb.SYN_E)
def test_host_synthetic(lib, synthetic, E, case):
    ids, chunks = mb.syn_case(case)
    srcs = synthetic[E]
    want_ei, want_ea, off = mb.expected(srcs["reference"].full, ids, chunks)
    assert len(off) - 1 == mb.graph_count(ids, chunks) == int(case.lstrip("idxchunk"))
    for layout in LAYOUTS:
        ei, ea, nnz, bad = mb.run_host(lib, srcs[layout], ids, chunks, cap=want_ea.shape[0])
        assert nnz == want_ea.shape[0] and bad == 0
        mb.assert_edges(ei, ea, want_ei, want_ea, (E, case, layout))


def test_host_synthetic_covers_the_edge_cases(synthetic):
    """The expectation itself: empty and full graphs, NaN edges and -0.0 non-edges occur in the cases."""
    full = synthetic[66]["reference"].full
    ids, chunks = mb.syn_case("idx9")
    ei, ea, off = mb.expected(full, ids, chunks)
    per = np.diff(off)
    assert (per == 0).any() and (per == 66 * 66).any() and np.isnan(ea).any()
    d = mb.dense(full, mb.graph_rows(ids, 12, chunks))
    assert (np.signbit(d) & (d == 0)).any() and len(set(ids.tolist())) < len(ids)


def test_host_empty_minibatch_and_small_cap(lib, synthetic):
    src = synthetic[24]["compact"]
    ei, ea, nnz, bad = mb.run_host(lib, src, [], None, cap=3)
    assert nnz == 0 and bad == 0 and ei.shape == (2, 0)
    ei, ea, nnz, bad = mb.run_host(lib, src, [], (3, mb.SYN_T, 4), cap=0)
    assert nnz == 0 and bad == 0
    ids, chunks = mb.syn_case("chunk9")
    want = mb.expected(src.full, ids, chunks)[1].shape[0]
    ei, ea, nnz, bad = mb.run_host(lib, src, ids, chunks, cap=want - 1)   # run_host: nothing was written
    assert nnz == want and ei.shape == (2, 0)
    ei, ea, nnz, bad = mb.run_host(lib, src, ids, chunks, cap=want + 5)   # a larger cap: [2][nnz] packed
    mb.assert_edges(ei, ea, *mb.expected(src.full, ids, chunks)[:2])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_host_bad_ids(lib, synthetic, layout):
    src = synthetic[24][layout]
    E, rows = 24, 12
    for chunks, limit in ((None, rows), ((3, mb.SYN_T, 4), rows // 3)):
        ids = np.array([2, -1, 1, limit, 2 ** 40, limit - 1, 2], dtype=np.int64)
        steps = chunks[0] if chunks else 1
        ei, ea, nnz, bad = mb.run_host(lib, src, ids, chunks)
        assert bad == 1
        want_ei, want_ea, off = mb.expected(src.full, ids, chunks)
        mb.assert_edges(ei, ea, want_ei, want_ea, (layout, chunks))
        per = np.diff(off).reshape(steps, len(ids))
        assert (per[:, [1, 3, 4]] == 0).all() and per[:, [0, 5, 6]].any()
        # the other graphs keep their g * E node offsets
        graphs = np.unique(ei[0] // E)
        assert set(graphs) == {g for g in range(steps * len(ids)) if per.reshape(-1)[g]}
        np.testing.assert_array_equal(ei[0] // E, ei[1] // E)
        good = ids[[0, 2, 5, 6]]
        assert mb.run_host(lib, src, good, chunks)[3] == 0


# ---- argument refusals: nonzero and a text, before any launch or write -----------------------------

REFUSALS = {
    "null adj": dict(d=dict(adj=None)),
    "null ids": dict(d=dict(ids=None)),
    "E = 0": dict(d=dict(E=0)),
    "E = 257": dict(d=dict(E=257)),
    "compact rows % N": dict(d=dict(N=5)),
    "compact N = 0": dict(d=dict(N=0)),
    "G = 2^31": dict(d=dict(count=2 ** 31)),
    "chunks G = 2^31": dict(chunks=True, d=dict(count=2 ** 29, L=4)),
    "rows = 2^32": dict(d=dict(rows=2 ** 32)),
    "chunks L = 0": dict(chunks=True, d=dict(L=0)),
    "chunks L > rows": dict(chunks=True, d=dict(L=13)),
    "chunks T * M != rows": dict(chunks=True, d=dict(T=4)),
    "count < 0": dict(d=dict(count=-1)),
    "unknown kind": dict(d=dict(kind=2)),
    "null offsets": dict(only=("count", "emit"), offsets=None),
    "null workspace": dict(only=("count",), workspace=None),
    "workspace too small": dict(only=("count",), short=True),
    "null edge_index": dict(only=("emit", "emit_dev", "host"), edge_index=None),
    "null edge_attr": dict(only=("emit", "emit_dev", "host"), edge_attr=None),
    "cap < 0": dict(only=("emit_dev", "host"), cap=-1),
    "null nnz_out": dict(only=("host",), nnz_out=None),
}


ENTRIES = ("count", "emit", "emit_dev", "host")


@pytest.mark.parametrize("entry,what", [(e, w) for w in sorted(REFUSALS) for e in REFUSALS[w].get("only", ENTRIES)])
def test_refusals(lib, entry, what):
    spec = REFUSALS[what]
    src = mb.synthetic(24)["compact"]
    ids = ra.Placed(np.zeros(8, np.int64).view(np.int32), 0)
    chunks = (3, mb.SYN_T, 4) if spec.get("chunks") else None
    d = src.desc(ids.ptr, 3, chunks, **spec.get("d", {}))
    # every destination sits in one canaried block: offsets [10], edge_index [2 * 8], edge_attr [8], nnz, bad
    block = np.full(64, mb.CANARY64, dtype=np.int64)
    at = lambda k: C.c_void_p(block.ctypes.data + 8 * k)
    nbytes = int(lib.lsm_mb_edges_workspace_bytes(9))
    assert nbytes >= 9 * 8
    ws = np.full(nbytes // 8 + 1, mb.CANARY64, dtype=np.int64)
    offsets = at(4) if "offsets" not in spec else None
    edge_index = at(16) if "edge_index" not in spec else None
    edge_attr = at(36) if "edge_attr" not in spec else None
    nnz_out = at(44) if "nnz_out" not in spec else None
    bad = at(46)
    cap = spec.get("cap", 8)
    if entry == "count":
        rc = lib.lsm_mb_edges_count(d, offsets, None if "workspace" in spec else C.c_void_p(ws.ctypes.data),
                                    8 if spec.get("short") else nbytes, bad, None)
    elif entry == "emit":
        rc = lib.lsm_mb_edges_emit(d, offsets, 8, 8, edge_index, edge_attr, None)
    elif entry == "emit_dev":
        rc = lib.lsm_mb_edges_emit(d, offsets, -1, cap, edge_index, edge_attr, None)
    else:
        rc = lib.lsm_host_mb_edges(d, cap, edge_index, edge_attr, nnz_out, bad)
    assert rc != 0
    assert lib.lsm_mb_edges_last_error().decode().startswith("mb_edges: ")
    assert len(lib.lsm_mb_edges_last_error().decode()) > len("mb_edges: ")
    assert (block == mb.CANARY64).all() and (ws == mb.CANARY64).all()   # nothing was written
