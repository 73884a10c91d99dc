"""CPU tests of the learner hand-off ABI (include/lsm_learner.h): the header and its exports, the
numpy model against the fixtures recorded from the reference (tests/golden/make_returns_golden.py),
lsm_host_compute_returns -- the text the kernel runs -- against every fixture bit for bit, and the
argument refusals (which return before any launch, so they need no device)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import learner_abi as la
import returns_model as rm
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_learner.h")
# lsm.build.build_id() on the parent commit (the step kernels, the host ABI, lsm_rollout.h and the
# compiler flags): this change must not move it, profiles/pmc_traffic.json is keyed by it
PARENT_BUILD_ID = "9a7cc674220ecd51"


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
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_LEARNER)
    assert len(capi.EXPORTED_LEARNER) == 7
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert not set(capi.EXPORTED) & declared


def test_build_id_unchanged():
    from lsm import build
    assert build.build_id() == PARENT_BUILD_ID
    assert "lsm_returns.hip" in build.UNITS and "lsm_gather.hip" in build.UNITS


def test_fixture_set():
    names = la.fixtures()
    combos = {(int(z["use_gae"]), int(z["use_proper_time_limits"]), int(z["use_valuenorm"]))
              for z in map(la.load_fixture, names) if z["T"] == 6}
    assert len(combos) == 8
    assert any(la.load_fixture(n)["T"] == 1 for n in names)
    for n in names:
        z = la.load_fixture(n)
        T = z["T"]
        for k in ("masks", "bad_masks"):
            assert (z[k][T] == 0).any() and (z[k][1] == 0).any() and 0.15 < (z[k] == 0).mean() < 0.45
        assert (z["active_masks"][:-1] == 0).any()
        np.testing.assert_array_equal(z["denorm"], [np.sqrt(z["vn_var"][0]), z["vn_mean"][0]])


def _model_returns(z):
    v = z["value_preds_in"].copy()
    ret = np.full_like(v, la.SENTINEL)
    rm.compute_returns(z["rewards"], v, z["masks"], z["bad_masks"], z["next_value"], z["den"], ret, float(z["gamma"]),
                       float(z["gae_lambda"]), bool(z["use_gae"]), bool(z["use_proper_time_limits"]))
    return ret, v


@pytest.mark.parametrize("name", la.fixtures())
def test_model_matches_fixture(name):
    z = la.load_fixture(name)
    ret, v = _model_returns(z)
    rows = la.written_rows(z["T"], z["use_gae"])
    np.testing.assert_array_equal(la.bits(ret[rows]), la.bits(z["returns"][rows]))
    np.testing.assert_array_equal(la.bits(v), la.bits(z["value_preds_out"]))
    adv = rm.raw_advantages(z["returns"], z["value_preds_out"], z["den"])
    np.testing.assert_array_equal(la.bits(adv), la.bits(z["adv_raw"]))
    active = z["active_masks"][:-1]
    # the reference's own lines restated: bit-equal; float64 statistics: within the float32 tolerance
    np.testing.assert_array_equal(la.bits(rm.reference_advantages(adv, active)), la.bits(z["adv_norm"]))
    st = rm.advantage_stats(adv, active)
    np.testing.assert_allclose(st[:2], [z["adv_mean"], z["adv_std"]], rtol=1e-6)
    np.testing.assert_allclose(rm.normalised_advantages(adv, st), z["adv_norm"], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", la.fixtures())
def test_host_compute_returns_matches_fixture(lib, name):
    z = la.load_fixture(name)
    T, M, gae = z["T"], z["M"], bool(z["use_gae"])
    ret, v = la.compute_returns(lib, z["rewards"], z["value_preds_in"], z["masks"], z["bad_masks"], z["next_value"],
                                z["den"], z["gamma"], z["gae_lambda"], gae, bool(z["use_proper_time_limits"]))
    want = z["returns"].reshape(T + 1, M)
    rows = la.written_rows(T, gae)
    np.testing.assert_array_equal(la.bits(ret[rows]), la.bits(want[rows]))
    np.testing.assert_array_equal(la.bits(v), la.bits(z["value_preds_out"].reshape(T + 1, M)))
    nv = z["next_value"].reshape(M)
    if gae:   # value_preds[T] = next_value, returns[T] not written
        np.testing.assert_array_equal(v[T], nv)
        assert (ret[T] == la.SENTINEL).all()
    else:     # returns[T] = next_value, value_preds untouched
        np.testing.assert_array_equal(ret[T], nv)
        np.testing.assert_array_equal(v, z["value_preds_in"].reshape(T + 1, M))


def test_host_compute_returns_allows_null_bad_masks_unless_proper(lib):
    z = la.load_fixture("t6_gae1_ptl0_vn1")
    a = la.compute_returns(lib, z["rewards"], z["value_preds_in"], z["masks"], None, z["next_value"], z["den"],
                           z["gamma"], z["gae_lambda"], True, False)
    np.testing.assert_array_equal(la.bits(a[0][:6]), la.bits(z["returns"].reshape(7, -1)[:6]))


def test_model_compact_gather_is_a_select():
    """A set bit assigns 0 whatever the table holds: inf under it gives 0, where a product gives NaN."""
    A = np.full((2, 3, 3), np.inf, dtype=np.float32)
    masks = np.array([[0], [0b010], [0], [0b101]], dtype=np.uint64)   # rows = 4 samples, N = 2
    out = rm.gather_compact_adj(A, masks, [1, 0, 3, 9], 2)
    keep = np.ones((3, 3), bool)
    keep[1, :] = keep[:, 1] = False
    np.testing.assert_array_equal(out[0], np.where(keep, np.inf, 0).astype(np.float32))
    assert np.isinf(out[1]).all()
    only = np.zeros((3, 3), np.float32)
    only[1, 1] = np.inf
    np.testing.assert_array_equal(out[2], only)
    assert (out[3] == 0).all()   # index out of range


# ---- argument refusals: nonzero and a text, before any launch ---------------------------------------

def _returns_args(T=2, M=3):
    a = dict(rewards=np.zeros((T, M), np.float32), value_preds=np.zeros((T + 1, M), np.float32),
             masks=np.ones((T + 1, M), np.float32), bad_masks=np.ones((T + 1, M), np.float32),
             next_value=np.zeros(M, np.float32), denorm=np.ones(2, np.float32),
             returns=np.zeros((T + 1, M), np.float32))
    return a, T, M


RETURNS_REFUSALS = [("T", 0), ("M", 0), ("rewards", None), ("value_preds", None), ("masks", None),
                    ("next_value", None), ("returns", None), ("cfg", None), ("bad_masks", None)]


@pytest.mark.parametrize("entry", ["lsm_buffer_compute_returns", "lsm_host_compute_returns"])
@pytest.mark.parametrize("what,value", RETURNS_REFUSALS)
def test_compute_returns_refusals(lib, entry, what, value):
    a, T, M = _returns_args()
    cfg = la.config(0.99, 0.95, True, True)   # proper: bad_masks is required
    if what == "T":
        T = value
    elif what == "M":
        M = value
    elif what != "cfg":
        a[what] = value
    p = lambda k: C.c_void_p(a[k].ctypes.data) if a[k] is not None else None
    args = [p("rewards"), p("value_preds"), p("masks"), p("bad_masks"), p("next_value"), p("denorm"), p("returns"),
            T, M, None if what == "cfg" else C.byref(cfg)]
    if entry == "lsm_buffer_compute_returns":
        args.append(None)
    before = {k: (v.copy() if v is not None else None) for k, v in a.items()}
    assert getattr(lib, entry)(*args) != 0
    assert lib.lsm_returns_last_error().decode().startswith("compute_returns: ")
    for k, v in a.items():   # nothing was written
        if v is not None:
            np.testing.assert_array_equal(v, before[k])


@pytest.mark.parametrize("what", ["count", "returns", "value_preds", "active_masks", "advantages", "stats",
                                  "workspace", "short workspace"])
def test_advantages_refusals(lib, what):
    count = 5000
    need = lib.lsm_buffer_advantages_workspace_bytes(count)
    assert need >= 24 and need % 8 == 0
    x = np.zeros(count, np.float32)
    ws = np.zeros(need // 8, np.float64)
    ptr = {k: C.c_void_p(x.ctypes.data) for k in ("returns", "value_preds", "active_masks", "advantages")}
    ptr["stats"], ptr["workspace"] = C.c_void_p(ws.ctypes.data), C.c_void_p(ws.ctypes.data)
    nbytes = need
    if what == "count":
        count = 0
    elif what == "short workspace":
        nbytes = need - 1
    else:
        ptr[what] = None
    rc = lib.lsm_buffer_advantages(ptr["returns"], ptr["value_preds"], ptr["active_masks"], None, count,
                                   ptr["advantages"], ptr["stats"], ptr["workspace"], nbytes, None)
    assert rc != 0
    assert lib.lsm_returns_last_error().decode().startswith("advantages: ")


def _field(**kw):
    buf = np.zeros(64, np.uint64)
    base = dict(kind=capi.LSM_GATHER_ROWS, src=buf.ctypes.data, dst=buf.ctypes.data, row_bytes=16,
                masks=buf.ctypes.data, E=4, N=2)
    base.update(kw)
    f = capi.LsmGatherField(**base)
    f._keep = buf
    return f


GATHER_REFUSALS = {
    "null fields": dict(fields=None),
    "no fields": dict(nfields=0),
    "17 fields": dict(nfields=17),
    "null indices": dict(indices=None),
    "B = 0": dict(B=0),
    "rows = 0": dict(rows=0),
    "null src": dict(field=dict(src=None)),
    "null dst": dict(field=dict(dst=None)),
    "row_bytes = 0": dict(field=dict(row_bytes=0)),
    "row_bytes = 6": dict(field=dict(row_bytes=6)),
    "unknown kind": dict(field=dict(kind=7)),
    "compact without masks": dict(field=dict(kind=capi.LSM_GATHER_COMPACT_ADJ, masks=None)),
    "compact E = 0": dict(field=dict(kind=capi.LSM_GATHER_COMPACT_ADJ, E=0)),
    "compact N = 0": dict(field=dict(kind=capi.LSM_GATHER_COMPACT_ADJ, N=0)),
    "compact rows % N": dict(field=dict(kind=capi.LSM_GATHER_COMPACT_ADJ, N=4)),
    # the kernel counts copy units and compact rows in 32 bits
    "2^32 copy units": dict(B=2 ** 32),
    "compact rows = 2^32": dict(rows=2 ** 32, field=dict(kind=capi.LSM_GATHER_COMPACT_ADJ)),
}


@pytest.mark.parametrize("what", sorted(GATHER_REFUSALS))
def test_gather_refusals(lib, what):
    spec = GATHER_REFUSALS[what]
    nfields = spec.get("nfields", 2)
    arr = (capi.LsmGatherField * 17)(*([_field()] * 16 + [_field()]))
    keep = [_field(**spec.get("field", {}))]
    arr[1] = keep[0]
    idx = np.zeros(4, np.int64)
    fields = None if "fields" in spec else arr
    indices = None if "indices" in spec else C.c_void_p(idx.ctypes.data)
    rc = lib.lsm_buffer_gather(fields, nfields, indices, spec.get("B", 4), spec.get("rows", 6), None, None)
    assert rc != 0
    assert lib.lsm_gather_last_error().decode().startswith("gather: ")
