"""CPU tests of the graph encoder's backward pass (include/lsm_gnn_backward.h): the header and its exports, the
float64 yardstick (tests/gnn_backward_model.py, torch.autograd over the edge-list formulas) pinned to
gnn_model.nodes64, lsm_host_gnn_backward -- the per-graph text the kernel runs, with the kernel's slabs -- against
it within the tolerance measured per case and gradient tensor (4 * e32 + 4 * 2^-23 * s), the structure cases, bad
inputs, slab boundaries, launch plans and the argument refusals (which return before any launch or write, so
they need no device)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gnn_abi as ga
import gnn_backward_cases as bc
import gnn_model as gm
import recurrent_abi as ra
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_gnn_backward.h")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


# ---- the ABI ----------------------------------------------------------------------------------------------------

def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    text = open(HDR).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_GNN_BACKWARD) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE, capi.EXPORTED_LOSS,
                  capi.EXPORTED_BACKWARD):
        assert not declared & set(other)
    body = hdr[hdr.index("typedef struct lsm_gnn_bwd_io"):hdr.index("} lsm_gnn_bwd_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmGnnBwdIo._fields_]
    body = hdr[hdr.index("typedef struct lsm_gnn_bwd_launch_plan"):hdr.index("} lsm_gnn_bwd_launch_plan")]
    fields = [n for decl in re.findall(r"int(?:32|64)_t\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in capi.LsmGnnBwdLaunchPlan._fields_]
    assert int(re.search(r"#define LSM_GNN_BWD_SLAB (\d+)", text).group(1)) == capi.LSM_GNN_BWD_SLAB


def test_the_forward_text_is_the_shared_one(lib):
    """The backward recomputes the forward with csrc/lsm_gnn_tile.h's graph_forward: neither unit holds a copy,
    and the rollout's build id does not cover the new files."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_gnn_backward.hip", "lsm_gnn_backward.h", "lsm_gnn_tile.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    shared = open(os.path.join(build.CSRC, "lsm_gnn_tile.h")).read()
    assert "void graph_forward(" in shared and "struct NoSaves" in shared
    for unit in ("lsm_gnn.hip", "lsm_gnn_backward.hip"):
        src = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "lsm_gnn_tile.h"' in src and "void graph_forward(" not in src and "expf(mx - a)" not in src
        assert "lsm_gnn_tile.h" in build.UNITS[unit]
        assert "atomic" not in src.split("#include", 1)[1]
    assert "graph_forward<HP, CP, Saver>(" in open(os.path.join(build.CSRC, "lsm_gnn_backward.hip")).read()


def test_workspace_bytes(lib):
    f = lambda cfg, B, E: bc.ws_bytes(cfg, B, E)
    cfg, S = bc.DEFAULT, bc.SLAB
    nconv = int(lib.lsm_gnn_weights_floats(cfg.struct())) - bc.conv0(cfg)
    assert nconv == 8304
    assert f(cfg, 0, 24) == 0 and f(cfg, -1, 24) == 0 and f(cfg, 1, 0) == 0 and f(cfg, 1, 257) == 0
    assert f(cfg, 1, 24) == 8 * nconv == f(cfg, S, 24) and f(cfg, S + 1, 24) == 16 * nconv
    assert f(cfg, 5 * 10 ** 5, 24) == 8 * nconv * ((5 * 10 ** 5 + S - 1) // S)
    sizes = [f(cfg, B, 24) for B in range(0, 3 * S + 2, 37)]
    assert sizes == sorted(sizes)
    assert f(cfg, 1, bc.largest_E(cfg) + 1) == 0 and f(dataclasses.replace(cfg, H=5), 1, 24) == 0
    p = bc.plan(cfg, S + 1, 24)[0]
    assert p["ws_bytes"] == 16 * nconv and p["slabs"] == 2 and p["acc_lds"] == 0


def test_limits():
    """Every config of gnn_cases.OPTIONS is accepted at E <= 65 and the defaults at E <= 64 (BASELINE config 4's
    graph has E = 48); beyond the largest E the refusal carries the figures."""
    import gnn_cases as gc
    for name, kw in gc.OPTIONS.items():
        cfg = dataclasses.replace(bc.DEFAULT, **kw)
        for E in (1, 24, 48, 64, 65):
            p, why = bc.plan(cfg, 5, E)
            assert p is not None and p["lds_bytes"] <= 163840 and p["G"] >= 1, (name, E, why)
    E = bc.largest_E(bc.DEFAULT)
    assert E >= 64
    p, why = bc.plan(bc.DEFAULT, 1, E + 1)
    assert p is None and why.startswith("gnn backward: ") and str(E + 1) in why and "163840" in why
    for E in (1, 24, 33, 65):
        p = bc.plan(bc.DEFAULT, 1, E)[0]
        assert p["TS"] == max(32, 1 << (E - 1).bit_length()) and p["fast"] == 1 and p["G"] <= 256 // p["TS"]
    assert bc.plan(dataclasses.replace(bc.DEFAULT, C=12), 1, 24)[0]["fast"] == 0
    assert bc.plan(bc.DEFAULT, 5, 24, N=2, masked=True)[0] is None and bc.plan(bc.DEFAULT, 4, 24, N=2, masked=True)[0]


# ---- the yardstick itself -----------------------------------------------------------------------------------

def _all_cases():
    cases = [(bc.shape_case, (E, w)) for E in bc.SHAPE_E for w in range(3)]
    cases += [(bc.option_case, (n,)) for n in bc.OPTION_NAMES]
    cases += [(bc.readout_case, (a,)) for a in ("node", "global_mean", "global_max", "global_add")]
    cases += [(bc.structure_case, ()), (bc.max_E_case, ())] + [(bc.slab_case, (B,)) for B in bc.SLAB_B]
    return cases


ALL = _all_cases()
IDS = ["%s%s" % (f.__name__, a) for f, a in ALL]


@pytest.mark.parametrize("make,args", ALL, ids=IDS)
def test_model_is_pinned_to_the_forward_yardstick(make, args):
    """The float64 model's forward equals gnn_model.nodes64 to 1e-12 relative, and the case found a seed."""
    case = make(*args)
    t = case.truth
    if case.B > 16:
        sel = np.r_[0:8, case.B - 8:case.B]     # nodes64 loops in Python: the slab cases pin their ends
    else:
        sel = np.arange(case.B)
    with np.errstate(all="ignore"):
        n64 = gm.nodes64(case.cfg, case.sd, case.x[sel], case.full[sel])
    scale = max(1.0, float(np.abs(n64).max()))
    assert np.abs(t.r64.nodes[sel] - n64).max() <= 1e-12 * scale
    assert t.why_not is None and case.seed < bc.SEEDS


# ---- the host entry point against the model ------------------------------------------------------------------

@pytest.mark.parametrize("make,args", ALL, ids=IDS)
def test_host_matches_model(lib, make, args):
    bc.check(lib, make(*args))


def test_plan_cases_on_the_host(lib):
    sizes = bc.plan_sizes()
    assert len(sizes) >= 4 and {k[0] for k in sizes} == {32, 64, 128} and {k[2] for k in sizes} == {0, 1}
    for key in sizes:
        case = bc.plan_case(key)
        assert bc.plan_key(bc.plan(case.cfg, case.B, case.E)[0]) == key
        bc.check(lib, case, layouts=("reference",))


def test_largest_E_and_the_refusal_beyond(lib):
    case = bc.max_E_case()
    E = case.E + 1
    x, table, bits = gm.random_graphs(1, E, case.cfg.F, seed=1)
    src = ga.sources(table, bits, 1, None)["reference"]
    r = bc.call(lib, case.cfg, case.blob, x, src, None, np.zeros((1, case.cfg.out_dim), np.float32), expect_rc=1)
    assert "bytes of LDS per graph" in r["err"]


def test_structure(lib):
    bc.structure_checks(lib)


def test_bad_inputs(lib):
    bc.bad_input_checks(lib)


def test_ego_only_is_ignored(lib):
    case = bc.shape_case(24, 1)
    src = case.sources()["compact"]
    a = bc.call(lib, case.cfg, case.blob, case.x, src, case.agent_id, case.dout)
    b = bc.call(lib, dataclasses.replace(case.cfg, ego_only=True), case.blob, case.x, src, case.agent_id, case.dout)
    np.testing.assert_array_equal(a["dweights"].view(np.int32), b["dweights"].view(np.int32))
    np.testing.assert_array_equal(a["dh0"].view(np.int32), b["dh0"].view(np.int32))


def test_dweights_is_overwritten(lib):
    case = bc.shape_case(3, 1)
    src = case.sources()["reference"]
    n = case.blob.size
    garbage = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
    a = bc.call(lib, case.cfg, case.blob, case.x, src, case.agent_id, case.dout, fill=garbage)
    b = bc.call(lib, case.cfg, case.blob, case.x, src, case.agent_id, case.dout, fill=~garbage)
    c = bc.call(lib, case.cfg, case.blob, case.x, src, case.agent_id, case.dout, want_dh0=False)
    for o in (b, c):
        np.testing.assert_array_equal(a["dweights"].view(np.int32), o["dweights"].view(np.int32))
    assert not a["dweights"][:bc.conv0(case.cfg)].view(np.int32).any()


def test_slabs_change_nothing_but_the_grouping(lib):
    """The first LSM_GNN_BWD_SLAB graphs of the larger cases are the smaller case's inputs when seeds agree; here:
    a call on 2 * SLAB + 3 graphs equals, to float64 rounding, the sum of calls on its slabs, and each slab's call
    is bit-equal to itself run alone."""
    case = bc.slab_case(2 * bc.SLAB + 3)
    src = case.sources()["reference"]
    whole = bc.call(lib, case.cfg, case.blob, case.x, src, None, case.dout)
    parts = []
    for lo in range(0, case.B, bc.SLAB):
        hi = min(lo + bc.SLAB, case.B)
        s = ga.dense_sources(case.full[lo:hi], None)["reference"]
        parts.append(bc.call(lib, case.cfg, case.blob, case.x[lo:hi], s, None, case.dout[lo:hi])["dweights"])
    want = np.sum(np.asarray(parts, dtype=np.float64), axis=0)
    got = whole["dweights"].astype(np.float64)
    # each part was rounded to float32 once (2^-24 relative each), the whole once
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(np.asarray(parts)).max()


# ---- refusals -----------------------------------------------------------------------------------------------------

def test_refusals(lib):
    case = bc.shape_case(3, 1)
    cfg, blob, x, ids, dout = case.cfg, case.blob, case.x, case.agent_id, case.dout
    srcs = case.sources()
    src, cmp_ = srcs["reference"], srcs["compact"]
    run = lambda **kw: bc.call(lib, kw.pop("cfg", cfg), blob, x, kw.pop("src", src), kw.pop("ids", ids), dout,
                               expect_rc=1, **kw)["err"]
    # null pointers
    assert "weights is null" in run(over=dict(weights=None))
    assert "io is null" in run(over=dict(io=None))
    for f in ("dweights", "workspace"):
        assert "is null" in run(io_over={f: None})
    for f in ("node_obs", "adj", "dout"):
        assert "is null" in run(io_over={f: None})
    assert "agent_id" in run(ids=None)
    # misalignment
    for f, by in (("node_obs", 2), ("adj", 2), ("dout", 2), ("dweights", 2), ("dh0", 2), ("workspace", 4),
                  ("agent_id", 4), ("bad", 4)):
        assert "misaligned" in run(io_over={f: (lambda fields, f=f, by=by: fields[f].value + by)}), f
    assert "misaligned" in run(src=cmp_, io_over={"masks": lambda fields: fields["masks"].value + 4})
    # sizes outside the limits
    assert "E must be" in run(over=dict(E=0)) and "E must be" in run(over=dict(E=257))
    assert "B < 0" in run(over=dict(B=-1)) and "INT32_MAX" in run(over=dict(B=2 ** 31))
    assert "H must be" in run(cfg=dataclasses.replace(cfg, H=5))
    assert "unknown aggregation" in run(cfg=_with_aggr_code(cfg, 7))
    assert "bytes of LDS per graph" in run(over=dict(E=bc.largest_E(cfg) + 1))
    # the compact layout
    assert "multiple of N" in run(src=cmp_, over=dict(N=2)) and "multiple of N" in run(src=cmp_, over=dict(N=0))
    # overlaps: an output on an input, two outputs on each other
    assert "overlaps an input" in run(io_over={"dweights": lambda f: f["dout"].value})
    assert "overlaps an input" in run(io_over={"dh0": lambda f: f["node_obs"].value + 8})
    assert "overlaps an input" in run(io_over={"workspace": lambda f: f["adj"].value})
    assert "overlaps an input" in run(io_over={"bad": lambda f: f["agent_id"].value})
    assert "outputs overlap" in run(io_over={"dh0": lambda f: f["dweights"].value + 16})
    assert "outputs overlap" in run(io_over={"workspace": lambda f: f["dweights"].value + 8})
    assert "outputs overlap" in run(io_over={"bad": lambda f: f["workspace"].value})
    # the plan's own null
    assert lib.lsm_gnn_backward_plan(cfg.struct(), 1, 3, 1, 0, None) == 1
    assert lib.lsm_gnn_backward_last_error().decode().startswith("gnn backward: ")


class _Coded:
    """A config whose struct() carries an aggregation code no name maps to."""

    def __init__(self, cfg, code):
        self._cfg, self._code = cfg, code

    def __getattr__(self, k):
        return getattr(self._cfg, k)

    def struct(self):
        s = self._cfg.struct()
        s.aggr = self._code
        return s


def _with_aggr_code(cfg, code):
    return _Coded(cfg, code)


def test_B_zero_writes_nothing(lib):
    case = bc.shape_case(3, 1)
    import mb_edges_abi as mb
    src = mb.Source(np.zeros((0, 3, 3), np.float32))
    r = bc.call(lib, case.cfg, case.blob, np.zeros((0, 3, case.cfg.F), np.float32), src, np.zeros(0, np.int64),
                np.zeros((0, case.cfg.out_dim), np.float32))
    assert r["bad"] == 0
