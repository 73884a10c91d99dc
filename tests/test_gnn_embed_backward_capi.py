"""CPU tests of EmbedConv's backward pass (include/lsm_gnn_embed_backward.h): the header and its exports, the
float64 yardstick (tests/gnn_embed_backward_model.py, torch.autograd over the edge-list EmbedConv) pinned to
gnn_backward_model's h0, lsm_host_gnn_embed_backward -- the per-graph text the kernel runs, with the kernel's
slabs -- against it within the tolerance measured per case and gradient tensor (4 * e32 + 4 * 2^-23 * s), the
structure cases, linearity in dh0, bad inputs, slab boundaries, launch plans, size limits and the argument
refusals (which return before any launch or write, so they need no device)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import gnn_abi as ga
import gnn_backward_cases as bc
import gnn_backward_model as gbm
import gnn_cases as gc
import gnn_embed_backward_cases as ec
import gnn_model as gm
import recurrent_abi as ra
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_gnn_embed_backward.h")


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
    assert declared == set(capi.EXPORTED_GNN_EMBED_BACKWARD) and len(declared) == 6
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE, capi.EXPORTED_LOSS,
                  capi.EXPORTED_BACKWARD, capi.EXPORTED_GNN_BACKWARD):
        assert not declared & set(other)
    body = hdr[hdr.index("typedef struct lsm_gnn_embed_bwd_io"):hdr.index("} lsm_gnn_embed_bwd_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmGnnEmbedBwdIo._fields_]
    body = hdr[hdr.index("typedef struct lsm_gnn_embed_bwd_launch_plan"):hdr.index("} lsm_gnn_embed_bwd_launch_plan")]
    fields = [n for decl in re.findall(r"int(?:32|64)_t\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in capi.LsmGnnEmbedBwdLaunchPlan._fields_]


def test_the_unit_is_built_apart_and_has_no_atomics(lib):
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_gnn_embed_backward.hip", "lsm_gnn_embed_backward.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    assert "lsm_gnn_tile.h" in build.UNITS["lsm_gnn_embed_backward.hip"]
    src = open(os.path.join(build.CSRC, "lsm_gnn_embed_backward.hip")).read()
    assert "atomic" not in src.split("#include", 1)[1]


def test_embed_floats_and_workspace_bytes(lib):
    cfg, S = ec.DEFAULT, ec.SLAB
    n = int(lib.lsm_gnn_embed_floats(cfg.struct()))
    assert n == ec.embed_floats(cfg) == 536
    assert int(lib.lsm_gnn_embed_floats(dataclasses.replace(cfg, H=5).struct())) == 0
    assert lib.lsm_gnn_embed_backward_last_error().decode().startswith("gnn embed backward: H must be")
    for name, kw in ec.OPTIONS.items():
        c = dataclasses.replace(cfg, **kw)
        assert int(lib.lsm_gnn_embed_floats(c.struct())) == ec.embed_floats(c), name
    f = ec.ws_bytes
    assert f(cfg, 0, 24) == 0 and f(cfg, -1, 24) == 0 and f(cfg, 1, 0) == 0 and f(cfg, 1, 257) == 0
    p = ec.plan(cfg, S + 1, 24)[0]
    per_slab = 8 * n + (0 if p["acc_lds"] else 8 * p["G"] * ((n + 3) // 4 * 4))
    assert p["entries"] == n and p["slabs"] == 2 and p["ws_bytes"] == 2 * per_slab == f(cfg, S + 1, 24)
    assert f(cfg, 1, 24) == per_slab == f(cfg, S, 24)
    sizes = [f(cfg, B, 24) for B in range(0, 3 * S + 2, 37)]
    assert sizes == sorted(sizes)


def test_limits():
    """Every (config, E <= 65) that lsm_gnn_backward_plan accepts is accepted here, over gnn_cases.OPTIONS, the
    plan configs and the widest config; the plan's figures follow the header's formulas; beyond the largest E the
    refusal carries the figures."""
    cfgs = dict(ec.OPTIONS, wide=gc.WIDE, **ec.PLAN_CFGS)
    accepted = 0
    for name, kw in cfgs.items():
        cfg = dataclasses.replace(ec.DEFAULT, **kw)
        for E in range(1, 66):
            p, why = ec.plan(cfg, 5, E)
            if bc.plan(cfg, 5, E)[0] is not None:
                accepted += 1
                assert p is not None, (name, E, why)
            if p is None:
                continue
            S = (cfg.embed_hidden + 3) // 4 * 4 + 4
            n4 = (ec.embed_floats(cfg) + 3) // 4 * 4
            base = 6 * E * S + 4 * ((E + 3) // 4 * 4)
            per = base + (p["adj_lds"] and (E * E + 3) // 4 * 4) + (p["acc_lds"] and 2 * n4)
            assert p["S"] == S and p["per_graph"] == per and p["lds_bytes"] == 4 * per * p["G"] <= 163840
            assert p["TS"] == max(32, 1 << (E - 1).bit_length()) and 1 <= p["G"] <= 256 // p["TS"]
            assert p["G"] == min(256 // p["TS"], 163840 // (4 * base))
            assert p["fast"] == (cfg.embed_hidden == 16)
    assert accepted > 500
    assert ec.largest_E(ec.DEFAULT) == 256 and ec.largest_E(bc.DEFAULT) >= bc.largest_E(bc.DEFAULT)
    cfg = ec.limit_cfg()
    E = ec.largest_E(cfg)
    assert E == 99 and cfg.embed_hidden == 64
    p, why = ec.plan(cfg, 1, E + 1)
    assert p is None and why.startswith("gnn embed backward: ") and str(E + 1) in why and "163840" in why
    assert str(4 * (6 * 100 * 68 + 4 * 100)) in why and "1632" in why
    assert ec.plan(ec.DEFAULT, 5, 24, N=2, masked=True)[0] is None and ec.plan(ec.DEFAULT, 4, 24, N=2, masked=True)[0]


# ---- the yardstick itself -----------------------------------------------------------------------------------

def _all_cases():
    cases = [(ec.shape_case, (E, w)) for E in ec.SHAPE_E for w in range(3)]
    cases += [(ec.option_case, (n,)) for n in ec.OPTION_NAMES]
    cases += [(ec.structure_case, ())] + [(ec.slab_case, (B,)) for B in ec.SLAB_B]
    return cases


ALL = _all_cases()
IDS = ["%s%s" % (f.__name__, a) for f, a in ALL]


@pytest.mark.parametrize("make,args", ALL + [(ec.max_E_case, ())], ids=IDS + ["max_E_case()"])
def test_model_is_pinned_to_the_backward_yardstick(make, args):
    """The float64 model's h0 equals gnn_backward_model.run's to 1e-12, and the case found a seed."""
    case = make(*args)
    cfg = dataclasses.replace(case.cfg, aggr="global_mean")
    with np.errstate(all="ignore"):
        r = gbm.run(cfg, case.sd, case.x, case.full, np.zeros((case.B, cfg.out_dim), np.float32), None, torch.float64)
    scale = max(1.0, float(np.abs(r.h0).max()))
    assert np.abs(case.truth.r64.h0 - r.h0).max() <= 1e-12 * scale
    assert case.truth.why_not is None and case.seed < ec.SEEDS


# ---- the host entry point against the model ------------------------------------------------------------------

@pytest.mark.parametrize("make,args", ALL, ids=IDS)
def test_host_matches_model(lib, make, args):
    ec.check(lib, make(*args))


def test_plan_cases_on_the_host(lib):
    sizes = ec.plan_sizes()
    assert len(sizes) >= 4 and {k[0] for k in sizes} == {32, 64, 128} and {k[2] for k in sizes} == {0, 1}
    assert {k[3] for k in sizes} == {0, 1}     # both accumulator placements occur
    for key in sizes:
        case = ec.plan_case(key)
        assert ec.plan_key(ec.plan(case.cfg, case.B, case.E)[0]) == key
        ec.check(lib, case, layouts=("reference",))


def test_largest_E_and_the_refusal_beyond(lib):
    case = ec.max_E_case()
    ec.check(lib, case, layouts=("reference",))
    E = case.E + 1
    x, table, bits = gm.random_graphs(1, E, case.cfg.F, seed=1)
    src = ga.sources(table, bits, 1, None)["reference"]
    r = ec.call(lib, case.cfg, case.blob, x, src, np.zeros((1, E, case.cfg.embed_hidden), np.float32), expect_rc=1)
    assert "bytes of LDS per graph" in r["err"]


def test_structure(lib):
    ec.structure_checks(lib)


def test_linearity_in_dh0(lib):
    ec.linearity_check(lib)


def test_bad_inputs(lib):
    ec.bad_input_checks(lib)


def test_dembed_is_overwritten(lib):
    case = ec.shape_case(3, 1)
    src = case.sources()["reference"]
    n = ec.embed_floats(case.cfg)
    garbage = np.random.default_rng(1).integers(-2 ** 31, 2 ** 31 - 1, n).astype(np.int32)
    a = ec.call(lib, case.cfg, case.blob, case.x, src, case.dh0, fill=garbage)
    b = ec.call(lib, case.cfg, case.blob, case.x, src, case.dh0, fill=~garbage)
    np.testing.assert_array_equal(a["dembed"].view(np.int32), b["dembed"].view(np.int32))


def test_slabs_change_nothing_but_the_grouping(lib):
    ec.slab_check(lib)


# ---- refusals -----------------------------------------------------------------------------------------------------

def test_refusals(lib):
    case = ec.shape_case(3, 1)
    cfg, blob, x, dh0 = case.cfg, case.blob, case.x, case.dh0
    srcs = case.sources()
    src, cmp_ = srcs["reference"], srcs["compact"]
    run = lambda **kw: ec.call(lib, kw.pop("cfg", cfg), blob, x, kw.pop("src", src), dh0, expect_rc=1, **kw)["err"]
    # null pointers
    assert "weights is null" in run(over=dict(weights=None))
    assert "io is null" in run(over=dict(io=None))
    for f in ("dembed", "workspace", "node_obs", "adj", "dh0"):
        assert "is null" in run(io_over={f: None})
    # misalignment
    for f, by in (("node_obs", 2), ("adj", 2), ("dh0", 2), ("dembed", 2), ("workspace", 4), ("bad", 4)):
        assert "misaligned" in run(io_over={f: (lambda fields, f=f, by=by: fields[f].value + by)}), f
    assert "misaligned" in run(src=cmp_, io_over={"masks": lambda fields: fields["masks"].value + 4})
    # sizes outside the limits
    assert "E must be" in run(over=dict(E=0)) and "E must be" in run(over=dict(E=257))
    assert "B < 0" in run(over=dict(B=-1)) and "INT32_MAX" in run(over=dict(B=2 ** 31))
    assert "H must be" in run(cfg=dataclasses.replace(cfg, H=5))
    assert "embed_hidden" in run(cfg=dataclasses.replace(cfg, embed_hidden=65))
    # the compact layout
    assert "multiple of N" in run(src=cmp_, over=dict(N=2)) and "multiple of N" in run(src=cmp_, over=dict(N=0))
    # overlaps: an output on an input, two outputs on each other
    assert "overlaps an input" in run(io_over={"dembed": lambda f: f["dh0"].value})
    assert "overlaps an input" in run(io_over={"workspace": lambda f: f["adj"].value})
    assert "overlaps an input" in run(io_over={"bad": lambda f: f["node_obs"].value + 8})
    assert "outputs overlap" in run(io_over={"workspace": lambda f: f["dembed"].value + 8})
    assert "outputs overlap" in run(io_over={"bad": lambda f: f["workspace"].value})
    # the plan's own null
    assert lib.lsm_gnn_embed_backward_plan(cfg.struct(), 1, 3, 1, 0, None) == 1
    assert lib.lsm_gnn_embed_backward_last_error().decode().startswith("gnn embed backward: ")


def test_the_lds_refusal_through_the_call(lib):
    cfg = ec.limit_cfg()
    E = ec.largest_E(cfg) + 1
    _, blob = gm.default_weights(dataclasses.replace(cfg, aggr="node"), 0)
    x, table, bits = gm.random_graphs(1, E, cfg.F, seed=1)
    src = ga.sources(table, bits, 1, None)["reference"]
    err = ec.call(lib, cfg, blob, x, src, np.zeros((1, E, cfg.embed_hidden), np.float32), expect_rc=1)["err"]
    assert "bytes of LDS per graph" in err and "163840" in err


def test_B_zero_writes_nothing(lib):
    case = ec.shape_case(3, 1)
    import mb_edges_abi as mb
    src = mb.Source(np.zeros((0, 3, 3), np.float32))
    r = ec.call(lib, case.cfg, case.blob, np.zeros((0, 3, case.cfg.F), np.float32), src,
                np.zeros((0, 3, case.cfg.embed_hidden), np.float32))
    assert r["bad"] == 0


def test_largest_ratio_is_reported(lib):
    """Runs last in this file: prints the largest err / e32 seen (DESIGN.md records it)."""
    seen = [(r, w) for w, r in gm.RATIOS if w.startswith("host ") and np.isfinite(r)]
    if seen:
        print("gnn embed backward, host: largest err/e32 %.2f (%s)" % max(seen))
