"""CPU tests of the spilled tier of the graph encoder's backward pass (include/lsm_gnn_backward_large.h): the
header and its exports; the launch plan at every size lsm_gnn_forward accepts, its level recomputed here from the
header's formula; lsm_host_gnn_backward_large bit-equal to lsm_host_gnn_backward where both accept and within
the case's own tolerance of the float64 model (tests/gnn_backward_model.py) at sizes the old entry points
refuse; and the refusals, which leave the outputs and the whole workspace untouched."""
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
import gnn_backward_large_cases as lc
import gnn_cases as gc
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_gnn_backward_large.h")
PLAN_CONFIGS = dict(lc.CONFIGS, **{"option " + k: dataclasses.replace(bc.DEFAULT, **kw) for k, kw in gc.OPTIONS.items()})
SHARED = ("TS", "G", "fast", "adj_lds", "acc_lds", "SA", "SK", "ST", "lds_bytes", "slabs")


@pytest.fixture(scope="module")
def lib():
    return bc._lib()


def forward_accepts(lib, cfg, B, E):
    p = capi.LsmGnnLaunchPlan()
    return lib.lsm_gnn_plan(cfg.struct(), B, E, 1, 0, C.byref(p)) == 0


# ---- the ABI ----------------------------------------------------------------------------------------------------

def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_GNN_BACKWARD_LARGE) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert not declared & set(capi.EXPORTED_GNN_BACKWARD) and not declared & set(capi.EXPORTED_GNN_EMBED_BACKWARD)
    body = hdr[hdr.index("typedef struct lsm_gnn_bwd_large_launch_plan"):hdr.index("} lsm_gnn_bwd_large_launch_plan")]
    decls = re.findall(r"(int(?:32|64)_t)\s+([^;]+);", body)
    fields = [(n, {"int32_t": C.c_int32, "int64_t": C.c_int64}[t]) for t, decl in decls for n in re.split(r",\s*", decl)]
    assert fields == list(capi.LsmGnnBwdLargeLaunchPlan._fields_)
    old = [f for f, _ in capi.LsmGnnBwdLaunchPlan._fields_]
    new = [f for f, _ in capi.LsmGnnBwdLargeLaunchPlan._fields_]
    assert set(new) - set(old) == {"spill", "spilled_floats", "scratch_bytes"} and set(old) <= set(new)
    assert lib.lsm_gnn_backward_large_last_error.restype is C.c_char_p


# ---- the plan ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(PLAN_CONFIGS))
def test_plan_at_every_size_the_forward_accepts(lib, name):
    cfg = PLAN_CONFIGS[name]
    B = bc.SLAB + 1
    nconv = int(lib.lsm_gnn_weights_floats(cfg.struct())) - bc.conv0(cfg)
    accepted = refused = 0
    for E in range(1, 257):
        p, why = lc.plan(cfg, B, E)
        if not forward_accepts(lib, cfg, B, E):
            assert p is None and why.startswith(lc.PREFIX) and "lsm_gnn_forward refuses" in why, (E, why)
            assert str(4 * lc.kept(cfg, E, 4)) in why and "163840" in why, why    # the forward's figures
            assert lc.ws_bytes(cfg, B, E) == 0
            refused += 1
            continue
        accepted += 1
        assert p is not None, (E, why)
        assert p["lds_bytes"] <= lc.LDS and p["G"] >= 1, (E, p)
        level = lc.lowest_level(cfg, E)
        assert level is not None and p["spill"] == level, (E, p, level)
        assert p["spilled_floats"] == lc.spilled_floats(cfg, E, level)
        assert p["TS"] == max(32, 1 << (E - 1).bit_length()) and p["slabs"] == 2
        assert p["G"] == min(256 // p["TS"], lc.LDS // (p["lds_bytes"] // p["G"]))
        # the adjacency and its transpose: both or neither, when they fit beside what the level keeps
        assert p["adj_lds"] == int(4 * (lc.kept(cfg, E, level) + 2 * ((E * E + 3) & ~3)) <= lc.LDS)
        assert p["scratch_bytes"] == (4 * p["slabs"] * p["G"] * p["spilled_floats"] + 8 if level else 0)
        assert p["ws_bytes"] == 8 * p["slabs"] * nconv + p["scratch_bytes"] == lc.ws_bytes(cfg, B, E)
        old, _ = bc.plan(cfg, B, E)
        assert (old is not None) == (level == 0), (E, level)
        if old is not None:
            assert all(p[k] == old[k] for k in SHARED), (E, p, old)
            assert p["ws_bytes"] == old["ws_bytes"] and p["scratch_bytes"] == 0 and p["spilled_floats"] == 0
        for k in range(5):
            q, why = lc.plan(cfg, B, E, min_spill=k)
            assert q is not None and q["spill"] == max(k, level) == lc.lowest_level(cfg, E, k), (E, k, q, why)
            assert q["lds_bytes"] <= lc.LDS and q["ws_bytes"] == lc.ws_bytes(cfg, B, E, k)
    assert accepted >= 39 and (refused > 0 or not name.startswith("wide"))


def test_limits_and_levels(lib):
    """The old limits and the forward's, as the three configs were chosen for; every level is reached by wideB."""
    assert bc.largest_E(lc.DEFAULT) == 113 and bc.largest_E(lc.WIDE_A) == 30 and bc.largest_E(lc.WIDE_B) == 19
    for name, last in (("default", 256), ("wideB", 39)):
        assert lc.plan(lc.CONFIGS[name], 1, last)[0] is not None
        assert last == 256 or lc.plan(lc.CONFIGS[name], 1, last + 1)[0] is None
    assert lc.plan(lc.WIDE_A, 1, 48)[0] is not None and lc.plan(lc.WIDE_A, 1, 65)[0] is None
    levels = lc.first_E_of_each_level("wideB")
    assert sorted(levels) == [0, 1, 2, 3, 4] and levels[0] == 1 and levels[1] == 20, levels
    assert sorted(lc.first_E_of_each_level("default")) == [0, 1, 2, 3, 4]
    assert lc.plan(lc.DEFAULT, 1, 192)[0]["spill"] >= 1
    assert lc.plan(lc.DEFAULT, 5, 24, N=2, masked=True)[0] is None and lc.plan(lc.DEFAULT, 4, 24, N=2, masked=True)[0]


def test_min_spill_outside_the_levels_is_refused(lib):
    for k in (-1, 5, 2 ** 31 - 1, -2 ** 31):
        p, why = lc.plan(lc.DEFAULT, 1, 24, min_spill=k)
        assert p is None and why == lc.PREFIX + "min_spill must be in [0, 4]", (k, why)
        assert lc.ws_bytes(lc.DEFAULT, 1, 24, k) == 0
    assert lib.lsm_gnn_backward_large_plan(lc.DEFAULT.struct(), 1, 3, 1, 0, 0, None) == 1
    assert lib.lsm_gnn_backward_large_last_error().decode().startswith(lc.PREFIX)
    # the two headers' texts are apart: a refusal here leaves the old header's last error alone
    bc.plan(lc.DEFAULT, 1, 300)
    old = lib.lsm_gnn_backward_last_error().decode()
    lc.plan(lc.DEFAULT, 1, 24, min_spill=7)
    assert lib.lsm_gnn_backward_last_error().decode() == old and old.startswith("gnn backward: E must be")


# ---- the host entry point ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("make,args", [(bc.shape_case, (24, 1)), (bc.structure_case, ()), (bc.slab_case, (bc.SLAB + 1,))],
                         ids=["shape", "structure", "slab"])
def test_host_equals_the_old_host_entry_point(lib, make, args):
    case = make(*args)
    aid = case.agent_id if case.cfg.aggr == "node" else None
    for layout, src in case.sources().items():
        old = bc.call(lib, case.cfg, case.blob, case.x, src, aid, case.dout)
        new = lc.call(lib, case.cfg, case.blob, case.x, src, aid, case.dout)
        lc.same_bits(old, new, "%s %s" % (case.name, layout))
        assert new["ws_bytes"] == bc.ws_bytes(case.cfg, case.B, case.E)


@pytest.mark.parametrize("name,E", [(n, E) for n in sorted(lc.BEYOND) for E in lc.BEYOND[n]])
def test_host_matches_model_beyond_the_old_limit(lib, name, E):
    """Within truth.want of the float64 model in both layouts, the layouts bit-equal, the EmbedConv range 0; the
    old entry point refuses the size."""
    case = lc.case(name, E)
    assert case.truth.why_not is None and case.seed < bc.SEEDS
    assert bc.plan(case.cfg, case.B, E)[0] is None
    lc.check(lib, case)


def test_refusals_write_nothing(lib):
    """call() checks the canaries around dweights, dh0 and the whole workspace (sized for level 4: the scratch is
    inside) after every refused call; the device entry point refuses before it touches the device."""
    case = bc.shape_case(3, 1)
    cfg, blob, x, ids, dout = case.cfg, case.blob, case.x, case.agent_id, case.dout
    srcs = case.sources()
    src, cmp_ = srcs["reference"], srcs["compact"]

    def run(**kw):
        return lc.call(lib, kw.pop("cfg", cfg), blob, x, kw.pop("src", src), kw.pop("ids", ids), dout, expect_rc=1,
                       ws_min_spill=4, **kw)["err"]
    assert "weights is null" in run(over=dict(weights=None)) and "io is null" in run(over=dict(io=None))
    for f in ("dweights", "workspace", "node_obs", "adj", "dout"):
        assert "is null" in run(io_over={f: None})
    assert "agent_id" in run(ids=None)
    for f, by in (("node_obs", 2), ("adj", 2), ("dout", 2), ("dweights", 2), ("dh0", 2), ("workspace", 4),
                  ("agent_id", 4), ("bad", 4)):
        assert "misaligned" in run(io_over={f: (lambda fields, f=f, by=by: fields[f].value + by)}), f
    assert "E must be" in run(over=dict(E=0)) and "E must be" in run(over=dict(E=257))
    assert "B < 0" in run(over=dict(B=-1)) and "INT32_MAX" in run(over=dict(B=2 ** 31))
    assert "H must be" in run(cfg=dataclasses.replace(cfg, H=5))
    assert "multiple of N" in run(src=cmp_, over=dict(N=2)) and "multiple of N" in run(src=cmp_, over=dict(N=0))
    assert "overlaps an input" in run(io_over={"workspace": lambda f: f["adj"].value})
    assert "outputs overlap" in run(io_over={"workspace": lambda f: f["dweights"].value + 8})
    assert "outputs overlap" in run(io_over={"bad": lambda f: f["workspace"].value})
    # a size the forward refuses, through the host entry point
    wide = lc.case("wideB", 39)
    big = lc.WIDE_B
    assert "lsm_gnn_forward refuses" in lc.call(lib, big, wide.blob, wide.x, wide.sources()["reference"], None,
                                                 wide.dout, expect_rc=1, over=dict(E=40))["err"]
    # the device entry point's own refusals need no device: they return before any launch
    io = capi.LsmGnnBwdIo()
    for k in (-1, 5):
        assert lib.lsm_gnn_backward_large(cfg.struct(), None, C.byref(io), 1, 3, 1, k, None) == 1
        assert lib.lsm_gnn_backward_large_last_error().decode() == lc.PREFIX + "min_spill must be in [0, 4]"
    assert lib.lsm_gnn_backward_large(cfg.struct(), None, C.byref(io), 1, 3, 1, 0, None) == 1
    assert "weights is null" in lib.lsm_gnn_backward_large_last_error().decode()


def test_the_scratch_is_inside_the_overlap_checks(lib):
    """An input that lies in the scratch's bytes, beyond the slab accumulators, is an overlap at a level that has
    a scratch (checked through the device entry point's argument checks, which launch nothing when they refuse)."""
    case = bc.shape_case(3, 1)
    cfg = case.cfg
    acc = bc.ws_bytes(cfg, case.B, 3)
    total = lc.ws_bytes(cfg, case.B, 3, 4)
    assert total > acc + 8
    ws = np.zeros(total // 8 + 2, np.float64)
    others = np.zeros(4096, np.float32)
    inside = ws.ctypes.data + acc + 16        # in the scratch
    io = capi.LsmGnnBwdIo(node_obs=C.c_void_p(inside), adj=C.c_void_p(others.ctypes.data),
                          dout=C.c_void_p(others.ctypes.data + 4096), dweights=C.c_void_p(others.ctypes.data + 8192),
                          agent_id=C.c_void_p(others.ctypes.data + 2048), workspace=C.c_void_p(ws.ctypes.data))
    w = np.ascontiguousarray(case.blob, np.float32)
    dw = np.zeros(w.size, np.float32)
    io.dweights = C.c_void_p(dw.ctypes.data)
    rc = lib.lsm_gnn_backward_large(cfg.struct(), C.c_void_p(w.ctypes.data), C.byref(io), case.B, 3, 1, 4, None)
    assert rc == 1 and "overlaps an input" in lib.lsm_gnn_backward_large_last_error().decode()
    assert not ws.any() and not dw.any()
