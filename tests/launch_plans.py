"""Helpers around the two plan entry points, lsm_gnn_plan (include/lsm_gnn.h) and lsm_head_plan
(include/lsm_policy.h): the launch plan the library itself computes for a config and sizes, as a dict, and
walks that find an acceptance boundary by asking the library (nothing here restates the plan's arithmetic).
Shared by the cases modules, which size their limit cases from it, and by tests/test_launch_plans.py."""
import ctypes as C
import dataclasses
import functools

from lsm import capi

LDS = 163840                      # a workgroup's LDS in bytes (the headers' figure)
FORWARD, EVALUATE, BACKWARD = capi.LSM_HEAD_PLAN_FORWARD, capi.LSM_HEAD_PLAN_EVALUATE, capi.LSM_HEAD_PLAN_BACKWARD
WHICH = {"forward": FORWARD, "evaluate": EVALUATE, "backward": BACKWARD}


@functools.lru_cache(maxsize=None)
def _lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@functools.lru_cache(maxsize=None)
def gnn_plan(cfg, B, E, N=1, masked=False):
    """(plan dict, None) or (None, the refusal's text) for lsm_gnn_forward at these sizes."""
    lib, p = _lib(), capi.LsmGnnLaunchPlan()
    if lib.lsm_gnn_plan(cfg.struct(), B, E, N, int(masked), C.byref(p)):
        return None, lib.lsm_gnn_last_error().decode()
    return {n: int(getattr(p, n)) for n, _ in p._fields_}, None


@functools.lru_cache(maxsize=None)
def head_plan(cfg, which, Cn=65, T=3):
    """(plan dict, None) or (None, the refusal's text); which: 'forward', 'evaluate' or 'backward'."""
    lib, p = _lib(), capi.LsmHeadLaunchPlan()
    if lib.lsm_head_plan(cfg.struct(), WHICH[which], Cn, T, C.byref(p)):
        return None, lib.lsm_policy_last_error().decode()
    d = {n: int(getattr(p, n)) for n in ("SX", "SA", "SH", "S0", "S1", "S2", "HP", "njobs", "ntiles", "slabs",
                                         "ws_floats", "o_feat")}
    d["lds_bytes"] = [int(v) for v in p.lds_bytes]
    d["o_ho"] = [int(v) for v in p.o_ho]
    d["jobs"] = [dict(nout=j.nout, nin=j.nin, ti_n=j.ti_n, tile0=j.tile0) for j in p.job[:p.njobs]]
    return d, None


def last_accepted(accepts, start, stop):
    """The largest v in [start, stop] with accepts(v), walking up from an accepted start; accepts(v + 1) is
    False or v == stop."""
    assert accepts(start), start
    v = start
    while v < stop and accepts(v + 1):
        v += 1
    return v


def with_in(cfg, width):
    """cfg with in0 + in1 == width: in1 keeps its value while it fits (the encoder's block), in0 takes the rest."""
    in1 = min(cfg.in1, width)
    return dataclasses.replace(cfg, in0=width - in1, in1=in1)


def largest_in(cfg, which):
    """The largest accepted in0 + in1 of cfg's other sizes (the ABI's own limit is 256)."""
    return last_accepted(lambda w: head_plan(with_in(cfg, w), which)[0] is not None, 1, 257)


def largest_hidden(cfg, which):
    return last_accepted(lambda h: head_plan(dataclasses.replace(cfg, hidden=h), which)[0] is not None, 1, 129)


def largest_E(cfg):
    return last_accepted(lambda E: gnn_plan(cfg, 1, E)[0] is not None, 1, 257)


def adj_switch(cfg):
    """(E, E + 1): the last E whose adjacency is staged in LDS and the first whose is not (None without one)."""
    last = largest_E(cfg)
    for E in range(1, last):
        if gnn_plan(cfg, 1, E)[0]["adj_lds"] and not gnn_plan(cfg, 1, E + 1)[0]["adj_lds"]:
            return E, E + 1
    return None
