"""The cases of the spilled tier's tests and the ctypes call (include/lsm_gnn_backward_large.h), shared by
tests/test_gnn_backward_large_capi.py (the plan and the host entry point) and tests/test_gpu_gnn_backward_large.py
(the kernels). The cases, the seeds, the float64 model and the tolerance are tests/gnn_backward_cases.py's, by
import. Every output and the whole workspace, scratch included, sit between canaries."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import gnn_backward_cases as bc
import recurrent_abi as ra
from lsm import capi

DEFAULT = bc.DEFAULT
LDS = 163840
# small graphs beyond lsm_gnn_backward's limit: the generic instance, wide heads
WIDE_A = dataclasses.replace(DEFAULT, H=4, C=64, concat=False, layer_N=0)    # old limit E = 30
WIDE_B = dataclasses.replace(WIDE_A, concat=True)                             # old limit E = 19, the forward's 39
CONFIGS = {"default": DEFAULT, "wideA": WIDE_A, "wideB": WIDE_B}
BEYOND = {"default": (114, 192, 256), "wideA": (31, 48), "wideB": (20, 33, 39)}
PREFIX = "gnn backward large: "


def pad(w):
    return ((w + 3) & ~3) + 4


def strides(cfg):
    """(SA, SK, ST) of lsm_gnn_backward.h."""
    HC, D = cfg.H * cfg.C, cfg.out_dim
    return (pad(max(cfg.embed_hidden, D)), pad(max(cfg.embed_hidden, HC)),
            (2 * cfg.H * (cfg.layer_N + 1) + 5 * cfg.H) | 1)


def kept(cfg, E, s):
    """The header's formula: a graph's LDS floats at level s."""
    SA, SK, ST = strides(cfg)
    per_node = 2 * SA + 2 * SK + (s < 1) * (cfg.layer_N + 2) * SA + (s < 2) * SK + (s < 3) * ST + (s < 4) * SK
    return E * per_node + ((E + 3) & ~3)


def spilled_floats(cfg, E, s):
    SA, SK, ST = strides(cfg)
    n = E * ((s >= 1) * (cfg.layer_N + 2) * SA + (s >= 2) * SK + (s >= 3) * ST + (s >= 4) * SK)
    return (n + 3) & ~3


def lowest_level(cfg, E, min_spill=0):
    """The lowest level >= min_spill whose LDS need fits, or None when even the forward's region does not."""
    for s in range(min_spill, 5):
        if 4 * kept(cfg, E, s) <= LDS:
            return s
    return None


def plan(cfg, B, E, N=1, masked=False, min_spill=0):
    """(plan dict, None) or (None, the refusal's text) from lsm_gnn_backward_large_plan."""
    lib, p = bc._lib(), capi.LsmGnnBwdLargeLaunchPlan()
    if lib.lsm_gnn_backward_large_plan(cfg.struct(), B, E, N, int(masked), min_spill, C.byref(p)):
        return None, lib.lsm_gnn_backward_large_last_error().decode()
    return {n: int(getattr(p, n)) for n, _ in p._fields_}, None


def ws_bytes(cfg, B, E, min_spill=0):
    return int(bc._lib().lsm_gnn_backward_large_workspace_bytes(cfg.struct(), B, E, min_spill))


@functools.lru_cache(maxsize=None)
def first_E_of_each_level(name):
    """{level: the smallest E at which the plan of CONFIGS[name] reports it}, over the sizes the forward accepts."""
    out = {}
    for E in range(1, 257):
        p = plan(CONFIGS[name], 2, E)[0]
        if p is None:
            break
        out.setdefault(p["spill"], E)
    return out


@functools.lru_cache(maxsize=None)
def case(name, E, B=2, aggr="global_mean"):
    """B graphs of E nodes on CONFIGS[name], at the density that keeps E = 24's mean in-degree, from _random's
    default seed base, as gnn_backward_cases.shape_case's."""
    cfg = dataclasses.replace(CONFIGS[name], aggr=aggr)
    return bc.Case("large %s E%d B%d" % (name, E, B), cfg, bc._random(cfg, B, E, 1), B, E)


def call(lib, cfg, blob, node_obs, src, agent_id, dout, min_spill=0, want_dh0=True, expect_rc=0, over=None,
         io_over=None, stream=None, ws_off=0, ws_min_spill=None):
    """lsm_host_gnn_backward_large (src.device is None) or lsm_gnn_backward_large on src.device, as
    gnn_backward_cases.call runs the old entry points. The workspace holds exactly
    lsm_gnn_backward_large_workspace_bytes(cfg, B, E, min_spill) bytes between canaries, ws_off words (an even
    number) past a 16-byte boundary. A refused call must have written nothing, the workspace included."""
    dev = src.device
    node_obs = np.ascontiguousarray(node_obs, dtype=np.float32)
    B, E = node_obs.shape[0], src.E
    nW = int(np.asarray(blob).size)
    w = ra.Placed(np.ascontiguousarray(blob, dtype=np.float32).view(np.int32), 0, dev)
    x = ra.Placed(node_obs.view(np.int32), 0, dev) if node_obs.size else None
    aid = None
    if agent_id is not None:
        aid = ra.Placed(np.ascontiguousarray(agent_id, dtype=np.int64).reshape(-1).view(np.int32), 0, dev)
    do = ra.Placed(np.ascontiguousarray(dout, dtype=np.float32).view(np.int32), 0, dev)
    dw = ra.destination(nW, 0, dev)
    dh = ra.destination(max(B * E * cfg.embed_hidden, 1), 0, dev)
    size_level = min_spill if ws_min_spill is None else ws_min_spill
    nbytes = ws_bytes(cfg, B, E, size_level) if 0 <= size_level <= 4 else 0
    nws = max(nbytes // 4, 2)
    ws = ra.destination(nws, ws_off, dev)
    bad = ra.Placed(np.zeros(1, np.int64).view(np.int32), 0, dev)
    ptr = lambda p: C.c_void_p(p.ptr) if p is not None else None
    fields = dict(node_obs=ptr(x), adj=ptr(src.adj), masks=ptr(src.masks), agent_id=ptr(aid), dout=ptr(do),
                  dweights=C.c_void_p(dw[0].ptr + 4 * ra.PRE),
                  dh0=C.c_void_p(dh[0].ptr + 4 * ra.PRE) if want_dh0 else None,
                  workspace=C.c_void_p(ws[0].ptr + 4 * ra.PRE), bad=ptr(bad))
    for k, v in (io_over or {}).items():
        fields[k] = None if v is None else C.c_void_p(v(fields) if callable(v) else v)
    io = capi.LsmGnnBwdIo(**fields)
    args = dict(weights=ptr(w), io=C.byref(io), B=B, E=E, N=src.N)
    args.update(over or {})
    a = (cfg.struct(), args["weights"], args["io"], args["B"], args["E"], args["N"])
    if dev is None:
        rc = lib.lsm_host_gnn_backward_large(*a)
    else:
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        rc = lib.lsm_gnn_backward_large(*a, min_spill, C.c_void_p(s.cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_gnn_backward_large_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    dww = ra.read_destination(dw, "dweights")
    dhw = ra.read_destination(dh, "dh0")
    wsw = ra.read_destination(ws, "workspace")
    badv = int(bad.read().view(np.int64)[0])
    if expect_rc:
        assert err.startswith(PREFIX) and len(err) > len(PREFIX), err
        assert (dww == ra.CANARY).all() and (dhw == ra.CANARY).all() and (wsw == ra.CANARY).all(), "a refused call wrote"
        assert badv == 0
        return dict(err=err)
    return dict(dweights=dww.view(np.float32).copy(), bad=badv, ws_bytes=nbytes,
                dh0=dhw[:B * E * cfg.embed_hidden].view(np.float32).reshape(B, E, cfg.embed_hidden).copy() if want_dh0 else None)


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(a["dweights"].view(np.int32), b["dweights"].view(np.int32), what)
    np.testing.assert_array_equal(a["dh0"].view(np.int32), b["dh0"].view(np.int32), what)


def check(lib, case_, device=None, min_spill=0, layouts=bc.LAYOUTS):
    """gnn_backward_cases.check for the large entry points: every conv entry's gradient and dh0 against the
    float64 model within the case's own tolerance in each layout, the EmbedConv range exactly 0, the layouts
    bit-equal. Returns {layout: result}."""
    outs = {}
    srcs = case_.sources(device)
    aid = case_.agent_id if case_.cfg.aggr == "node" else None
    for layout in layouts:
        r = call(lib, case_.cfg, case_.blob, case_.x, srcs[layout], aid, case_.dout, min_spill=min_spill)
        assert r["bad"] == 0
        what = "%s %s %s" % ("host" if device is None else "device", case_.name, layout)
        got = bc.split(case_.cfg, r["dweights"])
        assert not r["dweights"][:bc.conv0(case_.cfg)].view(np.int32).any(), "the EmbedConv range is not exactly 0"
        for name in case_.truth.names():
            bc.assert_close(r["dh0"] if name == "dh0" else got[name], case_.truth, name, what)
        outs[layout] = r
    if len(layouts) == 2:
        same_bits(outs[layouts[0]], outs[layouts[1]], "the layouts differ")
    return outs
