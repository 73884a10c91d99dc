"""The cases of the graph encoder's backward tests and the ctypes call (include/lsm_gnn_backward.h), shared by
tests/test_gnn_backward_capi.py (the host entry point) and tests/test_gpu_gnn_backward.py (the kernel). Every
output and the workspace sit between canaries. A case's inputs (weights, graphs, dout) come from one seed, the
first of at most 50 that tests/gnn_backward_model.py's two models admit; no admissible seed is an error."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import gnn_abi as ga
import gnn_backward_model as gbm
import gnn_cases as gc
import gnn_model as gm
import recurrent_abi as ra
from lsm import capi, gnn

DEFAULT = gc.DEFAULT
SLAB = capi.LSM_GNN_BWD_SLAB
SHAPE_E = (1, 3, 24, 33, 65)       # below a wave, TS = 64 and TS = 128
LAYOUTS = ga.LAYOUTS
SEEDS = 50
SMALL = dataclasses.replace(DEFAULT, C=4, embed_hidden=4, H=2)      # the slab cases' config
OPTION_NAMES = ("H1", "concat", "H1 concat", "gnn_layer_N 0", "tanh", "C12 hidden20", "C12 hidden20 tanh mean")
TANH = dataclasses.replace(DEFAULT, embed_relu=False, relu=False)


@functools.lru_cache(maxsize=None)
def _lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


def plan(cfg, B, E, N=1, masked=False):
    """(plan dict, None) or (None, the refusal's text) from lsm_gnn_backward_plan."""
    lib, p = _lib(), capi.LsmGnnBwdLaunchPlan()
    if lib.lsm_gnn_backward_plan(cfg.struct(), B, E, N, int(masked), C.byref(p)):
        return None, lib.lsm_gnn_backward_last_error().decode()
    return {n: int(getattr(p, n)) for n, _ in p._fields_}, None


def plan_key(p):
    return (p["TS"], p["G"], p["fast"], p["acc_lds"], p["adj_lds"])


def largest_E(cfg):
    E = 1
    while E < 256 and plan(cfg, 1, E + 1)[0] is not None:
        E += 1
    return E


def ws_bytes(cfg, B, E):
    return int(_lib().lsm_gnn_backward_workspace_bytes(cfg.struct(), B, E))


def conv0(cfg):
    """The blob offset of conv layer 0's first entry, from the entries' shapes."""
    o = 0
    for name, shape in gnn.weight_entries(cfg):
        if name.startswith("gnn1."):
            return o
        o += int(np.prod(shape))
    raise AssertionError


def split(cfg, dweights):
    """{name without prefix: array} views of a dweights blob, every entry."""
    out, o = {}, 0
    for name, shape in gnn.weight_entries(cfg):
        n = int(np.prod(shape))
        out[name] = dweights[o:o + n].reshape(shape)
        o += n
    assert o == dweights.size
    return out


def _ptr(p):
    return C.c_void_p(p.ptr) if p is not None else None


def call(lib, cfg, blob, node_obs, src, agent_id, dout, want_dh0=True, bad_init=0, expect_rc=0, over=None,
         io_over=None, fill=None, stream=None):
    """lsm_host_gnn_backward (src.device is None) or lsm_gnn_backward on src.device. Returns a dict: dweights
    [floats], dh0 [B, E, Hd] or None, bad, and the raw words. over: replace B / E / N / weights; io_over: replace
    io fields (a name set to None: a null pointer; to an int: that address). fill: the words dweights holds
    before the call (the canary by default). A refused call must have written nothing."""
    dev = src.device
    node_obs = np.ascontiguousarray(node_obs, dtype=np.float32)
    B, E = node_obs.shape[0], src.E
    nW = int(np.asarray(blob).size)
    w = ra.Placed(np.ascontiguousarray(blob, dtype=np.float32).view(np.int32), 0, dev)
    x = ra.Placed(node_obs.view(np.int32), 0, dev) if node_obs.size else None
    aid = None
    if agent_id is not None:
        aid = ra.Placed(np.ascontiguousarray(agent_id, dtype=np.int64).reshape(-1).view(np.int32), 0, dev)
    do = ra.Placed(np.ascontiguousarray(dout, dtype=np.float32).view(np.int32), 0, dev) if np.asarray(dout).size else None
    dw = ra.destination(nW, 0, dev)
    if fill is not None:
        host = np.full(ra.PRE + nW + ra.TAIL, ra.CANARY, np.int32)
        host[ra.PRE:ra.PRE + nW] = fill
        dw = (ra.Placed(host, 0, dev), nW)
    nh = max(B * E * cfg.embed_hidden, 1)
    dh = ra.destination(nh, 0, dev)
    nws = max(ws_bytes(cfg, B, E) // 4, 2)
    ws = ra.destination(nws, 0, dev)
    bad = ra.Placed(np.array([bad_init], np.int64).view(np.int32), 0, dev)
    fields = dict(node_obs=_ptr(x), adj=_ptr(src.adj), masks=_ptr(src.masks), agent_id=_ptr(aid), dout=_ptr(do),
                  dweights=C.c_void_p(dw[0].ptr + 4 * ra.PRE),
                  dh0=C.c_void_p(dh[0].ptr + 4 * ra.PRE) if want_dh0 else None,
                  workspace=C.c_void_p(ws[0].ptr + 4 * ra.PRE), bad=_ptr(bad))
    for k, v in (io_over or {}).items():
        fields[k] = None if v is None else C.c_void_p(v(fields) if callable(v) else v)
    io = capi.LsmGnnBwdIo(**fields)
    args = dict(weights=_ptr(w), io=C.byref(io), B=B, E=E, N=src.N)
    args.update(over or {})
    a = (cfg.struct(), args["weights"], args["io"], args["B"], args["E"], args["N"])
    if dev is None:
        rc = lib.lsm_host_gnn_backward(*a)
    else:
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        rc = lib.lsm_gnn_backward(*a, C.c_void_p(s.cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_gnn_backward_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    dww = ra.read_destination(dw, "dweights")
    dhw = ra.read_destination(dh, "dh0")
    ra.read_destination(ws, "workspace")
    badv = int(bad.read().view(np.int64)[0])
    if expect_rc:
        assert err.startswith("gnn backward: ") and len(err) > len("gnn backward: "), err
        assert (dww == (ra.CANARY if fill is None else fill)).all() and (dhw == ra.CANARY).all(), "a refused call wrote"
        assert badv == bad_init
        return dict(err=err)
    if not want_dh0 or B == 0:
        assert (dhw == ra.CANARY).all()
    if B == 0:
        assert (dww == (ra.CANARY if fill is None else fill)).all()
        return dict(bad=badv)
    return dict(dweights=dww.view(np.float32).copy(), bad=badv,
                dh0=dhw[:B * E * cfg.embed_hidden].view(np.float32).reshape(B, E, cfg.embed_hidden).copy() if want_dh0 else None)


class Case:
    """cfg (with its readout), inputs made by make(seed) -> (x, compact triple or None, dense or None), the ego
    ids, and the first admissible seed's weights, dout and truth."""

    def __init__(self, name, cfg, make, B, E):
        self.name, self.cfg, self._make, self.B, self.E = name, cfg, make, B, E
        self._placed = {}

    @functools.cached_property
    def _found(self):
        why = []
        for seed in range(SEEDS):
            x, compact, dense = self._make(seed)
            srcs = ga.sources(*compact, None) if compact is not None else ga.dense_sources(dense, None)
            full = srcs["reference"].full
            sd, blob = gm.default_weights(dataclasses.replace(self.cfg, aggr="node"), seed)
            dout = np.random.default_rng(4000 + seed).normal(0, 1, (self.B, self.cfg.out_dim)).astype(np.float32)
            truth = gbm.Truth(self.cfg, sd, x, full, dout, self.agent_id)
            if truth.why_not is None:
                return dict(seed=seed, x=x, compact=compact, dense=dense, full=full, sd=sd, blob=blob, dout=dout,
                            truth=truth)
            why.append(truth.why_not)
        raise AssertionError("%s: no admissible seed among %d (%s)" % (self.name, SEEDS, sorted(set(why))))

    @property
    def agent_id(self):
        return gc.ego_ids(self.B, self.E)

    def __getattr__(self, k):
        if k in ("seed", "x", "full", "sd", "blob", "dout", "truth"):
            return self._found[k]
        raise AttributeError(k)

    def sources(self, device=None):
        if device not in self._placed:
            f = self._found
            self._placed[device] = (ga.sources(*f["compact"], device) if f["compact"] is not None
                                    else ga.dense_sources(f["dense"], device))
        return self._placed[device]


def degree_density(E):
    """The density that keeps the mean in-degree at E = 24's 9.6 for larger graphs. EmbedConv sums over the
    incoming edges, so at a fixed density h0 and with it the logits grow with E, the softmax saturates and
    dalpha - s cancels almost completely: there the float32 model's error is itself unstable (on the same
    graphs with relabelled nodes, at E = 65 and density 0.4, the float32 model misses 4 * e32 of its own first
    labelling by up to 15 times), and e32 no longer measures anything."""
    return min(0.4, 9.6 / E)


def _random(cfg, B, E, N, base=0, density=None):
    density = degree_density(E) if density is None else density

    def make(seed):
        x, table, bits = gm.random_graphs(B, E, cfg.F, seed=base + seed, density=density, N=N)
        return x, (table, bits, N), None
    return make


def _connected(cfg, B, E, base=0, density=0.4):    # (its one user has E = 6)
    """Graphs without disconnect bits (dense statement): nodes without an incoming edge share their features
    through every layer, and two of them tie wherever they are a column's maximum."""
    def make(seed):
        x, table, _ = gm.random_graphs(B, E, cfg.F, seed=base + seed, density=density, N=1)
        return x, None, np.where(np.isfinite(table) & (table != 7.5), table, 0).astype(np.float32)
    return make


def group_B(cfg, E):
    """G + 1: one graph more than a workgroup takes at a time."""
    return plan(cfg, 1, E)[0]["G"] + 1


@functools.lru_cache(maxsize=None)
def shape_case(E, which):
    """which: 0 -> B = 1, 1 -> B = 5, 2 -> B = G + 1."""
    B = (1, 5, group_B(DEFAULT, E))[which]
    N = B if B <= 5 else 1
    return Case("shape E%d B%d" % (E, B), DEFAULT, _random(DEFAULT, B, E, N), B, E)


@functools.lru_cache(maxsize=None)
def option_case(name, aggr="node"):
    cfg = dataclasses.replace(DEFAULT, aggr=aggr, **gc.OPTIONS[name])
    return Case("option %s %s" % (name, aggr), cfg, _random(cfg, 5, 24, 5, base=100 + 50 * OPTION_NAMES.index(name)), 5, 24)


@functools.lru_cache(maxsize=None)
def readout_case(aggr):
    """All four readouts; global_max on a tanh config (under ReLU a tie at 0 carries gradient 0 whichever wins)."""
    cfg = dataclasses.replace(TANH if aggr == "global_max" else DEFAULT, aggr=aggr)
    if aggr == "global_max":    # few nodes: tanh saturates, and two nodes near 1 in one column are a tie
        return Case("readout " + aggr, cfg, _connected(cfg, 3, 6, base=700, density=0.6), 3, 6)
    return Case("readout " + aggr, cfg, _random(cfg, 5, 24, 5, base=700), 5, 24)


STRUCT_E = 12


def _structure(seed):
    """Graph 0: no edge. 1: target 5 has no incoming edge, target 7 exactly one (from 2), node 9 is a source
    but never a target. 2: a full graph. 3: asymmetric, r -> c only for r < c. 4: graph 3 transposed. 5: -0.0
    entries (not edges) among ordinary ones. 6: an ordinary graph."""
    E = STRUCT_E
    rng = np.random.default_rng(900 + seed)
    x, table, _ = gm.random_graphs(7, E, DEFAULT.F, seed=900 + seed)
    d = np.where(np.isfinite(table) & (table != 7.5), table, 0).astype(np.float32)
    d[0] = 0
    d[1, :, 5] = 0
    d[1, :, 7] = 0
    d[1, 2, 7] = 0.8
    d[1, :, 9] = 0
    d[1, 9, :4] = rng.uniform(0.1, 2.0, 4)
    d[1, 9, 7] = 0
    d[2] = rng.uniform(0.1, 2.0, (E, E))
    d[3] = np.triu(rng.uniform(0.1, 2.0, (E, E)), 1)
    d[4] = d[3].T
    x[4] = x[3]
    d[5][(d[5] == 0) & (rng.random((E, E)) < 0.5)] = -0.0
    assert (np.signbit(d[5]) & (d[5] == 0)).any()
    return x, None, d


@functools.lru_cache(maxsize=None)
def structure_case(aggr="global_add"):
    """global_add: every node receives gradient, so every structural property shows."""
    cfg = dataclasses.replace(DEFAULT, aggr=aggr)
    return Case("structure " + aggr, cfg, _structure, 7, STRUCT_E)


@functools.lru_cache(maxsize=None)
def slab_case(B):
    return Case("slab B%d" % B, dataclasses.replace(SMALL, aggr="global_mean"), _random(SMALL, B, 3, 1, base=300), B, 3)


SLAB_B = (SLAB, SLAB + 1, 2 * SLAB + 3)
PLAN_CFGS = {"default": {}, "concat": dict(concat=True), "generic": dict(C=12, embed_hidden=20, concat=True)}


@functools.lru_cache(maxsize=None)
def plan_sizes():
    """{plan key: (config name, E)}: the smallest E <= 65 of each distinct (TS, G, instance, accumulator
    placement, adjacency placement) the library's plan produces over PLAN_CFGS."""
    out = {}
    for name, kw in PLAN_CFGS.items():
        cfg = dataclasses.replace(DEFAULT, **kw)
        for E in range(1, 66):
            p, why = plan(cfg, 1, E)
            assert p is not None, (name, E, why)
            out.setdefault(plan_key(p), (name, E))
    return out


@functools.lru_cache(maxsize=None)
def plan_case(key):
    name, E = plan_sizes()[key]
    cfg = dataclasses.replace(DEFAULT, aggr="global_mean", **PLAN_CFGS[name])
    B = key[1] + 1
    return Case("plan %s E%d %s" % (name, E, key), cfg, _random(cfg, B, E, 1, base=500 + E), B, E)


@functools.lru_cache(maxsize=None)
def max_E_case():
    E = largest_E(DEFAULT)
    cfg = dataclasses.replace(DEFAULT, aggr="global_mean")
    return Case("largest E%d" % E, cfg, _random(cfg, 2, E, 1, base=600), 2, E)


def assert_close(out, truth, name, what):
    w64, tol, e32 = truth.want(name)
    err = float(np.abs(out.astype(np.float64) - w64).max()) if w64.size else 0.0
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    gm.RATIOS.append((what + " " + name, ratio))
    print("gnn backward %s %s: err %.3e  e32 %.3e  tol %.3e  err/e32 %.2f" % (what, name, err, e32, tol, ratio))
    assert np.isfinite(out).all(), (what, name)
    assert err <= tol, (what, name, err, tol, e32)


def check(lib, case, device=None, layouts=LAYOUTS):
    """Every conv entry's gradient and dh0 of the entry point against the float64 model within the tolerance, in
    each layout; the EmbedConv range exactly 0; the layouts bit-equal. Returns {layout: result}."""
    outs = {}
    srcs = case.sources(device)
    aid = case.agent_id if case.cfg.aggr == "node" else None
    for layout in layouts:
        r = call(lib, case.cfg, case.blob, case.x, srcs[layout], aid, case.dout)
        assert r["bad"] == 0
        what = "%s %s %s" % ("host" if device is None else "device", case.name, layout)
        got = split(case.cfg, r["dweights"])
        assert not r["dweights"][:conv0(case.cfg)].view(np.int32).any(), "the EmbedConv range is not exactly 0"
        for name in case.truth.names():
            assert_close(r["dh0"] if name == "dh0" else got[name], case.truth, name, what)
        outs[layout] = r
    if len(layouts) == 2:
        a, b = outs[layouts[0]], outs[layouts[1]]
        np.testing.assert_array_equal(a["dweights"].view(np.int32), b["dweights"].view(np.int32))
        np.testing.assert_array_equal(a["dh0"].view(np.int32), b["dh0"].view(np.int32))
    return outs


def structure_checks(lib, device=None):
    """The structural properties the parity check does not show by itself."""
    case = structure_case()
    r = check(lib, case, device)["reference"]
    others = [0, 1, 2, 4, 5, 6]
    # the asymmetric graph 3 against the same call with its transpose in its place: a different dh0 for that
    # graph, the same bytes for every other
    full = case.full.copy()
    full[3] = case.full[3].T
    t = call(lib, case.cfg, case.blob, case.x, ga.dense_sources(full, device)["reference"], None, case.dout)
    assert np.abs(t["dh0"][3] - r["dh0"][3]).max() > 1e-3
    np.testing.assert_array_equal(t["dh0"][others].view(np.int32), r["dh0"][others].view(np.int32))
    # -0.0 entries give the bytes of +0.0: the whole call with graph 5's -0.0 replaced by +0.0
    assert (np.signbit(case.full[5]) & (case.full[5] == 0)).any()
    full = case.full.copy()
    full[5] = np.where(full[5] == 0, np.float32(0.0), full[5])
    r2 = call(lib, case.cfg, case.blob, case.x, ga.dense_sources(full, device)["reference"], None, case.dout)
    np.testing.assert_array_equal(r["dweights"].view(np.int32), r2["dweights"].view(np.int32))
    np.testing.assert_array_equal(r["dh0"].view(np.int32), r2["dh0"].view(np.int32))
    # a target with exactly one incoming edge (2 -> 7 in graph 1): alpha = 1, so da = 0 up to 1e-16 and neither dq
    # of 7 nor dk of 2 through that edge exists. With layer_N = 0 and the node readout at 7, dh0 then comes from
    # the value and skip paths alone: it is independent of the query and key weights.
    cfg = dataclasses.replace(DEFAULT, layer_N=0, aggr="node")
    sd, blob = gm.default_weights(cfg, case.seed)
    ids = np.full(7, 7, np.int64)
    src = case.sources(device)["reference"]
    dout = np.random.default_rng(5).normal(0, 1, (7, cfg.out_dim)).astype(np.float32)
    a = call(lib, cfg, blob, case.x, src, ids, dout)
    got = split(cfg, a["dweights"])
    only = np.zeros_like(case.full)
    only[1] = case.full[1]
    x1 = case.x.copy()
    b = call(lib, cfg, blob, x1, ga.dense_sources(only, device)["reference"], ids, dout)
    gb = split(cfg, b["dweights"])
    # graphs without an edge contribute to the skip path only; graph 1 alone: q and k get nothing at all
    for nm in ("gnn1.lin_query.weight", "gnn1.lin_query.bias", "gnn1.lin_key.weight", "gnn1.lin_key.bias"):
        assert np.abs(gb[nm]).max() <= 1e-16 * 64, (nm, np.abs(gb[nm]).max())
    assert np.abs(gb["gnn1.lin_value.weight"]).max() > 1e-3 and np.abs(got["gnn1.lin_query.weight"]).max() > 1e-6
    # target 5 of graph 1 has no incoming edge: with the readout at 5 only the skip path carries gradient
    ids5 = np.full(7, 5, np.int64)
    c = call(lib, cfg, blob, case.x, ga.dense_sources(only, device)["reference"], ids5, dout)
    gc_ = split(cfg, c["dweights"])
    for nm in gc_:
        if nm.startswith("gnn1.") and "skip" not in nm:
            assert not gc_[nm].view(np.int32).any() or np.abs(gc_[nm]).max() == 0, nm
    assert np.abs(gc_["gnn1.lin_skip.bias"]).max() > 0      # (h0 of node 5 is 0, and with it the skip weight's term)
    assert not c["dh0"][1][np.arange(STRUCT_E) != 5].any() and np.abs(c["dh0"][1][5]).max() > 0
    return r


def bad_input_checks(lib, device=None):
    case = shape_case(24, 1)
    cfg, blob, ids = case.cfg, case.blob, case.agent_id
    src = case.sources(device)["compact"]
    clean = call(lib, cfg, blob, case.x, src, ids, case.dout)
    assert clean["bad"] == 0
    # agent_id = E: no contribution, bad set; the call equals one whose dout row is zero
    ids2 = ids.copy()
    ids2[2] = 24
    out = call(lib, cfg, blob, case.x, src, ids2, case.dout)
    assert out["bad"] == 1 and not out["dh0"][2].view(np.int32).any()
    d0 = case.dout.copy()
    d0[2] = 0
    zero = call(lib, cfg, blob, case.x, src, ids, d0)
    np.testing.assert_array_equal(out["dweights"].view(np.int32) & 0x7fffffff, zero["dweights"].view(np.int32) & 0x7fffffff)
    np.testing.assert_array_equal(out["dh0"][[0, 1, 3, 4]].view(np.int32), clean["dh0"][[0, 1, 3, 4]].view(np.int32))
    # bad is only ever set
    out = call(lib, cfg, blob, case.x, src, ids, case.dout, bad_init=5)
    assert out["bad"] == 5
    np.testing.assert_array_equal(out["dweights"].view(np.int32), clean["dweights"].view(np.int32))
    # a NaN edge: non-finite gradients, a clean finish, the canaries intact (call() checks them)
    c2 = dataclasses.replace(cfg, aggr="global_mean")
    full = case.full.copy()
    r, c = np.argwhere(full[2] == 0)[0]
    full[2, r, c] = np.nan
    out = call(lib, c2, blob, case.x, ga.dense_sources(full, device)["reference"], None, case.dout)
    assert out["bad"] == 0 and not np.isfinite(out["dweights"]).all() and not np.isfinite(out["dh0"][2]).all()
    assert np.isfinite(out["dh0"][[0, 1, 3, 4]]).all()
