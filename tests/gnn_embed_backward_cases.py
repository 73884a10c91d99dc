"""The cases of EmbedConv's backward tests and the ctypes call (include/lsm_gnn_embed_backward.h), shared by
tests/test_gnn_embed_backward_capi.py (the host entry point) and tests/test_gpu_gnn_embed_backward.py (the
kernel). Every output and the workspace sit between canaries. A case's inputs (weights, graphs, dh0) come from
one seed, the first of at most 50 that tests/gnn_embed_backward_model.py's two models admit; no admissible seed
is an error. Graphs and configs are tests/gnn_backward_cases.py's."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import gnn_abi as ga
import gnn_backward_cases as bc
import gnn_cases as gc
import gnn_embed_backward_model as gem
import gnn_model as gm
import recurrent_abi as ra
from lsm import capi, gnn

DEFAULT = bc.DEFAULT
SLAB = capi.LSM_GNN_BWD_SLAB
SHAPE_E = (1, 3, 24, 33, 65)       # below a wave, TS = 64 and TS = 128
LAYOUTS = ga.LAYOUTS
SEEDS = 50
SMALL = bc.SMALL
OPTIONS = dict(gc.OPTIONS)
OPTIONS["no layer norm tanh"] = dict(layer_norm=False, embed_relu=False)
NO_LN = [k for k, v in gc.OPTIONS.items() if v == dict(layer_norm=False)][0]
OPTION_NAMES = ("embed_layer_N 0", "embed_layer_N 2", "tanh", NO_LN, "F10", "C12 hidden20", "C12 hidden20 tanh mean",
                "no layer norm tanh")
LIMIT = dict(embed_hidden=64, embed_layer_N=4)     # a config whose largest E is below 256
PLAN_CFGS = dict(bc.PLAN_CFGS, limit=LIMIT)


@functools.lru_cache(maxsize=None)
def _lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


def plan(cfg, B, E, N=1, masked=False):
    """(plan dict, None) or (None, the refusal's text) from lsm_gnn_embed_backward_plan."""
    lib, p = _lib(), capi.LsmGnnEmbedBwdLaunchPlan()
    if lib.lsm_gnn_embed_backward_plan(cfg.struct(), B, E, N, int(masked), C.byref(p)):
        return None, lib.lsm_gnn_embed_backward_last_error().decode()
    return {n: int(getattr(p, n)) for n, _ in p._fields_}, None


def plan_key(p):
    return (p["TS"], p["G"], p["fast"], p["acc_lds"], p["adj_lds"])


def largest_E(cfg):
    E = 1
    while E < 256 and plan(cfg, 1, E + 1)[0] is not None:
        E += 1
    return E


def ws_bytes(cfg, B, E):
    return int(_lib().lsm_gnn_embed_backward_workspace_bytes(cfg.struct(), B, E))


def embed_floats(cfg):
    """The number of EmbedConv entries, from the entries' shapes."""
    return bc.conv0(cfg)


def split(cfg, dembed):
    """{name without prefix: array} views of a dembed blob, every EmbedConv entry."""
    out, o = {}, 0
    for name, shape in gnn.weight_entries(cfg):
        if not name.startswith("embed_layer."):
            break
        n = int(np.prod(shape))
        out[name] = dembed[o:o + n].reshape(shape)
        o += n
    assert o == dembed.size
    return out


def _ptr(p):
    return C.c_void_p(p.ptr) if p is not None else None


def call(lib, cfg, blob, node_obs, src, dh0, bad_init=0, expect_rc=0, over=None, io_over=None, fill=None, stream=None):
    """lsm_host_gnn_embed_backward (src.device is None) or lsm_gnn_embed_backward on src.device. Returns a dict:
    dembed [floats] and bad. over: replace B / E / N / weights / io; io_over: replace io fields (None: a null
    pointer; an int or a function of the fields: that address). fill: the words dembed holds before the call
    (the canary by default). A refused call must have written nothing."""
    dev = src.device
    node_obs = np.ascontiguousarray(node_obs, dtype=np.float32)
    B, E = node_obs.shape[0], src.E
    nE = embed_floats(cfg)
    w = ra.Placed(np.ascontiguousarray(blob, dtype=np.float32).view(np.int32), 0, dev)
    x = ra.Placed(node_obs.view(np.int32), 0, dev) if node_obs.size else None
    dh = ra.Placed(np.ascontiguousarray(dh0, dtype=np.float32).view(np.int32).reshape(-1), 0, dev) if np.asarray(dh0).size else None
    de = ra.destination(nE, 0, dev)
    if fill is not None:
        host = np.full(ra.PRE + nE + ra.TAIL, ra.CANARY, np.int32)
        host[ra.PRE:ra.PRE + nE] = fill
        de = (ra.Placed(host, 0, dev), nE)
    nws = max(ws_bytes(cfg, B, E) // 4, 2)
    ws = ra.destination(nws, 0, dev)
    bad = ra.Placed(np.array([bad_init], np.int64).view(np.int32), 0, dev)
    fields = dict(node_obs=_ptr(x), adj=_ptr(src.adj), masks=_ptr(src.masks), dh0=_ptr(dh),
                  dembed=C.c_void_p(de[0].ptr + 4 * ra.PRE), workspace=C.c_void_p(ws[0].ptr + 4 * ra.PRE), bad=_ptr(bad))
    for k, v in (io_over or {}).items():
        fields[k] = None if v is None else C.c_void_p(v(fields) if callable(v) else v)
    io = capi.LsmGnnEmbedBwdIo(**fields)
    args = dict(weights=_ptr(w), io=C.byref(io), B=B, E=E, N=src.N)
    args.update(over or {})
    a = (cfg.struct(), args["weights"], args["io"], args["B"], args["E"], args["N"])
    if dev is None:
        rc = lib.lsm_host_gnn_embed_backward(*a)
    else:
        import torch
        s = torch.cuda.current_stream() if stream is None else stream
        rc = lib.lsm_gnn_embed_backward(*a, C.c_void_p(s.cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_gnn_embed_backward_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    dew = ra.read_destination(de, "dembed")
    ra.read_destination(ws, "workspace")
    badv = int(bad.read().view(np.int64)[0])
    if expect_rc:
        assert err.startswith("gnn embed backward: ") and len(err) > len("gnn embed backward: "), err
        assert (dew == (ra.CANARY if fill is None else fill)).all(), "a refused call wrote"
        assert badv == bad_init
        return dict(err=err)
    if B == 0:
        assert (dew == (ra.CANARY if fill is None else fill)).all()
        return dict(bad=badv)
    return dict(dembed=dew.view(np.float32).copy(), bad=badv)


class Case:
    """cfg, inputs made by make(seed) -> (x, compact triple or None, dense or None), and the first admissible
    seed's weights, dh0 and truth."""

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
            dh0 = np.random.default_rng(6000 + seed).normal(0, 1, (self.B, self.E, self.cfg.embed_hidden)).astype(np.float32)
            truth = gem.Truth(self.cfg, sd, x, full, dh0)
            if truth.why_not is None:
                return dict(seed=seed, x=x, compact=compact, dense=dense, full=full, sd=sd, blob=blob, dh0=dh0,
                            truth=truth)
            why.append(truth.why_not)
        raise AssertionError("%s: no admissible seed among %d (%s)" % (self.name, SEEDS, sorted(set(why))))

    def __getattr__(self, k):
        if k in ("seed", "x", "full", "sd", "blob", "dh0", "truth", "compact"):
            return self._found[k]
        raise AttributeError(k)

    def sources(self, device=None):
        if device not in self._placed:
            f = self._found
            self._placed[device] = (ga.sources(*f["compact"], device) if f["compact"] is not None
                                    else ga.dense_sources(f["dense"], device))
        return self._placed[device]


def group_B(cfg, E):
    """G + 1: one graph more than a workgroup takes at a time."""
    return plan(cfg, 1, E)[0]["G"] + 1


@functools.lru_cache(maxsize=None)
def shape_case(E, which):
    """which: 0 -> B = 1, 1 -> B = 5, 2 -> B = G + 1."""
    B = (1, 5, group_B(DEFAULT, E))[which]
    N = B if B <= 5 else 1
    return Case("shape E%d B%d" % (E, B), DEFAULT, bc._random(DEFAULT, B, E, N), B, E)


@functools.lru_cache(maxsize=None)
def option_case(name):
    cfg = dataclasses.replace(DEFAULT, **OPTIONS[name])
    return Case("option %s" % name, cfg, bc._random(cfg, 5, 24, 5, base=100 + 50 * OPTION_NAMES.index(name)), 5, 24)


STRUCT_E = bc.STRUCT_E


@functools.lru_cache(maxsize=None)
def structure_case():
    return Case("structure", DEFAULT, bc._structure, 7, STRUCT_E)


@functools.lru_cache(maxsize=None)
def slab_case(B):
    return Case("slab B%d" % B, SMALL, bc._random(SMALL, B, 3, 1, base=300), B, 3)


SLAB_B = (SLAB, SLAB + 1, 2 * SLAB + 3)


def _poisoned(seed):
    """Four graphs of two envs (N = 2) in which nodes 3 and 10 are disconnected for both egos of every env, with
    inf / 7.5 in the table's rows and columns under those bits (gnn_model.random_graphs' rule, forced)."""
    E = 24
    x, table, bits = gm.random_graphs(4, E, DEFAULT.F, seed=800 + seed, N=2)
    bits[:, [3, 10]] = True
    poison = np.where((np.arange(E)[:, None] + np.arange(E)[None, :]) % 2 == 0, np.float32(np.inf), np.float32(7.5))
    for n in (3, 10):
        table[:, n, :] = poison[n, :]
        table[:, :, n] = poison[:, n]
    return x, (table, bits, 2), None


@functools.lru_cache(maxsize=None)
def poison_case():
    return Case("poison", DEFAULT, _poisoned, 4, 24)


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
    cfg = dataclasses.replace(DEFAULT, **PLAN_CFGS[name])
    B = key[1] + 1
    return Case("plan %s E%d %s" % (name, E, key), cfg, bc._random(cfg, B, E, 1, base=500 + E), B, E)


@functools.lru_cache(maxsize=None)
def limit_cfg():
    """The defaults when they have a largest E below 256, else LIMIT's config."""
    return DEFAULT if largest_E(DEFAULT) < 256 else dataclasses.replace(DEFAULT, **LIMIT)


@functools.lru_cache(maxsize=None)
def max_E_case():
    cfg = limit_cfg()
    E = largest_E(cfg)
    return Case("largest E%d" % E, cfg, bc._random(cfg, 2, E, 1, base=600), 2, E)


def assert_close(out, truth, name, what):
    w64, tol, e32 = truth.want(name)
    err = float(np.abs(out.astype(np.float64) - w64).max()) if w64.size else 0.0
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    gm.RATIOS.append((what + " " + name, ratio))
    print("gnn embed backward %s %s: err %.3e  e32 %.3e  tol %.3e  err/e32 %.2f" % (what, name, err, e32, tol, ratio))
    assert np.isfinite(out).all(), (what, name)
    assert err <= tol, (what, name, err, tol, e32)


def compare(cfg, dembed, truth, what):
    """Every EmbedConv entry's gradient against the float64 model within the tolerance; without layer norm the
    gamma and beta entries exactly 0."""
    got = split(cfg, dembed)
    for name in truth.names():
        assert_close(got[name], truth, name, what)
    if not cfg.layer_norm:
        for name in ("embed_layer.layer_norm.weight", "embed_layer.layer_norm.bias"):
            assert not got[name].view(np.int32).any(), "%s is not exactly 0" % name


def check(lib, case, device=None, layouts=LAYOUTS):
    """The entry point against the model in each layout; the layouts bit-equal. Returns {layout: result}."""
    outs = {}
    srcs = case.sources(device)
    for layout in layouts:
        r = call(lib, case.cfg, case.blob, case.x, srcs[layout], case.dh0)
        assert r["bad"] == 0
        compare(case.cfg, r["dembed"], case.truth, "%s %s %s" % ("host" if device is None else "device", case.name, layout))
        outs[layout] = r
    if len(layouts) == 2:
        np.testing.assert_array_equal(outs[layouts[0]]["dembed"].view(np.int32), outs[layouts[1]]["dembed"].view(np.int32))
    return outs


def _same(a, b):
    np.testing.assert_array_equal(a["dembed"].view(np.int32), b["dembed"].view(np.int32))


def structure_checks(lib, device=None):
    """The structural properties: each compares one call with another, bit-equal; the last is an exact value."""
    case = structure_case()
    cfg, blob, x, full, dh0 = case.cfg, case.blob, case.x, case.full, case.dh0
    r = check(lib, case, device)["reference"]
    ref = lambda f: ga.dense_sources(f, device)["reference"]
    # the edgeless graph 0 adds nothing to any entry: the call without it
    assert not full[0].any()
    _same(r, call(lib, cfg, blob, x[1:], ref(full[1:]), dh0[1:]))
    # a node that is never a source adds nothing, whatever its features: node 4 of graph 6, its row cleared
    f2 = full.copy()
    f2[6, 4, :] = 0
    assert f2[6, :, 4].any() and f2[6].any()
    a = call(lib, cfg, blob, x, ref(f2), dh0)
    x2 = x.copy()
    x2[6, 4, :cfg.F - 1] = np.array([np.nan, 1e30, -7.0] + [3.0] * (cfg.F - 4), np.float32)
    _same(a, call(lib, cfg, blob, x2, ref(f2), dh0))
    assert np.isfinite(a["dembed"]).all() and np.abs(a["dembed"] - r["dembed"]).max() > 0
    # a target without an incoming edge (5 of graph 1) makes its dh0 row irrelevant
    assert not full[1, :, 5].any()
    d2 = dh0.copy()
    d2[1, 5] = np.array([np.inf, np.nan, 1e20] + [-2.0] * (cfg.embed_hidden - 3), np.float32)
    _same(r, call(lib, cfg, blob, x, ref(full), d2))
    # -0.0 entries give the bytes of +0.0
    assert (np.signbit(full[5]) & (full[5] == 0)).any()
    f3 = full.copy()
    f3[5] = np.where(f3[5] == 0, np.float32(0.0), f3[5])
    _same(r, call(lib, cfg, blob, x, ref(f3), dh0))
    # an entity type that no node carries leaves its entity_embed row exactly 0
    x3 = x.copy()
    x3[:, :, cfg.F - 1] = x3[:, :, cfg.F - 1] % 3
    got = split(cfg, call(lib, cfg, blob, x3, ref(full), dh0)["dembed"])["embed_layer.entity_embed.weight"]
    assert not got[3].view(np.int32).any() and all(np.abs(got[t]).max() > 0 for t in range(3))
    return r


def linearity_check(lib, device=None):
    """A dh0 that is zero except on one graph equals that graph's own call."""
    case = shape_case(24, 1)
    src = case.sources(device)["reference"]
    for g in (0, 3):
        d = np.zeros_like(case.dh0)
        d[g] = case.dh0[g]
        a = call(lib, case.cfg, case.blob, case.x, src, d)
        own = ga.dense_sources(case.full[g:g + 1], device)["reference"]
        _same(a, call(lib, case.cfg, case.blob, case.x[g:g + 1], own, case.dh0[g:g + 1]))
        assert np.abs(a["dembed"]).max() > 0


def bad_input_checks(lib, device=None):
    case = shape_case(24, 1)
    cfg, blob = case.cfg, case.blob
    srcs = case.sources(device)
    src = srcs["compact"]
    clean = call(lib, cfg, blob, case.x, src, case.dh0)
    assert clean["bad"] == 0
    # inf / 7.5 under the common disconnect bits of the compact table: never read as edges (check() compares the
    # compact call with the model and with the reference layout's bytes)
    pc = poison_case()
    table, bits, N = pc.compact
    common = bits.reshape(-1, N, pc.E).all(axis=1)
    assert common[:, [3, 10]].all() and np.isinf(table[:, 3]).any() and (table[:, :, 10] == 7.5).any()
    check(lib, pc, device)
    # invalid entity types (NaN, -1, num_embeddings) on nodes that are sources: bad is set, the node contributes a
    # zero embedding to lin1 and nothing to entity_embed -- the model's rule, so the call is judged against the
    # model on these inputs
    x = case.x.copy()
    outdeg = (case.full != 0).sum(axis=2)
    nodes = [(g, int(np.argmax(outdeg[g]))) for g in (0, 2, 4)]
    for (g, r), t in zip(nodes, (np.nan, -1.0, float(cfg.num_embeddings))):
        assert outdeg[g, r] > 0
        x[g, r, cfg.F - 1] = t
    truth = gem.Truth(cfg, case.sd, x, case.full, case.dh0)
    assert truth.why_not is None
    out = call(lib, cfg, blob, x, src, case.dh0)
    assert out["bad"] == 1
    compare(cfg, out["dembed"], truth, "%s bad types" % ("host" if device is None else "device"))
    _same(out, call(lib, cfg, blob, x, srcs["reference"], case.dh0))
    # bad is only ever set
    out = call(lib, cfg, blob, case.x, src, case.dh0, bad_init=5)
    assert out["bad"] == 5
    _same(out, clean)
    # a NaN edge: non-finite entries, a clean finish, the canaries intact (call() checks them)
    full = case.full.copy()
    r, c = np.argwhere(full[2] == 0)[0]
    full[2, r, c] = np.nan
    out = call(lib, cfg, blob, case.x, ga.dense_sources(full, device)["reference"], case.dh0)
    assert out["bad"] == 0 and not np.isfinite(out["dembed"]).all()


def slab_check(lib, device=None):
    """A call on 2 * SLAB + 3 graphs equals, to float64 rounding, the float64 sum of its three slabs' own calls."""
    case = slab_case(2 * SLAB + 3)
    src = case.sources(device)["reference"]
    whole = call(lib, case.cfg, case.blob, case.x, src, case.dh0)
    parts = []
    for lo in range(0, case.B, SLAB):
        hi = min(lo + SLAB, case.B)
        s = ga.dense_sources(case.full[lo:hi], device)["reference"]
        parts.append(call(lib, case.cfg, case.blob, case.x[lo:hi], s, case.dh0[lo:hi])["dembed"])
    want = np.sum(np.asarray(parts, dtype=np.float64), axis=0)
    got = whole["dembed"].astype(np.float64)
    # each part was rounded to float32 once (2^-24 relative each), the whole once
    assert np.abs(got - want).max() <= 4 * 2.0 ** -24 * np.abs(np.asarray(parts)).max()
    return whole
