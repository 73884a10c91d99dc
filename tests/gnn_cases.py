"""The graph-encoder tests' cases (shared by tests/test_gnn_capi.py on the host entry point and
tests/test_gpu_gnn.py on the kernel): small graphs in both adjacency layouts with tests/gnn_model.py's
two models computed once per case."""
import dataclasses
import functools

import numpy as np

import gnn_abi as ga
import gnn_model as gm
import launch_plans as lp
from lsm.gnn import GnnConfig

DEFAULT = GnnConfig(F=11)          # the reference's defaults (onpolicy/config.py:400-446)
SHAPE_E = (1, 3, 24, 65, 192)      # below one wave, across the wave boundary, the workgroup-per-env size
SHAPE_B = (1, 5, 67)               # 67 does not fill the last packed workgroup
BOTH = ("node", "global_mean")


class Case:
    def __init__(self, name, cfg, x, agent_id, aggrs=BOTH, compact=None, dense=None, seed=0):
        self.name, self.cfg, self.x, self.agent_id, self.aggrs, self.seed = name, cfg, x, agent_id, aggrs, seed
        self._compact, self._dense = compact, dense
        self._placed = {}

    def sources(self, device=None):
        if device not in self._placed:
            if self._compact is not None:
                self._placed[device] = ga.sources(*self._compact, device)
            else:
                self._placed[device] = ga.dense_sources(self._dense, device)
        return self._placed[device]

    @property
    def full(self):
        return self.sources(None)["reference"].full

    def weights(self, aggr=None):
        """(state dict, blob): the same for every readout (the entries do not depend on aggr)."""
        return gm.default_weights(self.with_aggr(aggr or self.cfg.aggr), self.seed)

    def with_aggr(self, aggr):
        return dataclasses.replace(self.cfg, aggr=aggr)

    @functools.cached_property
    def ref(self):
        return gm.Reference(self.cfg, self.weights()[0], self.x, self.full)


def ego_ids(B, E):
    """Differing per graph, with 0 and E - 1 among them."""
    ids = (np.arange(B, dtype=np.int64) * 7 + 4) % E
    ids[0], ids[-1] = 0, E - 1
    return ids


@functools.lru_cache(maxsize=None)
def shape_case(E, B):
    N = B if B <= 5 else 1
    x, table, bits = gm.random_graphs(B, E, DEFAULT.F, density=0.1 if E > 100 else 0.4, N=N)
    return Case("shape E%d B%d" % (E, B), DEFAULT, x, ego_ids(B, E), compact=(table, bits, N))


STRUCT_E = 24


@functools.lru_cache(maxsize=None)
def structure_case():
    """Graph 0: no edges at all. 1: target 5 has no incoming edge, target 7 exactly one (alpha = 1), node 9
    neither in nor out edges. 2: a full graph. 3: asymmetric, r -> c only for r < c. 4: -0.0 entries (not
    edges) among ordinary ones."""
    E = STRUCT_E
    rng = np.random.default_rng(5)
    x, table, _ = gm.random_graphs(5, E, DEFAULT.F, seed=3)
    d = np.where(np.isfinite(table) & (table != 7.5), table, 0).astype(np.float32)
    d[0] = 0
    d[1, :, 5] = 0
    d[1, :, 7] = 0
    d[1, 2, 7] = 0.8
    d[1, 9, :] = 0
    d[1, :, 9] = 0
    d[2] = rng.uniform(0.1, 2.0, (E, E))
    d[3] = np.triu(rng.uniform(0.1, 2.0, (E, E)), 1)
    d[4][(d[4] == 0) & (rng.random((E, E)) < 0.5)] = -0.0
    assert (np.signbit(d[4]) & (d[4] == 0)).any() and (d[2] != 0).all() and (d[3].T[d[3] != 0] == 0).all()
    return Case("structure", DEFAULT, x, ego_ids(5, E), dense=d)


OPTIONS = {
    "H1": dict(H=1),
    "concat": dict(concat=True),
    "H1 concat": dict(H=1, concat=True),
    "gnn_layer_N 0": dict(layer_N=0),
    "embed_layer_N 0": dict(embed_layer_N=0),
    "embed_layer_N 2": dict(embed_layer_N=2),
    "tanh": dict(embed_relu=False, relu=False),
    "no layer norm": dict(layer_norm=False),
    "F10": dict(F=10),
    "C12 hidden20": dict(C=12, embed_hidden=20, concat=True),
    "C12 hidden20 tanh mean": dict(C=12, embed_hidden=20, embed_relu=False, relu=False, embed_layer_N=2),
}
OPTION_AGGRS = {"H1": ("node", "global_max"), "concat": ("node", "global_add"), "tanh": ("global_max", "global_add")}


@functools.lru_cache(maxsize=None)
def option_case(name):
    cfg = dataclasses.replace(DEFAULT, **OPTIONS[name])
    x, table, bits = gm.random_graphs(5, 24, cfg.F, seed=1 + sorted(OPTIONS).index(name), N=5)
    return Case("option " + name, cfg, x, ego_ids(5, 24), aggrs=OPTION_AGGRS.get(name, BOTH), compact=(table, bits, 5),
                seed=2)


# ---- one case per launch plan (lsm_gnn_plan, include/lsm_gnn.h) ---------------------------------------------
# The sizes are read from the plan the library computes (tests/launch_plans.py), not restated here: "last" is
# the last E whose adjacency is staged in LDS, "first" the one after it, "max" the largest accepted E.
# tests/test_launch_plans.py asserts that these cases' plans cover every branch of the plan.
GENERIC = dict(C=12, embed_hidden=20)
WIDE = dict(F=64, H=4, C=64, concat=True, embed_hidden=64, embed_layer_N=4, layer_N=4)
PLAN_CASES = {
    "default E33": ({}, 33),                  # TS 64, four graphs per workgroup
    "default E48": ({}, 48),                  # BASELINE config 4's graph
    "default E64": ({}, 64),                  # G cut to 3 by the LDS: a 192-thread workgroup
    "default E99": ({}, 99),                  # G cut to 1
    "default E128": ({}, 128),                # the exact team size
    "default adj_lds last": ({}, "last"),
    "default adj_lds first": ({}, "first"),
    "default E256": ({}, 256),
    "generic E64": (GENERIC, 64),             # the generic instance with G cut (to 3)
    "generic E65": (GENERIC, 65),
    "generic E192": (GENERIC, 192),           # TS 256 without the adjacency in LDS
    "generic adj_lds last": (GENERIC, "last"),
    "generic adj_lds first": (GENERIC, "first"),
    "wide corner max E": (WIDE, "max"),
    # H 4, C 64 without concat: k and v rows of 260 floats; E = 65 does not fit (the largest E that does is
    # found from the plan and is 62), so the case runs at the largest accepted E and 65 is asserted refused
    "H4 C64 max E": (dict(H=4, C=64), "max"),
}
PLAN_SEED = 20


def plan_cfg(name):
    return dataclasses.replace(DEFAULT, **PLAN_CASES[name][0])


def plan_E(name):
    cfg, E = plan_cfg(name), PLAN_CASES[name][1]
    if E == "max":
        return lp.largest_E(cfg)
    if E in ("last", "first"):
        return lp.adj_switch(cfg)[E == "first"]
    return E


def plan_B(name):
    """5, or G + 1 when a packed workgroup takes 5 or more, or 2 at the largest graphs: the smallest batch
    with a partly filled last workgroup."""
    cfg, E = plan_cfg(name), plan_E(name)
    if E == 256:
        return 2
    G = lp.gnn_plan(cfg, 5, E)[0]["G"]
    return 5 if G < 5 else G + 1


def plan_of(name):
    return lp.gnn_plan(plan_cfg(name), plan_B(name), plan_E(name))[0]


@functools.lru_cache(maxsize=None)
def plan_case(name):
    cfg, E, B = plan_cfg(name), plan_E(name), plan_B(name)
    seed = PLAN_SEED + sorted(PLAN_CASES).index(name)
    x, table, bits = gm.random_graphs(B, E, cfg.F, seed=seed, density=0.1 if E > 100 else 0.4, N=B)
    return Case("plan " + name, cfg, x, ego_ids(B, E), compact=(table, bits, B), seed=seed)


def refused_beyond(lib, name, device=None):
    """The case's config one node beyond its largest accepted E: refused with the LDS text, nothing written."""
    case = plan_case(name)
    E = case.x.shape[1] + 1
    x, table, bits = gm.random_graphs(1, E, case.cfg.F, seed=1)
    src = ga.sources(table, bits, 1, device)["reference"]
    ga.run(lib, case.cfg, case.weights()[1], x, src, np.zeros(1, np.int64), bad_init=3, expect_rc=1)
    assert "exceed the LDS" in lib.lsm_gnn_last_error().decode()


def check(lib, case, device=None, layouts=ga.LAYOUTS):
    """Parity of the entry point (host, or the kernel on `device`) with model64 within the measured
    tolerance, in each layout and for each of the case's readouts. Returns {(layout, aggr): out}."""
    outs = {}
    srcs = case.sources(device)
    for layout in layouts:
        for aggr in case.aggrs:
            cfg = case.with_aggr(aggr)
            out, bad = ga.run(lib, cfg, case.weights(aggr)[1], case.x, srcs[layout], case.agent_id)
            assert bad == 0, (case.name, layout, aggr)
            w64, tol, e32 = case.ref.want(cfg, case.agent_id)
            gm.assert_close(out, w64, tol, e32, "%s %s %s %s" % ("host" if device is None else "device", case.name,
                                                                 layout, aggr))
            outs[(layout, aggr)] = out
    return outs


def bad_input_checks(lib, device):
    """Shared with the GPU file: entity types 7 and NaN, agent_id = E, and a NaN edge."""
    case = shape_case(24, 5)
    cfg, blob, ids = case.cfg, case.weights()[1], case.agent_id
    src = case.sources(device)["compact"]
    clean, bad = ga.run(lib, cfg, blob, case.x, src, ids)
    assert bad == 0
    x = case.x.copy()
    x[1, 4, -1] = 7
    x[3, 0, -1] = np.nan
    assert (case.full[1][4] != 0).any() and (case.full[3][0] != 0).any()    # both nodes send messages
    out, bad = ga.run(lib, cfg, blob, x, src, ids)
    assert bad == 1
    ref = gm.Reference(cfg, case.weights()[0], x, case.full)                 # the models use a zero embedding
    gm.assert_close(out, *ref.want(cfg, ids), "bad entity types")
    assert np.abs(out[1] - clean[1]).max() > 0 and np.abs(out[3] - clean[3]).max() > 0
    np.testing.assert_array_equal(out[[0, 2, 4]].view(np.int32), clean[[0, 2, 4]].view(np.int32))
    # agent_id = E: a zero row
    ids2 = ids.copy()
    ids2[2] = 24
    out, bad = ga.run(lib, cfg, blob, case.x, src, ids2)
    assert bad == 1 and not out[2].view(np.int32).any()
    np.testing.assert_array_equal(out[[0, 1, 3, 4]].view(np.int32), clean[[0, 1, 3, 4]].view(np.int32))
    ids2[2] = -1
    out, bad = ga.run(lib, cfg, blob, case.x, src, ids2)
    assert bad == 1 and not out[2].view(np.int32).any()
    # bad is never cleared by the call
    out, bad = ga.run(lib, cfg, blob, case.x, src, ids, bad_init=5)
    assert bad == 5
    np.testing.assert_array_equal(out.view(np.int32), clean.view(np.int32))
    # a NaN edge is an edge; every other graph's row is byte-identical
    for aggr in ("node", "global_mean"):
        c2 = case.with_aggr(aggr)
        ref_src = case.sources(device)["reference"]
        clean, _ = ga.run(lib, c2, blob, case.x, ref_src, ids)
        full = case.full.copy()
        r, c = np.argwhere(full[2] == 0)[0]
        full[2, r, c] = np.nan
        out, bad = ga.run(lib, c2, blob, case.x, ga.dense_sources(full, device)["reference"], ids)
        assert bad == 0
        np.testing.assert_array_equal(out[[0, 1, 3, 4]].view(np.int32), clean[[0, 1, 3, 4]].view(np.int32))
        if aggr == "global_mean":
            assert np.isnan(out[2]).any()     # the edge was not dropped: some node of the graph saw it
