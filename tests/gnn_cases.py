"""The graph-encoder tests' cases (shared by tests/test_gnn_capi.py on the host entry point and
tests/test_gpu_gnn.py on the kernel): small graphs in both adjacency layouts with tests/gnn_model.py's
two models computed once per case."""
import dataclasses
import functools

import numpy as np

import gnn_abi as ga
import gnn_model as gm
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
