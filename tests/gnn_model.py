"""Independent statements of GNNBase.forward (include/lsm_gnn.h restates the formulas; torch_geometric
is not needed) for the graph-encoder tests, plus seeded weights and graphs. Nothing here comes from
the code under test.

model64        numpy float64, loops over graphs and targets
model32_torch  the same on the edge list of nonzero(), float32 torch ops on the CPU
bound          the tests' tolerance, measured per case: 4 * e32 + 4 * 2^-23 * s with
               e32 = max |model32_torch - model64| and s = max |model64|. The factor 4 allows for a
               different but fixed summation order over at most 256 incoming edges and four layers;
               the second term covers cases model32_torch gets exactly right.

A state dict `sd` maps the reference's parameter names (prefix "gnn.") to float32 arrays. Both models
use a zero embedding for an entity type outside [0, num_embeddings) and a zero row for an agent_id
outside [0, E), as the header specifies."""
import functools

import numpy as np

from lsm import gnn

PREFIX = "gnn."


def random_weights(cfg, seed=0):
    """Seeded state dict: lin1 and the conv weights at O(1) output scale (rows ~ U(-1, 1) * 1.5 /
    sqrt(fan_in)) so the softmax is neither uniform nor one-hot; a non-trivial layer-norm gamma / beta."""
    rng = np.random.default_rng(1000 + seed)
    sd = {}
    for name, shape in gnn.weight_entries(cfg):
        if ".layer_norm." in name:
            if not cfg.layer_norm:
                continue
            a = 1.0 + 0.3 * rng.normal(size=shape) if name.endswith("weight") else 0.2 * rng.normal(size=shape)
        elif name.endswith("entity_embed.weight"):
            a = rng.normal(size=shape)
        elif name.endswith("lin_edge.weight"):
            a = 0.5 * rng.normal(size=shape)
        elif name.endswith("bias"):
            a = 0.3 * rng.normal(size=shape)
        else:
            a = rng.uniform(-1, 1, size=shape) * 1.5 / np.sqrt(shape[1])
        sd[PREFIX + name] = a.astype(np.float32)
    return sd


def random_graphs(B, E, F, seed=0, density=0.4, N=1):
    """Seeded graphs in the compact statement: node_obs [B, E, F] float32 (entity types 0 .. 3 in the
    last column), table [B / N, E, E] with `density` of its entries nonzero (distances in (0.1, 2)), bits
    [B, E] bool disconnect bits (15 %), with inf / 7.5 in the table under bits common to an env's egos
    (a select gives 0 there, a product would not)."""
    assert B % N == 0
    rng = np.random.default_rng(77 * E + B + 100000 * seed)
    x = rng.normal(0, 1, (B, E, F)).astype(np.float32)
    x[:, :, F - 1] = rng.integers(0, 4, (B, E))
    table = rng.uniform(0.1, 2.0, (B // N, E, E)).astype(np.float32)
    table[rng.random(table.shape) >= density] = 0
    bits = rng.random((B, E)) < 0.15
    common = bits.reshape(B // N, N, E).all(axis=1)
    under = common[:, :, None] | common[:, None, :]
    poison = np.where((np.arange(E)[:, None] + np.arange(E)[None, :]) % 2 == 0, np.float32(np.inf), np.float32(7.5))
    table = np.where(under, poison, table).astype(np.float32)
    return x, table, bits


def _act(v, relu):
    return np.maximum(v, 0) if relu else np.tanh(v)


def _params(cfg, sd, dtype):
    return {k[len(PREFIX):]: np.asarray(v).astype(dtype) for k, v in sd.items() if k.startswith(PREFIX)}


def _conv_names(cfg):
    return ["gnn1"] + ["gnn2.%d" % i for i in range(cfg.layer_N)]


def _entity(cfg, types):
    """(index, valid) of node_obs' last column: trunc, valid when finite and in [0, num_embeddings)."""
    t = np.asarray(types, dtype=np.float64)
    fin = np.isfinite(t)
    ti = np.trunc(np.where(fin, t, -1)).astype(np.int64)
    ok = fin & (ti >= 0) & (ti < cfg.num_embeddings)
    return np.where(ok, ti, 0), ok


def readout(cfg, nodes, agent_id):
    """[B, E, D] node features -> [B, D]."""
    B, E, D = nodes.shape
    if cfg.aggr == "node":
        out = np.zeros((B, D), nodes.dtype)
        ids = np.asarray(agent_id).reshape(B)
        for b in range(B):
            if 0 <= ids[b] < E:
                out[b] = nodes[b, int(ids[b])]
        return out
    return {"global_mean": nodes.mean(axis=1), "global_max": nodes.max(axis=1), "global_add": nodes.sum(axis=1)}[cfg.aggr]


def nodes64(cfg, sd, node_obs, adj):
    """[B, E, out_dim] float64: every node's features after the last layer."""
    p = _params(cfg, sd, np.float64)
    B, E, F = node_obs.shape
    H, C, D, Hd = cfg.H, cfg.C, cfg.out_dim, cfg.embed_hidden
    x = node_obs.astype(np.float64)
    out = np.zeros((B, E, D))

    def ln(v):
        if not cfg.layer_norm:
            return v
        mu = v.mean(axis=-1, keepdims=True)
        var = ((v - mu) ** 2).mean(axis=-1, keepdims=True)
        return (v - mu) / np.sqrt(var + 1e-5) * p["embed_layer.layer_norm.weight"] + p["embed_layer.layer_norm.bias"]

    for b in range(B):
        a = adj[b]
        edge = a != 0                      # NaN != 0, -0.0 == 0: nonzero()
        a = a.astype(np.float64)
        ti, ok = _entity(cfg, node_obs[b, :, F - 1])
        emb = p["embed_layer.entity_embed.weight"][ti] * ok[:, None]
        h = np.zeros((E, Hd))
        for c in range(E):
            src = np.nonzero(edge[:, c])[0]
            if len(src) == 0:
                continue
            cat = np.concatenate([x[b, src, :F - 1], emb[src], a[src, c][:, None]], axis=1)
            m = ln(_act(cat @ p["embed_layer.lin1.weight"].T + p["embed_layer.lin1.bias"], cfg.embed_relu))
            for k in range(cfg.embed_layer_N):
                m = m @ p["embed_layer.layers.%d.weight" % (3 * k)].T + p["embed_layer.layers.%d.bias" % (3 * k)]
                m = ln(_act(m, cfg.embed_relu))
            h[c] = m.sum(axis=0)
        for conv in _conv_names(cfg):
            lin = lambda nm, v: v @ p["%s.lin_%s.weight" % (conv, nm)].T + p["%s.lin_%s.bias" % (conv, nm)]
            q, k, v = (lin(nm, h).reshape(E, H, C) for nm in ("query", "key", "value"))
            skip = lin("skip", h)
            we = p["%s.lin_edge.weight" % conv][:, 0]
            new = np.zeros((E, D))
            for c in range(E):
                src = np.nonzero(edge[:, c])[0]
                o = np.zeros((H, C))
                if len(src):
                    ee = (a[src, c][:, None] * we[None, :]).reshape(-1, H, C)
                    logit = (q[c][None] * (k[src] + ee)).sum(axis=-1) / np.sqrt(C)      # [deg, H]
                    pexp = np.exp(logit - logit.max(axis=0, keepdims=True))
                    alpha = pexp / (pexp.sum(axis=0, keepdims=True) + 1e-16)
                    o = (alpha[:, :, None] * (v[src] + ee)).sum(axis=0)
                merged = o.reshape(H * C) if cfg.concat else o.mean(axis=0)
                new[c] = _act(merged + skip[c], cfg.relu)
            h = new
        out[b] = h
    return out


def model64(cfg, sd, node_obs, adj, agent_id=None):
    with np.errstate(all="ignore"):
        return readout(cfg, nodes64(cfg, sd, node_obs, adj), agent_id)


def nodes32_torch(cfg, sd, node_obs, adj):
    """[B, E, out_dim] float32: the edge-list formulation with torch ops on the CPU."""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.from_numpy(v) for k, v in _params(cfg, sd, np.float32).items()}
    B, E, F = node_obs.shape
    H, C, D, Hd = cfg.H, cfg.C, cfg.out_dim, cfg.embed_hidden
    act_e = torch.relu if cfg.embed_relu else torch.tanh
    act_g = torch.relu if cfg.relu else torch.tanh
    adj_t = torch.from_numpy(np.ascontiguousarray(adj, dtype=np.float32))
    idx = (adj_t != 0).nonzero()
    src, dst = idx[:, 0] * E + idx[:, 1], idx[:, 0] * E + idx[:, 2]
    e = adj_t[idx[:, 0], idx[:, 1], idx[:, 2]].unsqueeze(1)
    x = torch.from_numpy(np.ascontiguousarray(node_obs, dtype=np.float32)).reshape(B * E, F)
    ti, ok = _entity(cfg, node_obs.reshape(B * E, F)[:, F - 1])
    emb = p["embed_layer.entity_embed.weight"][torch.from_numpy(ti)] * torch.from_numpy(ok).unsqueeze(1)

    def ln(v):
        if not cfg.layer_norm:
            return v
        return Fn.layer_norm(v, (Hd,), p["embed_layer.layer_norm.weight"], p["embed_layer.layer_norm.bias"], 1e-5)

    m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
    m = ln(act_e(Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])))
    for k in range(cfg.embed_layer_N):
        m = ln(act_e(Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)], p["embed_layer.layers.%d.bias" % (3 * k)])))
    h = torch.zeros(B * E, Hd).index_add_(0, dst, m)
    for conv in _conv_names(cfg):
        lin = lambda nm, v: Fn.linear(v, p["%s.lin_%s.weight" % (conv, nm)], p["%s.lin_%s.bias" % (conv, nm)])
        q, k, v = (lin(nm, h).view(-1, H, C) for nm in ("query", "key", "value"))
        ee = Fn.linear(e, p["%s.lin_edge.weight" % conv]).view(-1, H, C)
        kj = k.index_select(0, src) + ee
        logit = (q.index_select(0, dst) * kj).sum(dim=-1) / float(np.sqrt(C))
        amax = torch.full((B * E, H), -float("inf")).scatter_reduce_(0, dst.unsqueeze(1).expand(-1, H), logit, "amax")
        pexp = torch.exp(logit - amax.index_select(0, dst))
        den = torch.zeros(B * E, H).index_add_(0, dst, pexp)
        alpha = pexp / (den.index_select(0, dst) + 1e-16)
        o = torch.zeros(B * E, H, C).index_add_(0, dst, alpha.unsqueeze(-1) * (v.index_select(0, src) + ee))
        o = o.reshape(B * E, H * C) if cfg.concat else o.mean(dim=1)
        h = act_g(o + lin("skip", h))
    return h.view(B, E, D).numpy()


def model32_torch(cfg, sd, node_obs, adj, agent_id=None):
    return readout(cfg, nodes32_torch(cfg, sd, node_obs, adj), agent_id)


class Reference:
    """Both models' node features of one case, computed once; bound() / want() per readout."""

    def __init__(self, cfg, sd, node_obs, adj):
        self.cfg = cfg
        with np.errstate(all="ignore"):
            self.n64 = nodes64(cfg, sd, node_obs, adj)
        self.n32 = nodes32_torch(cfg, sd, node_obs, adj)

    def want(self, cfg, agent_id=None):
        """(model64 output, the tolerance, e32) for cfg's readout (cfg differs from the stored one in aggr only)."""
        w64 = readout(cfg, self.n64, agent_id)
        w32 = readout(cfg, self.n32, agent_id)
        e32 = float(np.abs(w32 - w64).max())
        return w64, bound(w64, e32), e32


def bound(w64, e32):
    return 4.0 * e32 + 4.0 * 2.0 ** -23 * float(np.abs(w64).max())


RATIOS = []   # (what, max |out - model64| / e32) of every comparison made in this session


def assert_close(out, w64, tol, e32, what, rows=None):
    """max |out - model64| <= tol over `rows` (all by default); prints the figures first."""
    sel = slice(None) if rows is None else rows
    err = float(np.abs(out[sel].astype(np.float64) - w64[sel]).max()) if out[sel].size else 0.0
    ratio = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    RATIOS.append((what, ratio))
    print("gnn %s: err %.3e  e32 %.3e  tol %.3e  err/e32 %.2f" % (what, err, e32, tol, ratio))
    assert np.isfinite(out[sel]).all(), what
    assert err <= tol, (what, err, tol, e32)


@functools.lru_cache(maxsize=None)
def default_weights(cfg, seed=0):
    """The case's state dict and its packed blob (GnnConfig is hashable)."""
    sd = random_weights(cfg, seed)
    return sd, gnn.pack_weights(sd, cfg)
