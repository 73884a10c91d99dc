"""The yardstick of the graph encoder's backward tests (include/lsm_gnn_backward.h): tests/gnn_model.py's
edge-list formulas as torch ops in a given dtype, differentiated by torch.autograd. Nothing here comes from the
code under test.

EmbedConv runs without a graph and its output h0 becomes a leaf, as do the conv parameters; the conv layers and
the readout run with the graph kept, and torch.autograd.backward([out], [dout]) gives the gradient of every
conv parameter and dh0. float64 is the truth; the same in float32 gives e32, the error a float32 evaluation
of the same formulas makes, and the tests' tolerance per gradient tensor is gnn_model.bound's:
4 * e32 + 4 * 2^-23 * max |truth|.

torch_geometric is not needed: the formulas are lsm_gnn.h's restatement of TransformerConv, pinned to
gnn_model.nodes64 by tests/test_gnn_backward_capi.py."""
import numpy as np
import torch
import torch.nn.functional as Fn

import gnn_model as gm

PREFIX = gm.PREFIX
NEAR = 2.0 ** -17      # admission: how close to a kink a float64 value may lie


def conv_names(cfg):
    """The state-dict names (without prefix) of the conv layers' parameters, in the blob's order."""
    out = []
    for conv in gm._conv_names(cfg):
        for lin in ("query", "key", "value"):
            out += ["%s.lin_%s.weight" % (conv, lin), "%s.lin_%s.bias" % (conv, lin)]
        out += ["%s.lin_edge.weight" % conv, "%s.lin_skip.weight" % conv, "%s.lin_skip.bias" % conv]
    return out


class Result:
    """One dtype's run: nodes [B, E, D] (the last layer's output), pre [L + 1][B, E, D] (each conv layer's
    pre-activation), h0, out [B, D], grads {name without prefix: array}, dh0 [B, E, Hd], and for global_max
    the per (graph, column) winner and its margin over the runner-up."""


def run(cfg, sd, node_obs, adj, dout, agent_id=None, dtype=torch.float64):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    p = {k: torch.from_numpy(v) for k, v in gm._params(cfg, sd, npdt).items()}
    B, E, F = node_obs.shape
    H, C, D, Hd = cfg.H, cfg.C, cfg.out_dim, cfg.embed_hidden
    act_e = torch.relu if cfg.embed_relu else torch.tanh
    act_g = torch.relu if cfg.relu else torch.tanh
    adj32 = torch.from_numpy(np.ascontiguousarray(adj, dtype=np.float32))
    idx = (adj32 != 0).nonzero()                       # NaN is an edge, -0.0 is not
    src, dst = idx[:, 0] * E + idx[:, 1], idx[:, 0] * E + idx[:, 2]
    e = adj32[idx[:, 0], idx[:, 1], idx[:, 2]].unsqueeze(1).to(dtype)
    x = torch.from_numpy(np.ascontiguousarray(node_obs, dtype=np.float32)).reshape(B * E, F).to(dtype)
    ti, ok = gm._entity(cfg, node_obs.reshape(B * E, F)[:, F - 1])
    emb = p["embed_layer.entity_embed.weight"][torch.from_numpy(ti)] * torch.from_numpy(ok).unsqueeze(1).to(dtype)

    def ln(v):
        if not cfg.layer_norm:
            return v
        return Fn.layer_norm(v, (Hd,), p["embed_layer.layer_norm.weight"], p["embed_layer.layer_norm.bias"], 1e-5)

    with torch.no_grad():
        m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
        m = ln(act_e(Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])))
        for k in range(cfg.embed_layer_N):
            m = ln(act_e(Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)],
                                   p["embed_layer.layers.%d.bias" % (3 * k)])))
        h0 = torch.zeros(B * E, Hd, dtype=dtype).index_add_(0, dst, m)
    h0.requires_grad_(True)
    names = conv_names(cfg)
    for nm in names:
        p[nm] = p[nm].clone().requires_grad_(True)

    h, pre = h0, []
    for conv in gm._conv_names(cfg):
        lin = lambda nm, v: Fn.linear(v, p["%s.lin_%s.weight" % (conv, nm)], p["%s.lin_%s.bias" % (conv, nm)])
        q, k, v = (lin(nm, h).view(-1, H, C) for nm in ("query", "key", "value"))
        ee = Fn.linear(e, p["%s.lin_edge.weight" % conv]).view(-1, H, C)
        kj = k.index_select(0, src) + ee
        logit = (q.index_select(0, dst) * kj).sum(dim=-1) / float(np.sqrt(C))
        amax = torch.full((B * E, H), -float("inf"), dtype=dtype).scatter_reduce_(
            0, dst.unsqueeze(1).expand(-1, H), logit.detach(), "amax")
        pexp = torch.exp(logit - amax.index_select(0, dst))
        den = torch.zeros(B * E, H, dtype=dtype).index_add(0, dst, pexp)
        alpha = pexp / (den.index_select(0, dst) + 1e-16)
        o = torch.zeros(B * E, H, C, dtype=dtype).index_add(0, dst, alpha.unsqueeze(-1) * (v.index_select(0, src) + ee))
        o = o.reshape(B * E, H * C) if cfg.concat else o.mean(dim=1)
        z = o + lin("skip", h)
        pre.append(z.detach().view(B, E, D).numpy())
        h = act_g(z)
    nodes = h.view(B, E, D)

    res = Result()
    if cfg.aggr == "node":
        ids = torch.from_numpy(np.asarray(agent_id, dtype=np.int64).reshape(B))
        valid = (ids >= 0) & (ids < E)
        out = nodes[torch.arange(B), torch.where(valid, ids, torch.zeros_like(ids))] * valid.unsqueeze(1).to(dtype)
    elif cfg.aggr == "global_mean":
        out = nodes.mean(dim=1)
    elif cfg.aggr == "global_add":
        out = nodes.sum(dim=1)
    else:
        out, win = nodes.max(dim=1)
        res.winner = win.numpy()
        if E > 1:
            top2 = nodes.detach().topk(2, dim=1).values
            res.margin = (top2[:, 0] - top2[:, 1]).numpy()
        else:
            res.margin = np.full((B, D), np.inf)
    torch.autograd.backward([out], [torch.from_numpy(np.ascontiguousarray(dout)).to(dtype)])
    res.nodes, res.pre, res.h0, res.out = nodes.detach().numpy(), pre, h0.detach().view(B, E, Hd).numpy(), out.detach().numpy()
    res.grads = {nm: (p[nm].grad if p[nm].grad is not None else torch.zeros_like(p[nm])).numpy() for nm in names}
    res.dh0 = (h0.grad if h0.grad is not None else torch.zeros_like(h0)).view(B, E, Hd).numpy()
    return res


def admissible(cfg, r64, r32):
    """None when the two models admit the case, else the reason (the rules of the issue, decided from the two
    models alone). 1: under ReLU no conv pre-activation lies within 2^-17 of 0 and the float32 model is on the
    same side of 0 everywhere (at a kink the subgradient is a convention, and a float32 evaluation on the other
    side differs by a whole term, not by rounding). 2: under global_max both models pick the same node per
    (graph, column) with the runner-up more than 2^-17 below."""
    if cfg.relu:
        for a, b in zip(r64.pre, r32.pre):
            if (np.abs(a) < NEAR).any():
                return "a pre-activation within 2^-17 of 0"
            if ((a > 0) != (b > 0)).any():
                return "the float32 model is on the other side of 0"
    if cfg.aggr == "global_max":
        if (r64.winner != r32.winner).any():
            return "the models pick different nodes"
        if (r64.margin <= NEAR).any() or (r32.margin <= NEAR).any():
            return "the runner-up is within 2^-17"
    return None


class Truth:
    """Both models of one case: want(name) -> (truth64, tol, e32) per gradient tensor; names() lists them all
    ('dh0' included)."""

    def __init__(self, cfg, sd, node_obs, adj, dout, agent_id=None):
        self.cfg = cfg
        with np.errstate(all="ignore"):
            self.r64 = run(cfg, sd, node_obs, adj, dout, agent_id, torch.float64)
            self.r32 = run(cfg, sd, node_obs, adj, dout, agent_id, torch.float32)
        self.why_not = admissible(cfg, self.r64, self.r32)

    def names(self):
        return conv_names(self.cfg) + ["dh0"]

    def want(self, name):
        a = self.r64.dh0 if name == "dh0" else self.r64.grads[name]
        b = self.r32.dh0 if name == "dh0" else self.r32.grads[name]
        e32 = float(np.abs(b.astype(np.float64) - a).max()) if a.size else 0.0
        return a, gm.bound(a, e32) if a.size else 0.0, e32
