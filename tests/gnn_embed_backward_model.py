"""The yardstick of EmbedConv's backward tests (include/lsm_gnn_embed_backward.h): tests/gnn_model.py's
edge-list EmbedConv as torch ops in a given dtype, every EmbedConv parameter a leaf, differentiated by
torch.autograd.backward([h0], [dh0]). Nothing here comes from the code under test.

float64 is the truth; the same in float32 gives e32, the error a float32 evaluation of the same formulas makes,
and the tolerance per gradient tensor is the project's rule, gnn_model.bound: 4 * e32 + 4 * 2^-23 * max |truth|.
The float64 h0 is pinned to gnn_backward_model.run's by tests/test_gnn_embed_backward_capi.py."""
import numpy as np
import torch
import torch.nn.functional as Fn

import gnn_model as gm
from lsm import gnn

NEAR = 2.0 ** -17      # admission: how close to ReLU's kink a float64 pre-activation may lie


def embed_names(cfg):
    """The state-dict names (without prefix) of EmbedConv's parameters, in the blob's order (the LayerNorm's
    only with layer norm)."""
    return [n for n, _ in gnn.weight_entries(cfg)
            if n.startswith("embed_layer.") and (cfg.layer_norm or ".layer_norm." not in n)]


class Result:
    """One dtype's run: h0 [B, E, Hd], pre [embed_layer_N + 1][edges, Hd] (every pre-activation z_k), grads
    {name without prefix: array}."""


def run(cfg, sd, node_obs, adj, dh0, dtype=torch.float64):
    npdt = np.float64 if dtype == torch.float64 else np.float32
    p = {k: torch.from_numpy(v) for k, v in gm._params(cfg, sd, npdt).items()}
    names = embed_names(cfg)
    for nm in names:
        p[nm] = p[nm].clone().requires_grad_(True)
    B, E, F = node_obs.shape
    Hd = cfg.embed_hidden
    act_e = torch.relu if cfg.embed_relu else torch.tanh
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

    pre = []
    m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
    z = Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])
    pre.append(z.detach().numpy())
    m = ln(act_e(z))
    for k in range(cfg.embed_layer_N):
        z = Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)], p["embed_layer.layers.%d.bias" % (3 * k)])
        pre.append(z.detach().numpy())
        m = ln(act_e(z))
    h0 = torch.zeros(B * E, Hd, dtype=dtype).index_add(0, dst, m)
    res = Result()
    if h0.requires_grad:
        seed = torch.from_numpy(np.ascontiguousarray(dh0, dtype=np.float32)).reshape(B * E, Hd).to(dtype)
        torch.autograd.backward([h0], [seed])
    res.h0, res.pre = h0.detach().view(B, E, Hd).numpy(), pre
    res.grads = {nm: (p[nm].grad if p[nm].grad is not None else torch.zeros_like(p[nm])).numpy() for nm in names}
    return res


def admissible(cfg, r64, r32):
    """None when the two models admit the case, else the reason. Under embed_relu: no embed pre-activation z_k
    within 2^-17 of 0 in float64, and the float32 model on the same side everywhere. Under tanh: every case."""
    if cfg.embed_relu:
        for a, b in zip(r64.pre, r32.pre):
            if (np.abs(a) < NEAR).any():
                return "a pre-activation within 2^-17 of 0"
            if ((a > 0) != (b > 0)).any():
                return "the float32 model is on the other side of 0"
    return None


class Truth:
    """Both models of one case: want(name) -> (truth64, tol, e32) per gradient tensor; names() lists them."""

    def __init__(self, cfg, sd, node_obs, adj, dh0):
        self.cfg = cfg
        with np.errstate(all="ignore"):
            self.r64 = run(cfg, sd, node_obs, adj, dh0, torch.float64)
            self.r32 = run(cfg, sd, node_obs, adj, dh0, torch.float32)
        self.why_not = admissible(cfg, self.r64, self.r32)

    def names(self):
        return embed_names(self.cfg)

    def want(self, name):
        a, b = self.r64.grads[name], self.r32.grads[name]
        e32 = float(np.abs(b.astype(np.float64) - a).max()) if a.size else 0.0
        return a, gm.bound(a, e32) if a.size else 0.0, e32
