"""The yardstick of the heads' backward pass (include/lsm_backward.h): tests/policy_model.py's TorchHead
modules with grad enabled, run as evaluate_model.TorchEval runs them (one nn.GRU step per call, h * mask
first), and torch.autograd.backward([out], [seed]). In float64 it is the truth, in float32 it gives e32. Nothing
here comes from the code under test.

A seed is the gradient at the head's output: dlogits [T*C, A] (actor; entries under available_actions == 0
are cut by the masking assignment, whatever they hold) or dvalues [T*C] (critic)."""
import numpy as np

import policy_model as pm
from lsm import policy

FLT_MIN = pm.FLT_MIN


def parameters(mods, cfg):
    """{state-dict name: the module's parameter}, the names of lsm.policy.head_weight_entries."""
    out = {}
    if mods.fn is not None:
        out["base.feature_norm.weight"], out["base.feature_norm.bias"] = mods.fn.weight, mods.fn.bias
    for k, seq in enumerate(mods.fc):
        pre = "base.mlp.fc1" if k == 0 else "base.mlp.fc2.%d" % (k - 1)
        for idx in (0, 2):
            out["%s.%d.weight" % (pre, idx)], out["%s.%d.bias" % (pre, idx)] = seq[idx].weight, seq[idx].bias
    if mods.gru is not None:
        for l in range(cfg.recurrent_N):
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                out["rnn.rnn.%s_l%d" % (nm, l)] = getattr(mods.gru, "%s_l%d" % (nm, l))
        out["rnn.norm.weight"], out["rnn.norm.bias"] = mods.norm.weight, mods.norm.bias
    last = "act.action_out.linear" if cfg.kind == "actor" else "v_out"
    out[last + ".weight"], out[last + ".bias"] = mods.out.weight, mods.out.bias
    names = [n for n, _ in policy.head_weight_entries(cfg) if cfg.feature_norm or "feature_norm" not in n]
    assert sorted(out) == sorted(names)
    return out


class TorchBackward:
    """The head from torch.nn modules on the CPU in `dtype`, differentiated by autograd."""

    def __init__(self, cfg, sd, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.mods = pm.TorchHead(cfg, sd, dtype)
        self.params = parameters(self.mods, cfg)

    def forward(self, inp, C, T):
        """(out, x0, x1, pre): the masked logits [T*C, A] or the values [T*C, 1] with their graph, the two
        input leaves, and every activation's pre-activation (detached)."""
        import torch
        cfg, m = self.cfg, self.mods
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dtype)
        x0 = t(inp["x0"]).requires_grad_(True) if inp.get("x0") is not None else None
        x1 = t(inp["x1"]).requires_grad_(True)
        x = torch.cat([v for v in (x0, x1) if v is not None], dim=1)
        pre = []
        if m.fn is not None:
            x = m.fn(x)
        for seq in m.fc:
            a = seq[0](x)
            pre.append(a.detach().numpy().copy())
            x = seq[2](seq[1](a))
        if m.gru is not None:
            h = t(inp["states"]).transpose(0, 1).contiguous()        # [RN, C, Hd]
            mk = t(inp["masks"]).view(T, C)
            tops = []
            for l in range(T):
                h = h * mk[l].view(1, C, 1)
                y, h = m.gru(x[l * C:(l + 1) * C].unsqueeze(0), h)
                tops.append(y.squeeze(0))
            x = m.norm(torch.cat(tops, dim=0))
        if cfg.kind == "actor":
            x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
        o = m.out(x)
        if cfg.kind == "actor" and inp.get("avail") is not None:
            o = torch.where(t(inp["avail"]) == 0, torch.full_like(o, FLT_MIN), o)
        return o, x0, x1, pre

    def __call__(self, inp, seed, C, T):
        """{name: the parameter's gradient, 'dx0', 'dx1', 'out', 'pre'} as float64 / float32 arrays."""
        import torch
        for p in self.params.values():
            p.grad = None
        o, x0, x1, pre = self.forward(inp, C, T)
        s = torch.from_numpy(np.ascontiguousarray(seed)).to(self.dtype).reshape(o.shape)
        torch.autograd.backward([o], [s])
        out = {k: p.grad.detach().numpy().copy() for k, p in self.params.items()}
        if x1.shape[1]:                      # in1 == 0: x1 is null and there is no dx1, as with x0
            out["dx1"] = x1.grad.numpy().copy()
        if x0 is not None:
            out["dx0"] = x0.grad.numpy().copy()
        out["out"], out["pre"] = o.detach().numpy().copy(), pre
        return out


def model64(cfg, sd, inp, seed, C, T):
    import torch
    return TorchBackward(cfg, sd, torch.float64)(inp, seed, C, T)


def model32(cfg, sd, inp, seed, C, T):
    import torch
    return TorchBackward(cfg, sd, torch.float32)(inp, seed, C, T)


def dlogits_of(logits, actions, c, kappa, avail=None, active=None):
    """The gradient at the (masked) logits of J = sum_m c_m * log_probs_m + kappa * dist_entropy, float64:
    tests/loss_model.py's closed forms with dlogp = c and dent = kappa * active / sum(active) (1 / M without
    active masks)."""
    lg = np.asarray(logits, dtype=np.float64)
    M, A = lg.shape
    act = np.asarray(actions).astype(np.int64).reshape(M)
    mx = lg.max(axis=1, keepdims=True)
    d = lg - mx
    e = np.exp(d)
    s = e.sum(axis=1, keepdims=True)
    lp = d - np.log(s)
    p = e / s
    H = -(np.where(e > 0, p * lp, 0.0)).sum(axis=1)
    w = np.ones(M) if active is None else np.asarray(active, dtype=np.float64).reshape(M)
    dent = kappa * w / w.sum()
    hot = np.zeros((M, A))
    hot[np.arange(M), act] = 1.0
    c = np.asarray(c, dtype=np.float64).reshape(M)
    dl = c[:, None] * (hot - p) + dent[:, None] * -(p * (lp + H[:, None]))
    dl = np.where(e > 0, dl, c[:, None] * hot)
    if avail is not None:
        dl = np.where(np.asarray(avail) == 0, 0.0, dl)
    return dl
