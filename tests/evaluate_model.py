"""Independent statements of the heads' sequence form (include/lsm_evaluate.h restates the formulas) for the
evaluate tests, plus seeded inputs. Nothing here comes from the code under test.

model64   numpy float64, written out from the formulas: the GRU state carried through each chunk's steps
          with the per-step mask product, every action's log-probability, the entropy, dist_entropy
model32   the same network from torch.nn modules in float32 on the CPU (tests/policy_model.py's TorchHead
          holds them): nn.GRU over the sequence, one step per call, with the per-step product, and
          torch.distributions.Categorical; TorchEval(.., torch.float64) pins model64

A minibatch is time-major: row l * C + b is step l of chunk b. Inputs: x0 [T*C, in0] or None, x1 [T*C, in1],
states [C, recurrent_N, hidden], masks [T*C, 1], actions [T*C] float32, avail [T*C, A] or None, active
[T*C, 1] or None."""
import numpy as np

import policy_model as pm

FLT_MIN = pm.FLT_MIN


def random_inputs(cfg, C, T, seed=0, mask_zeros=False, avail=None, active=None):
    """Seeded inputs. mask_zeros: a third of the masks zero, among them chunk 0's at l = 0 and (T > 1) chunk
    0's at the last step while its tile neighbours' are 1 there, with large finite garbage in the initial
    states under the zero l = 0 masks. avail 'some': a third of the actions masked per row, row 1 with a
    single available action, row 2 with none, row 3 storing an unavailable action; every other stored action
    is drawn among the row's available ones. active: None, 'some' (a fifth zero) or 'zero' (all zero)."""
    rng = np.random.default_rng(7000 + 977 * seed + 31 * C + T)
    R = C * T
    inp = {"x0": rng.normal(size=(R, cfg.in0)).astype(np.float32) if cfg.in0 else None,
           "x1": rng.normal(size=(R, cfg.in1)).astype(np.float32),
           "states": None, "masks": None, "actions": None, "avail": None, "active": None}
    if cfg.recurrent_N:
        st = (0.5 * rng.normal(size=(C, cfg.recurrent_N, cfg.hidden))).astype(np.float32)
        mk = np.ones((T, C), np.float32)
        if mask_zeros:
            mk[rng.random((T, C)) < 0.34] = 0
            mk[0, 0] = 0
            if C > 1:
                mk[0, 1] = 1
            if T > 1:
                mk[T - 1, 0] = 0
                mk[T - 1, 1:3] = 1
            z0 = mk[0] == 0
            st[z0] = np.where(rng.random(st[z0].shape) < 0.5, np.float32(1e30), np.float32(-7.5e20))
        inp["states"], inp["masks"] = st, mk.reshape(R, 1)
    if cfg.kind == "actor":
        A = cfg.num_actions
        av = np.ones((R, A), np.float32)
        if avail == "some":
            assert R >= 4 and A >= 2
            av = (rng.random((R, A)) >= 0.34).astype(np.float32)
            av[np.arange(R), rng.integers(0, A, R)] = 1       # at least one per row
            av[1] = 0
            av[1, A // 2] = 1
            av[2] = 0
        # the stored action: drawn among the row's available ones (any, where the row has none)
        pick = rng.random((R, A)) * np.where(av.sum(axis=1, keepdims=True) > 0, av, 1.0)
        act = pick.argmax(axis=1)
        if avail == "some":
            av[3] = 1
            av[3, act[3]] = 0                                 # row 3 stores an unavailable action
            inp["avail"] = av
        inp["actions"] = act.astype(np.float32)
        if active == "some":
            am = (rng.random((R, 1)) >= 0.2).astype(np.float32)
            am[0], am[R - 1] = 0, 1
            inp["active"] = am
        elif active == "zero":
            inp["active"] = np.zeros((R, 1), np.float32)
    return inp


def clamp_actions(a, A):
    """The header's treatment of a stored action: NaN 0, otherwise into [0, A - 1] and truncated; and which
    entries that changed."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore"):
        bad = ~((a >= 0) & (a < A) & (a == np.floor(a)))
        c = np.trunc(np.clip(np.where(np.isnan(a), 0.0, a), 0, A - 1)).astype(np.int64)
    return c, bad


def model64(cfg, sd, inp, C, T):
    """{features, rnn_out, values | logits, logp [T*C, A], log_probs, entropy, dist_entropy} in float64, and amp
    [T*C]: the product of the row's LayerNorm gains above 1 (how ill-conditioned the row is)."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    Hd, R = cfg.hidden, C * T
    x = np.concatenate([np.asarray(inp[k], dtype=np.float64) for k in ("x0", "x1") if inp[k] is not None], axis=1)
    assert x.shape[0] == R
    act = (lambda v: np.maximum(v, 0)) if cfg.relu else np.tanh
    amp = np.ones(R)

    def ln(v, g, b):
        """pm._ln, noting by how much the row's LayerNorm scales an error of its input: 1 / sqrt(var + eps),
        counted when above 1 (a row of equal values, var == 0, gives beta exactly in any precision)."""
        var = ((v - v.mean(axis=-1, keepdims=True)) ** 2).mean(axis=-1)
        with np.errstate(invalid="ignore"):
            gain = np.where(var > 0, 1.0 / np.sqrt(var + 1e-5), 1.0)
        amp[...] = amp * np.where(gain > 1, gain, 1.0)
        return pm._ln(v, g, b)

    with np.errstate(invalid="ignore"):
        if cfg.feature_norm:
            x = ln(x, p["base.feature_norm.weight"], p["base.feature_norm.bias"])
        y = ln(act(x @ p["base.mlp.fc1.0.weight"].T + p["base.mlp.fc1.0.bias"]), p["base.mlp.fc1.2.weight"],
               p["base.mlp.fc1.2.bias"])
        for i in range(cfg.layer_N):
            y = ln(act(y @ p["base.mlp.fc2.%d.0.weight" % i].T + p["base.mlp.fc2.%d.0.bias" % i]),
                   p["base.mlp.fc2.%d.2.weight" % i], p["base.mlp.fc2.%d.2.bias" % i])
    out = {"amp": amp}
    if cfg.recurrent_N:
        h = np.asarray(inp["states"], dtype=np.float64).copy()           # [C, RN, Hd], carried over the steps
        mk = np.asarray(inp["masks"], dtype=np.float64).reshape(T, C)
        top = np.zeros((R, Hd))
        for l in range(T):
            h = h * mk[l][:, None, None]
            xl = y[l * C:(l + 1) * C]
            for k in range(cfg.recurrent_N):
                gi = xl @ p["rnn.rnn.weight_ih_l%d" % k].T + p["rnn.rnn.bias_ih_l%d" % k]
                gh = h[:, k] @ p["rnn.rnn.weight_hh_l%d" % k].T + p["rnn.rnn.bias_hh_l%d" % k]
                r = pm._sig(gi[:, :Hd] + gh[:, :Hd])
                z = pm._sig(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
                g = np.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
                xl = (1 - z) * g + z * h[:, k]
                h[:, k] = xl
            top[l * C:(l + 1) * C] = xl
        out["rnn_out"] = h
        y = ln(top, p["rnn.norm.weight"], p["rnn.norm.bias"])
    if cfg.kind == "critic":
        out["features"] = y
        out["values"] = (y @ p["v_out.weight"].T + p["v_out.bias"]).reshape(R)
        return out
    y = np.where(np.isnan(y), 0.0, y)
    out["features"] = y
    lg = y @ p["act.action_out.linear.weight"].T + p["act.action_out.linear.bias"]
    if inp.get("avail") is not None:
        lg = np.where(np.asarray(inp["avail"]) == 0, FLT_MIN, lg)
    mx = lg.max(axis=1, keepdims=True)
    e = np.exp(lg - mx)
    s = e.sum(axis=1, keepdims=True)
    logp = (lg - mx) - np.log(s)
    out["logits"], out["logp"] = lg, logp
    a, _ = clamp_actions(inp["actions"], cfg.num_actions)
    out["log_probs"] = logp[np.arange(R), a]
    out["entropy"] = -np.where(e > 0, (e / s) * logp, 0.0).sum(axis=1)
    out["dist_entropy"] = dist_entropy(out["entropy"], inp.get("active"))
    return out


def dist_entropy(entropy, active):
    entropy = np.asarray(entropy, dtype=np.float64)
    if active is None:
        return float(entropy.mean())
    w = np.asarray(active, dtype=np.float64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64((entropy * w).sum()) / np.float64(w.sum()))


class TorchEval:
    """The sequence form from torch.nn modules on the CPU, in `dtype`: nn.GRU fed one step at a time with
    h * masks[l] before each, Categorical(logits=...).log_prob / .entropy()."""

    def __init__(self, cfg, sd, dtype):
        self.cfg, self.dtype = cfg, dtype
        self.mods = pm.TorchHead(cfg, sd, dtype)      # the modules, loaded from the state dict

    def __call__(self, inp, C, T):
        import torch
        cfg, m = self.cfg, self.mods
        R = C * T
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dtype)
        with torch.no_grad():
            x = torch.cat([t(inp[k]) for k in ("x0", "x1") if inp[k] is not None], dim=1)
            if m.fn is not None:
                x = m.fn(x)
            for seq in m.fc:
                x = seq(x)
            out = {}
            if m.gru is not None:
                h = t(inp["states"]).transpose(0, 1).contiguous()        # [RN, C, Hd]
                mk = t(inp["masks"]).view(T, C)
                tops = []
                for l in range(T):
                    h = h * mk[l].view(1, C, 1)
                    y, h = m.gru(x[l * C:(l + 1) * C].unsqueeze(0), h)
                    tops.append(y.squeeze(0))
                out["rnn_out"] = h.transpose(0, 1).contiguous().numpy()
                x = m.norm(torch.cat(tops, dim=0))
            if cfg.kind == "critic":
                out["features"] = x.numpy()
                out["values"] = m.out(x).reshape(R).numpy()
                return out
            x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
            out["features"] = x.numpy()
            o = m.out(x)
            if inp.get("avail") is not None:
                o = torch.where(t(inp["avail"]) == 0, torch.full_like(o, FLT_MIN), o)
            out["logits"] = o.numpy()
            dist = torch.distributions.Categorical(logits=o)
            a, _ = clamp_actions(inp["actions"], cfg.num_actions)
            out["log_probs"] = dist.log_prob(torch.from_numpy(a)).numpy()
            out["entropy"] = dist.entropy().numpy()
        return out


def model32(cfg, sd, inp, C, T):
    import torch
    return TorchEval(cfg, sd, torch.float32)(inp, C, T)


def model64_torch(cfg, sd, inp, C, T):
    import torch
    return TorchEval(cfg, sd, torch.float64)(inp, C, T)
