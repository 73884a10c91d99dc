"""Independent statements of the actor / critic heads (include/lsm_policy.h restates the formulas) for the
policy-head tests, plus seeded weights and inputs. Nothing here comes from the code under test.

model64        numpy float64, written out from the formulas; also returns the masked logits, every action's
               log-probability, the normalised CDF and the top-two logit gap
TorchHead      the same network built from torch.nn modules (nn.Linear, nn.LayerNorm, nn.GRU, log_softmax) on
               the CPU: .float() is the float32 model, .double() pins model64 (tests/test_policy_capi.py)
bound          the project's tolerance (tests/gnn_model.py), per output tensor: 4 * e32 + 4 * 2^-23 * s with
               e32 = max |model32 - model64| and s = max |model64|

A state dict maps the reference's parameter names (GR_Actor / GR_Critic) to float32 arrays."""
import numpy as np

from gnn_model import bound   # the project's criterion, one definition
from lsm import policy

FLT_MIN = float(np.finfo(np.float32).min)   # -FLT_MAX, torch.finfo(float32).min


def random_head_weights(cfg, seed=0):
    """Seeded state dict at ordinary scale: weights ~ N(0, 1 / fan_in) -- the action layer too, not the
    reference's 0.01 gain, which makes every distribution uniform --, nonzero biases, non-unit LayerNorm
    gamma, nonzero beta. Also the entries forward() does not use (base.mlp.fc_h.*), which packing ignores."""
    rng = np.random.default_rng(4000 + seed)
    sd = {}
    for name, shape in policy.head_weight_entries(cfg):
        if name.startswith("base.feature_norm.") and not cfg.feature_norm:
            continue
        norm = ".norm." in name or "feature_norm" in name or name.endswith((".2.weight", ".2.bias"))
        if norm:
            a = 1.0 + 0.3 * rng.normal(size=shape) if name.endswith("weight") else 0.2 * rng.normal(size=shape)
        elif len(shape) == 1:
            a = 0.3 * rng.normal(size=shape)
        else:
            a = rng.normal(size=shape) / np.sqrt(shape[1])
        sd[name] = a.astype(np.float32)
    Hd = cfg.hidden
    sd["base.mlp.fc_h.0.weight"] = rng.normal(size=(Hd, Hd)).astype(np.float32)
    sd["base.mlp.fc_h.0.bias"] = rng.normal(size=(Hd,)).astype(np.float32)
    sd["base.mlp.fc_h.2.weight"] = rng.normal(size=(Hd,)).astype(np.float32)
    sd["base.mlp.fc_h.2.bias"] = rng.normal(size=(Hd,)).astype(np.float32)
    return sd


def random_inputs(cfg, M, seed=0, mask_zeros=False, avail=None):
    """Seeded inputs: x0, x1 ~ N(0, 1), states ~ N(0, 0.5), masks all ones or with a third of zeros and
    large finite garbage in the states under them (a product with 0 gives 0; it must not leak), u uniform
    in [0, 1), available_actions by `avail`: None, or 'some' (a third of the actions masked per row; row 1
    with a single available action; row 2 with none)."""
    rng = np.random.default_rng(9000 + 131 * seed + M)
    inp = {"x0": rng.normal(size=(M, cfg.in0)).astype(np.float32) if cfg.in0 else None,
           "x1": rng.normal(size=(M, cfg.in1)).astype(np.float32),
           "states": None, "masks": None, "u": None, "avail": None}
    if cfg.recurrent_N:
        st = (0.5 * rng.normal(size=(M, cfg.recurrent_N, cfg.hidden))).astype(np.float32)
        mk = np.ones((M, 1), np.float32)
        if mask_zeros:
            zero = rng.random(M) < 0.34
            zero[0] = True
            mk[zero] = 0
            st[zero] = np.where(rng.random(st[zero].shape) < 0.5, np.float32(1e30), np.float32(-7.5e20))
        inp["states"], inp["masks"] = st, mk
    if cfg.kind == "actor":
        inp["u"] = rng.random(M).astype(np.float32)
        assert (inp["u"] < 1).all()
        if avail == "some":
            A = cfg.num_actions
            av = (rng.random((M, A)) >= 0.34).astype(np.float32)
            av[np.arange(M), rng.integers(0, A, M)] = 1       # at least one per row
            if M > 1:
                av[1] = 0
                av[1, A // 2] = 1
            if M > 2:
                av[2] = 0
            inp["avail"] = av
    return inp


def _ln(v, g, b):
    mu = v.mean(axis=-1, keepdims=True)
    var = ((v - mu) ** 2).mean(axis=-1, keepdims=True)
    return (v - mu) / np.sqrt(var + 1e-5) * g + b


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def model64(cfg, sd, inp):
    """{features, rnn_out, values | logits, logp [M, A], cdf [M, A], gap [M]} in float64."""
    p = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    Hd = cfg.hidden
    parts = [np.asarray(inp[k], dtype=np.float64) for k in ("x0", "x1") if inp[k] is not None]
    x = np.concatenate(parts, axis=1)
    M = x.shape[0]
    act = (lambda v: np.maximum(v, 0)) if cfg.relu else np.tanh
    if cfg.feature_norm:
        x = _ln(x, p["base.feature_norm.weight"], p["base.feature_norm.bias"])
    y = _ln(act(x @ p["base.mlp.fc1.0.weight"].T + p["base.mlp.fc1.0.bias"]), p["base.mlp.fc1.2.weight"],
            p["base.mlp.fc1.2.bias"])
    for i in range(cfg.layer_N):
        y = _ln(act(y @ p["base.mlp.fc2.%d.0.weight" % i].T + p["base.mlp.fc2.%d.0.bias" % i]),
                p["base.mlp.fc2.%d.2.weight" % i], p["base.mlp.fc2.%d.2.bias" % i])
    out = {}
    if cfg.recurrent_N:
        h_all = np.asarray(inp["states"], dtype=np.float64) * np.asarray(inp["masks"], dtype=np.float64).reshape(M, 1, 1)
        rnn_out = np.zeros((M, cfg.recurrent_N, Hd))
        xl = y
        for l in range(cfg.recurrent_N):
            h = h_all[:, l]
            gi = xl @ p["rnn.rnn.weight_ih_l%d" % l].T + p["rnn.rnn.bias_ih_l%d" % l]
            gh = h @ p["rnn.rnn.weight_hh_l%d" % l].T + p["rnn.rnn.bias_hh_l%d" % l]
            r = _sig(gi[:, :Hd] + gh[:, :Hd])
            z = _sig(gi[:, Hd:2 * Hd] + gh[:, Hd:2 * Hd])
            g = np.tanh(gi[:, 2 * Hd:] + r * gh[:, 2 * Hd:])
            xl = (1 - z) * g + z * h
            rnn_out[:, l] = xl
        out["rnn_out"] = rnn_out
        y = _ln(xl, p["rnn.norm.weight"], p["rnn.norm.bias"])
    out["features"] = y
    if cfg.kind == "critic":
        out["values"] = (y @ p["v_out.weight"].T + p["v_out.bias"]).reshape(M)
        return out
    lg = y @ p["act.action_out.linear.weight"].T + p["act.action_out.linear.bias"]
    if inp.get("avail") is not None:
        lg = np.where(np.asarray(inp["avail"]) == 0, FLT_MIN, lg)
    mx = lg.max(axis=1, keepdims=True)
    e = np.exp(lg - mx)
    s = e.sum(axis=1, keepdims=True)
    out["logits"] = lg
    out["logp"] = (lg - mx) - np.log(s)
    out["cdf"] = np.cumsum(e, axis=1) / s
    srt = np.sort(lg, axis=1)
    out["gap"] = srt[:, -1] - srt[:, -2] if lg.shape[1] > 1 else np.full(M, np.inf)
    return out


def clamp_u(u):
    """The header's treatment of a bad uniform: NaN and negatives 0, >= 1 the largest float below 1."""
    u = np.asarray(u, dtype=np.float32).copy()
    with np.errstate(invalid="ignore"):
        hi = u >= 1
        bad = ~((u >= 0) & (u < 1))
    u[bad & ~hi] = 0
    u[hi] = np.float32(0.99999994)
    return u, bad


def sample64(cdf, u):
    """The inverse CDF: per row the first a with cdf[a] > u; without one, the last a with p_a > 0."""
    cdf = np.asarray(cdf)
    u = np.asarray(u, dtype=np.float64).reshape(-1, 1)
    over = cdf > u
    first = over.argmax(axis=1)
    p = np.diff(np.concatenate([np.zeros((cdf.shape[0], 1)), cdf], axis=1), axis=1)
    last = cdf.shape[1] - 1 - (p[:, ::-1] > 0).argmax(axis=1)
    return np.where(over.any(axis=1), first, last)


def mode64(logits):
    return np.asarray(logits).argmax(axis=1)    # the first a attaining the maximum


class TorchHead:
    """The head from torch.nn modules on the CPU, in `dtype` (torch.float32: the float32 model;
    torch.float64: the pin of model64)."""

    def __init__(self, cfg, sd, dtype):
        import torch
        from torch import nn
        self.cfg, self.dtype = cfg, dtype
        n, Hd = cfg.in0 + cfg.in1, cfg.hidden
        act = nn.ReLU if cfg.relu else nn.Tanh
        self.fn = nn.LayerNorm(n) if cfg.feature_norm else None
        self.fc = [nn.Sequential(nn.Linear(n if k == 0 else Hd, Hd), act(), nn.LayerNorm(Hd)) for k in range(cfg.layer_N + 1)]
        self.gru = nn.GRU(Hd, Hd, num_layers=cfg.recurrent_N) if cfg.recurrent_N else None
        self.norm = nn.LayerNorm(Hd) if cfg.recurrent_N else None
        self.out = nn.Linear(Hd, cfg.out_rows)

        def put(mod, attr, key):
            with torch.no_grad():
                getattr(mod, attr).copy_(torch.from_numpy(np.asarray(sd[key])))

        if self.fn is not None:
            put(self.fn, "weight", "base.feature_norm.weight")
            put(self.fn, "bias", "base.feature_norm.bias")
        for k, seq in enumerate(self.fc):
            pre = "base.mlp.fc1" if k == 0 else "base.mlp.fc2.%d" % (k - 1)
            for idx in (0, 2):
                put(seq[idx], "weight", "%s.%d.weight" % (pre, idx))
                put(seq[idx], "bias", "%s.%d.bias" % (pre, idx))
        if self.gru is not None:
            for l in range(cfg.recurrent_N):
                for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                    put(self.gru, "%s_l%d" % (nm, l), "rnn.rnn.%s_l%d" % (nm, l))
            put(self.norm, "weight", "rnn.norm.weight")
            put(self.norm, "bias", "rnn.norm.bias")
        last = "act.action_out.linear" if cfg.kind == "actor" else "v_out"
        put(self.out, "weight", last + ".weight")
        put(self.out, "bias", last + ".bias")
        for mod in [self.fn, self.gru, self.norm, self.out] + self.fc:
            if mod is not None:
                mod.to(dtype)

    def __call__(self, inp):
        import torch
        cfg = self.cfg
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dtype)
        with torch.no_grad():
            x = torch.cat([t(inp[k]) for k in ("x0", "x1") if inp[k] is not None], dim=1)
            M = x.shape[0]
            if self.fn is not None:
                x = self.fn(x)
            for seq in self.fc:
                x = seq(x)
            out = {}
            if self.gru is not None:
                h = (t(inp["states"]) * t(inp["masks"]).view(M, 1, 1)).transpose(0, 1).contiguous()
                y, hn = self.gru(x.unsqueeze(0), h)
                out["rnn_out"] = hn.transpose(0, 1).contiguous().numpy()
                x = self.norm(y.squeeze(0))
            out["features"] = x.numpy()
            o = self.out(x)
            if cfg.kind == "critic":
                out["values"] = o.reshape(M).numpy()
                return out
            if inp.get("avail") is not None:
                o = torch.where(t(inp["avail"]) == 0, torch.full_like(o, FLT_MIN), o)
            out["logits"] = o.numpy()
            out["logp"] = torch.log_softmax(o, dim=1).numpy()
        return out


def model32(cfg, sd, inp):
    import torch
    return TorchHead(cfg, sd, torch.float32)(inp)


def model64_torch(cfg, sd, inp):
    import torch
    return TorchHead(cfg, sd, torch.float64)(inp)


def finite_logits(a):
    """A mask of the logits that are not the availability mask's -FLT_MAX."""
    return np.asarray(a) > FLT_MIN / 2


def tensor_bound(w64, w32, sel=None):
    """(tolerance, e32) of one output tensor over `sel` (a boolean mask; all by default)."""
    w64 = np.asarray(w64, dtype=np.float64)
    d = np.abs(np.asarray(w32, dtype=np.float64) - w64)
    if sel is not None:
        d, w64 = d[sel], w64[sel]
    if d.size == 0:
        return 0.0, 0.0
    e32 = float(d.max())
    return bound(w64, e32), e32


RATIOS = []   # (what, max |out - model64| / e32, the same / tolerance) of every comparison made in this session


def assert_close(out, w64, tol, e32, what, sel=None):
    """max |out - model64| <= tol over `sel`; prints the figures first."""
    out = np.asarray(out, dtype=np.float64)
    w64 = np.asarray(w64, dtype=np.float64)
    if sel is not None:
        out, w64 = out[sel], w64[sel]
    err = float(np.abs(out - w64).max()) if out.size else 0.0
    r32 = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    rtol = err / tol if tol > 0 else float("inf") if err > 0 else 0.0
    RATIOS.append((what, r32, rtol))
    print("head %s: err %.3e  e32 %.3e  tol %.3e  err/e32 %.2f  err/tol %.2f" % (what, err, e32, tol, r32, rtol))
    assert np.isfinite(out).all(), what
    assert err <= tol, (what, err, tol, e32)
