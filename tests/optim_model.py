"""Three restatements of include/lsm_optim.h for the tests: `model32`, numpy float32 that follows the header
operation for operation (the yardstick for bit equality; numpy neither fuses nor reorders), `truth64`, the same
formulas in float64 with a plain float64 norm, and `torch32`, torch.optim.Adam + clip_grad_norm_ on CPU float32
tensors (the float32 yardstick of the project's criterion, 4 * e32 + 4 * 2^-23 * max|truth|)."""
import dataclasses
import math

import numpy as np

CHUNK, LANES = 1024, 256
F32 = np.float32


@dataclasses.dataclass(frozen=True)
class Hyper:
    lr: float = 7e-4
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-5
    weight_decay: float = 0.0
    max_grad_norm: float = 10.0
    use_max_grad_norm: bool = True
    skip_nonfinite: bool = True


def fresh_state():
    return np.array([0.0, 1.0, 1.0, 0.0], np.float64)


def chunk_partial(g):
    """The header's in-workgroup order for one chunk of float32 gradients (len <= CHUNK)."""
    sq = np.zeros(CHUNK, np.float64)
    d = g.astype(np.float64)
    sq[:g.size] = d * d          # an absent element adds +0: no change to a sum that starts at +0
    rows = sq.reshape(CHUNK // LANES, LANES)
    q = np.zeros(LANES, np.float64)
    for r in rows:               # lane j: elements j, j + 256, ... ascending
        q = q + r
    s = LANES // 2
    while s:
        q[:s] = q[:s] + q[s:2 * s]
        s //= 2
    return q[0]


def norm_sum(grads):
    total = np.float64(0.0)
    for g in grads:
        for k in range(0, g.size, CHUNK):
            total = total + chunk_partial(g[k:k + CHUNK])
    return total


def model32(h, segs, state):
    """One call on one group. segs: [(w, g, m, v)] float32 arrays; state: float64[4]. Returns (new segs, new
    state, info float32[4]); nothing is modified in place."""
    with np.errstate(all="ignore"):
        norm = F32(np.sqrt(norm_sum([s[1] for s in segs])))
        coef = F32(1.0)
        if h.use_max_grad_norm:
            c = F32(h.max_grad_norm) / (norm + F32(1e-6))
            coef = F32(1.0) if c > F32(1.0) else c
        skipped = bool(h.skip_nonfinite and not np.isfinite(norm))
        info = np.array([norm, coef, 1.0 if skipped else 0.0, 0.0], F32)
        if skipped:
            return [tuple(a.copy() for a in s) for s in segs], state.copy(), info
        st = state.copy()
        st[0] = state[0] + 1.0
        st[1] = state[1] * np.float64(h.beta1)
        st[2] = state[2] * np.float64(h.beta2)
        step_size = F32(np.float64(h.lr) / (np.float64(1.0) - st[1]))
        s2 = F32(np.sqrt(np.float64(1.0) - st[2]))
        omb1, omb2 = F32(1.0 - h.beta1), F32(1.0 - h.beta2)
        b2f, epsf, wdf = F32(h.beta2), F32(h.eps), F32(h.weight_decay)
        out = []
        for w, grad, m, v in segs:
            g = coef * grad
            if wdf != 0:
                g = g + wdf * w
            m = m + omb1 * (g - m)
            v = v * b2f + (omb2 * g) * g
            w = w - step_size * (m / (np.sqrt(v) / s2 + epsf))
            assert w.dtype == m.dtype == v.dtype == F32
            out.append((w, grad.copy(), m, v))
        return out, st, info


def truth64(h, segs, steps):
    """The same step in float64 on float64 arrays [(w, g, m, v)], `steps` the executed steps before it. Returns
    (new segs, grad_norm)."""
    norm = math.sqrt(sum(float(np.sum(s[1].astype(np.float64) ** 2)) for s in segs))
    coef = min(h.max_grad_norm / (norm + 1e-6), 1.0) if h.use_max_grad_norm else 1.0
    t = steps + 1
    step_size = h.lr / (1.0 - h.beta1 ** t)
    s2 = math.sqrt(1.0 - h.beta2 ** t)
    out = []
    for w, grad, m, v in segs:
        g = coef * grad
        if h.weight_decay != 0:
            g = g + h.weight_decay * w
        m = m + (1.0 - h.beta1) * (g - m)
        v = v * h.beta2 + (1.0 - h.beta2) * g * g
        w = w - step_size * (m / (np.sqrt(v) / s2 + h.eps))
        out.append((w, grad, m, v))
    return out, norm


class Torch32:
    """torch.optim.Adam (single tensor, CPU float32) + clip_grad_norm_ over the segments as parameters."""

    def __init__(self, h, weights):
        import torch
        self.h = h
        self.params = [torch.nn.Parameter(torch.tensor(np.array(w, np.float32))) for w in weights]
        self.opt = torch.optim.Adam(self.params, lr=h.lr, betas=(h.beta1, h.beta2), eps=h.eps,
                                    weight_decay=h.weight_decay, foreach=False)

    def step(self, grads, lr=None, weights=None):
        """One step on these gradients (weights: the parameters are set to them first; the moments stay
        torch's own). Returns ([(w, m, v)] as float32 arrays, the norm torch reports)."""
        import torch
        if lr is not None:
            for pg in self.opt.param_groups:
                pg["lr"] = lr
        if weights is not None:
            for p, w in zip(self.params, weights):
                p.data.copy_(torch.tensor(np.array(w, np.float32)))
        for p, g in zip(self.params, grads):
            p.grad = torch.tensor(np.array(g, np.float32))
        if self.h.use_max_grad_norm:
            norm = torch.nn.utils.clip_grad_norm_(self.params, self.h.max_grad_norm)
        else:
            norm = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in self.params))
        self.opt.step()
        out = [(p.detach().numpy().copy(), self.opt.state[p]["exp_avg"].numpy().copy(),
                self.opt.state[p]["exp_avg_sq"].numpy().copy()) for p in self.params]
        return out, float(norm)


def bound(truth, e32):
    """The project's criterion (bench_common.criterion, gnn_model.bound)."""
    return 4.0 * e32 + 4.0 * 2.0 ** -23 * float(np.abs(truth).max())


def within(out, truth, t32, what):
    """|out - truth| <= 4 * |t32 - truth| + 4 * 2^-23 * max|truth|, the figures printed first."""
    truth = np.asarray(truth, np.float64)
    e32 = float(np.abs(np.asarray(t32, np.float64) - truth).max())
    err = float(np.abs(np.asarray(out, np.float64) - truth).max())
    tol = bound(truth, e32)
    print("optim %s: err %.3e  e32 %.3e  tol %.3e" % (what, err, e32, tol))
    assert np.isfinite(np.asarray(out)).all(), what
    assert err <= tol, (what, err, tol, e32)
    return err, e32, tol


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))
