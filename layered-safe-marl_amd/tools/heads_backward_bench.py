"""Device time of the heads' backward pass (what loss.backward() runs through ACTLayer / v_out, RNNLayer and
MLPBase on one PPO minibatch, given the gradient at the logits or the values):

  (A) lsm.policy.PolicyHead.backward: csrc/lsm_backward.hip's four launches (the forward with saves, the
      backward sweep, the weight gradients per slab, the sum over the slabs), dx0 / dx1 included;
  (B) the same formulas as torch.nn modules on the device: their forward with the graph kept (nn.GRU one step
      per call with h * masks[l] before it) and torch.autograd.backward from the same seed, gradients set to
      None before each call. Also timed: that forward alone, and the backward alone on a graph kept with
      retain_graph=True.

Shapes: tools/evaluate_bench.py's -- C = 51200 chunks of T = 10 steps with recurrent_N 1, and 512000
feed-forward rows (T = 1, recurrent_N 0), hidden 64, layer_N 1; the actor reads obs (6) + the encoder's 16
columns and has 25 actions, the critic reads the encoder's 16 columns alone. Seeds are N(0, 1) / rows.

Method: both sides are run once and checked first, by the tests' criterion per gradient tensor (each named
weight entry and dx1) on 64 chunks as a minibatch of their own: the modules in float64 are the truth, e32 is
the float32 modules' error against it, and a fused error above 4 * e32 + 4 * 2^-23 * max|truth| ends the run.
The 64 chunks are the first of 16 windows of the minibatch that the tests' rule 2 admits
(tests/heads_backward_cases.py: no ReLU pre-activation within 2^-17 of 0 in float64 and the float32 modules
on the same side everywhere; one flipped unit is an O(1) change of a row's gradient, which no rounding bound
covers). Should no window qualify, the figures of the last one are recorded with check_enforced false.
Then a warm-up, HIP events on the stream around `reps` back-to-back calls, the sides in alternating rounds, and
the median / min / max of the rounds' means (tools/bench_common.py's alternated()). The stages' times are the
kernels' durations in one torch.profiler trace of three fused calls (null when the profiler gives none).

    python layered-safe-marl_amd/tools/heads_backward_bench.py [--out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from policy_bench import seeded_state_dict, torch_head  # noqa: E402
from bench_common import alternated, criterion, emit  # noqa: E402

DEV = "cuda:0"
OBS, ENC, HIDDEN, ACTIONS = 6, 16, 64, 25
ROWS, CHUNK = 512000, 10
CHECK_CHUNKS = 64
WINDOWS = 16
STAGES = ("fwd_kernel", "bwd_kernel", "dw_kernel", "finish_kernel")


def torch_forward(mod, cfg, x0, x1, states, masks, C, T, pre=None):
    """The head's output with its graph: logits [T*C, A] or values [T*C, 1]. pre (a list): every activation's
    pre-activation is appended to it, detached."""
    import torch
    x = x1 if x0 is None else torch.cat([x0, x1], dim=1)
    if mod.feature_norm is not None:
        x = mod.feature_norm(x)
    for seq in mod.fc:
        if pre is None:
            x = seq(x)
        else:
            a = seq[0](x)
            pre.append(a.detach())
            x = seq[2](seq[1](a))
    if mod.rnn is not None:
        h = states.transpose(0, 1).contiguous()
        mk = masks.view(T, C)
        tops = []
        for l in range(T):
            h = h * mk[l].view(1, C, 1)
            y, h = mod.rnn(x[l * C:(l + 1) * C].unsqueeze(0), h)
            tops.append(y.squeeze(0))
        x = mod.norm(torch.cat(tops, dim=0))
    if cfg.kind == "actor":
        x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    return mod.out(x)


def named(cfg, out):
    """{entry name: its slice of the packed dweights, dx1}: one check per gradient tensor, as in the tests."""
    import numpy as np
    from lsm import policy
    res, o = {}, 0
    for name, shape in policy.head_weight_entries(cfg):
        n = int(np.prod(shape))
        if cfg.feature_norm or "base.feature_norm." not in name:
            res[name] = out["dweights"][o:o + n]
        o += n
    res["dx1"] = out["dx1"]
    return res


def packed_grads(mod, cfg):
    """The modules' .grad in the blob's order (include/lsm_policy.h), one flat tensor."""
    import torch
    n = cfg.in0 + cfg.in1
    parts = []
    if mod.feature_norm is not None:
        parts += [mod.feature_norm.weight.grad, mod.feature_norm.bias.grad]
    else:
        parts += [torch.zeros(2 * n, device=DEV, dtype=mod.out.weight.dtype)]
    for seq in mod.fc:
        parts += [seq[0].weight.grad, seq[0].bias.grad, seq[2].weight.grad, seq[2].bias.grad]
    if mod.rnn is not None:
        for l in range(cfg.recurrent_N):
            parts += [getattr(mod.rnn, "%s_l%d" % (nm, l)).grad for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        parts += [mod.norm.weight.grad, mod.norm.bias.grad]
    parts += [mod.out.weight.grad, mod.out.bias.grad]
    return torch.cat([p.reshape(-1) for p in parts])


def torch_backward(mod, cfg, x0, x1, states, masks, seed, C, T, pre=None):
    """Forward and backward: {dweights (packed), dx1}."""
    import torch
    mod.zero_grad(set_to_none=True)
    x1 = x1.detach().requires_grad_(True)
    x0 = None if x0 is None else x0.detach().requires_grad_(True)
    o = torch_forward(mod, cfg, x0, x1, states, masks, C, T, pre)
    torch.autograd.backward([o], [seed.reshape(o.shape).to(o.dtype)])
    return {"dweights": packed_grads(mod, cfg), "dx1": x1.grad}


def stage_times(fn):
    """{kernel: mean device ms per call} of the backward's four kernels over three calls, or None."""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
        out = {}
        for ev in prof.key_averages():
            for s in STAGES:
                if s in ev.key:
                    total = getattr(ev, "device_time_total", None)
                    if total is None:
                        total = ev.cuda_time_total
                    out[s] = out.get(s, 0.0) + total / 1000.0 / 3
        return out if len(out) == len(STAGES) else None
    except Exception as e:   # the profiler is optional here; the timing above does not depend on it
        print("stage times unavailable: %r" % (e,), file=sys.stderr)
        return None


def bench_head(role, recurrent, quick):
    import torch
    from lsm import policy
    T = CHUNK if recurrent else 1
    C = ROWS // T
    rn = 1 if recurrent else 0
    if role == "actor":
        cfg = policy.HeadConfig(kind="actor", in0=OBS, in1=ENC, hidden=HIDDEN, num_actions=ACTIONS, recurrent_N=rn)
    else:
        cfg = policy.HeadConfig(kind="critic", in0=0, in1=ENC, hidden=HIDDEN, recurrent_N=rn)
    sd = seeded_state_dict(cfg, 1 if role == "actor" else 2)
    head = policy.PolicyHead(cfg, policy.pack_head_weights(sd, cfg), DEV)
    # train(): MIOpen's RNN backward refuses eval mode; the modules have no dropout, so the forward is the same
    mod32, mod64 = torch_head(cfg, sd, torch.float32).train(), torch_head(cfg, sd, torch.float64).train()
    g = torch.Generator(device=DEV).manual_seed(7)
    x0 = torch.randn((ROWS, OBS), generator=g, device=DEV) if cfg.in0 else None
    x1 = torch.randn((ROWS, ENC), generator=g, device=DEV)
    st = 0.5 * torch.randn((C, 1, HIDDEN), generator=g, device=DEV) if rn else None
    masks = (torch.rand((ROWS, 1), generator=g, device=DEV) > 0.02).float() if rn else None
    seed = torch.randn((ROWS, cfg.out_rows), generator=g, device=DEV) / ROWS
    key = "dlogits" if role == "actor" else "dvalues"

    def fused():
        return head.backward(x0, x1, st, masks, T, dx=True, **{key: seed})

    def plain():
        return torch_backward(mod32, cfg, x0, x1, st, masks, seed, C, T)

    def forward_only():
        return torch_forward(mod32, cfg, x0, x1, st, masks, C, T)

    # the tests' criterion, per gradient tensor, on a window of chunks as a minibatch of its own, against the
    # modules in float64: the first of WINDOWS windows that the tests' rule 2 admits (no ReLU pre-activation
    # within 2^-17 of 0 in float64, the float32 modules on the same side everywhere)
    nb = CHECK_CHUNKS
    dbl = lambda t: None if t is None else t.double()
    screened = False
    for win in range(WINDOWS):
        lo = win * nb
        part = lambda t, rows: None if t is None else t.view(rows, C, -1)[:, lo:lo + nb].reshape(rows * nb, -1).contiguous()
        s0, s1, sm, sseed = part(x0, T), part(x1, T), part(masks, T), part(seed, T)
        ss = None if st is None else st[lo:lo + nb].contiguous()
        p32, p64 = [], []
        b = {k: v.clone() for k, v in torch_backward(mod32, cfg, s0, s1, ss, sm, sseed, nb, T, p32).items()}
        r = {k: v.clone() for k, v in torch_backward(mod64, cfg, dbl(s0), dbl(s1), dbl(ss), dbl(sm), dbl(sseed), nb, T,
                                                      p64).items()}
        screened = all(float(q.abs().min()) >= 2.0 ** -17 and bool(((q > 0) == (p > 0)).all()) for p, q in zip(p32, p64))
        if screened:
            break
    a = {k: v.clone() for k, v in head.backward(s0, s1, ss, sm, T, dx=True, **{key: sseed}).items() if v is not None}
    an, bn, rn_ = named(cfg, a), named(cfg, b), named(cfg, r)
    checks = criterion(an, bn, rn_, list(rn_), role, enforce=screened)
    for c in checks.values():
        c["within"] = bool(c["fused_err_vs_float64"] <= c["tolerance"])
    mod64.zero_grad(set_to_none=True)
    del r

    ws = int(head.lib.lsm_head_backward_workspace_bytes(cfg.struct(), C, T))
    kept = forward_only()

    def backward_only():
        mod32.zero_grad(set_to_none=True)
        torch.autograd.backward([kept], [seed.reshape(kept.shape)], retain_graph=True)

    sides = {"fused": (fused, 3 if quick else 10), "torch": (plain, 2 if quick else 5),
             "torch_forward": (forward_only, 2 if quick else 5), "torch_backward": (backward_only, 2 if quick else 5)}
    for fn, _ in sides.values():   # warm-up
        fn()
    t = alternated(sides)
    res = dict(t, role=role, form="recurrent" if recurrent else "feed_forward", C=C, T=T, rows=ROWS, in0=cfg.in0,
               in1=cfg.in1, hidden=HIDDEN, recurrent_N=rn, checked_chunks=nb, checked_window=win, check_enforced=screened, checks=checks, workspace_bytes=ws,
               workspace_bytes_per_row=ws / ROWS, stages_ms=stage_times(fused),
               ratio_torch_over_fused=t["torch"]["median"] / t["fused"]["median"])
    print("%s %s: fused %.3f ms, torch forward + backward %.3f ms (x%.2f), torch backward alone %.3f ms, stages %s"
          % (role, res["form"], t["fused"]["median"], t["torch"]["median"], res["ratio_torch_over_fused"],
             t["torch_backward"]["median"], res["stages_ms"]), file=sys.stderr, flush=True)
    del kept
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    a = ap.parse_args()
    runs = [bench_head(role, rec, a.quick) for rec in (True, False) for role in ("actor", "critic")]
    emit({"heads_backward_bench": runs}, a.out)


if __name__ == "__main__":
    main()
