"""Device time of the actor and critic heads (the rest of GR_Actor.forward / GR_Critic.forward after the
graph encoder) on one collect step's rows:

  (A) lsm.policy.PolicyHead: one launch of csrc/lsm_policy.hip per head;
  (B) the same formulas as torch.nn modules on the device: torch.cat, nn.LayerNorm, nn.Linear, nn.GRU
      (MIOpen), log_softmax, torch.multinomial and a gather for the actor, v_out for the critic, under
      torch.no_grad(): the launches the reference makes.

Configuration: M = 32768 rows (4096 envs x 8 agents), hidden 64, layer_N 1, recurrent_N 1, ReLU, feature
normalisation on; the actor reads obs (6) + the encoder's 16 columns and samples one of 25 actions, the
critic reads the encoder's 16 columns alone. Inputs and weights are seeded (weights ~ N(0, 1 / fan_in)).

Method: both sides are run once and checked first, by the tests' criterion on the first 4096 rows: the
same modules in float64 are the truth, e32 is the float32 modules' error against it, and a fused error above
4 * e32 + 4 * 2^-23 * max|truth| on the features, the new state, the values or the log-probability of the
action the fused head chose ends the run. Then a warm-up, HIP events on the stream around `reps`
back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds' means
(tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/policy_bench.py [--out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, criterion, emit  # noqa: E402

DEV = "cuda:0"
M, OBS, ENC, HIDDEN, ACTIONS = 32768, 6, 16, 64, 25


def torch_head(cfg, sd, dtype):
    """The head as torch.nn modules on the device (the reference's MLPBase, RNNLayer, ACTLayer / v_out)."""
    import torch
    from torch import nn
    n, Hd = cfg.in0 + cfg.in1, cfg.hidden
    act = nn.ReLU if cfg.relu else nn.Tanh

    class Head(nn.Module):
        def __init__(self):
            super().__init__()
            self.feature_norm = nn.LayerNorm(n) if cfg.feature_norm else None
            self.fc = nn.ModuleList([nn.Sequential(nn.Linear(n if k == 0 else Hd, Hd), act(), nn.LayerNorm(Hd))
                                     for k in range(cfg.layer_N + 1)])
            self.rnn = nn.GRU(Hd, Hd, num_layers=cfg.recurrent_N) if cfg.recurrent_N else None
            self.norm = nn.LayerNorm(Hd) if cfg.recurrent_N else None
            self.out = nn.Linear(Hd, cfg.out_rows)

        def forward(self, x0, x1, states, masks, sample=True):
            x = x1 if x0 is None else torch.cat([x0, x1], dim=1)
            if self.feature_norm is not None:
                x = self.feature_norm(x)
            for seq in self.fc:
                x = seq(x)
            new = None
            if self.rnn is not None:
                h = (states * masks.view(-1, 1, 1)).transpose(0, 1).contiguous()
                y, hn = self.rnn(x.unsqueeze(0), h)
                new = hn.transpose(0, 1)
                x = self.norm(y.squeeze(0))
            o = self.out(x)
            if cfg.kind == "critic":
                return {"values": o, "features": x, "rnn_states": new}
            logp = torch.log_softmax(o, dim=1)
            res = {"features": x, "rnn_states": new, "logp": logp}
            if sample:
                a = torch.multinomial(logp.exp(), 1)
                res["actions"], res["action_log_probs"] = a, logp.gather(1, a)
            return res

    head = Head()
    names = {"feature_norm": "base.feature_norm", "norm": "rnn.norm",
             "out": "act.action_out.linear" if cfg.kind == "actor" else "v_out"}
    with torch.no_grad():
        for mod, pre in names.items():
            if getattr(head, mod) is not None:
                getattr(head, mod).weight.copy_(torch.from_numpy(sd[pre + ".weight"]))
                getattr(head, mod).bias.copy_(torch.from_numpy(sd[pre + ".bias"]))
        for k, seq in enumerate(head.fc):
            pre = "base.mlp.fc1" if k == 0 else "base.mlp.fc2.%d" % (k - 1)
            for idx in (0, 2):
                seq[idx].weight.copy_(torch.from_numpy(sd["%s.%d.weight" % (pre, idx)]))
                seq[idx].bias.copy_(torch.from_numpy(sd["%s.%d.bias" % (pre, idx)]))
        for l in range(cfg.recurrent_N):
            for nm in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"):
                getattr(head.rnn, "%s_l%d" % (nm, l)).copy_(torch.from_numpy(sd["rnn.rnn.%s_l%d" % (nm, l)]))
    return head.to(DEV).to(dtype).eval()


def seeded_state_dict(cfg, seed=0):
    """Weights ~ N(0, 1 / fan_in) (the action layer too), nonzero biases, non-unit norms, as the tests use."""
    import numpy as np
    from lsm import policy
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in policy.head_weight_entries(cfg):
        if "norm" in name or name.endswith((".2.weight", ".2.bias")):
            a = 1.0 + 0.3 * rng.normal(size=shape) if name.endswith("weight") else 0.2 * rng.normal(size=shape)
        elif len(shape) == 1:
            a = 0.3 * rng.normal(size=shape)
        else:
            a = rng.normal(size=shape) / np.sqrt(shape[1])
        sd[name] = a.astype(np.float32)
    return sd


def bench_head(role, quick):
    import torch
    from lsm import policy
    if role == "actor":
        cfg = policy.HeadConfig(kind="actor", in0=OBS, in1=ENC, hidden=HIDDEN, num_actions=ACTIONS)
    else:
        cfg = policy.HeadConfig(kind="critic", in0=0, in1=ENC, hidden=HIDDEN)
    sd = seeded_state_dict(cfg, 1 if role == "actor" else 2)
    head = policy.PolicyHead(cfg, policy.pack_head_weights(sd, cfg), DEV)
    mod32, mod64 = torch_head(cfg, sd, torch.float32), torch_head(cfg, sd, torch.float64)
    g = torch.Generator(device=DEV).manual_seed(7)
    x0 = torch.randn((M, OBS), generator=g, device=DEV) if cfg.in0 else None
    x1 = torch.randn((M, ENC), generator=g, device=DEV)
    st = 0.5 * torch.randn((M, 1, HIDDEN), generator=g, device=DEV)
    masks = (torch.rand((M, 1), generator=g, device=DEV) > 0.02).float()
    u = torch.rand(M, generator=g, device=DEV)

    def fused():
        return head.forward(x0, x1, st, masks, u=u if role == "actor" else None)

    def plain():
        with torch.no_grad():
            return mod32(x0, x1, st, masks)

    # the tests' criterion on the first rows, against the same modules in float64
    nb = 4096
    a = {k: v[:nb].clone() for k, v in fused().items()}
    b = plain()
    with torch.no_grad():
        r = mod64(None if x0 is None else x0[:nb].double(), x1[:nb].double(), st[:nb].double(), masks[:nb].double(),
                  sample=False)
    b32 = {k: b[k][:nb] for k in ("features", "rnn_states")}
    if role == "actor":
        act = a["actions_env"].long().view(-1, 1)
        b32["action_log_probs"], r["action_log_probs"] = b["logp"][:nb].gather(1, act), r["logp"].gather(1, act)
    else:
        b32["values"] = b["values"][:nb]
    checks = criterion(a, b32, r, list(b32), role, bound="4 * e32 + 4 ulp =")
    if role == "actor":
        # the sampler as a distribution: the fused head's action frequencies against the float64 probabilities
        p = r["logp"].exp().mean(dim=0)
        freq = torch.bincount(a["actions_env"].long(), minlength=ACTIONS).double() / nb
        checks["action_frequency_max_abs_diff"] = float((freq - p).abs().max().item())
    sides = {"fused": (fused, 10 if quick else 50), "torch": (plain, 3 if quick else 10)}
    for fn, _ in sides.values():   # warm-up
        fn()
    t = alternated(sides)
    res = dict(t, role=role, M=M, in0=cfg.in0, in1=cfg.in1, hidden=HIDDEN, checked_rows=nb, checks=checks,
               ratio_torch_over_fused=t["torch"]["median"] / t["fused"]["median"])
    print("%s: fused %.3f ms, torch %.3f ms (x%.2f)" % (role, t["fused"]["median"], t["torch"]["median"],
                                                       res["ratio_torch_over_fused"]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    a = ap.parse_args()
    runs = [bench_head("actor", a.quick), bench_head("critic", a.quick)]
    emit({"policy_bench": runs}, a.out)


if __name__ == "__main__":
    main()
