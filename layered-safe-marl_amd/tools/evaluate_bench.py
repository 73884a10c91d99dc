"""Device time of the heads' sequence form (what GR_Actor.evaluate_actions and GR_Critic.forward run after
the graph encoder on one PPO minibatch):

  (A) lsm.policy.PolicyHead.evaluate: one launch of csrc/lsm_evaluate.hip per head (two for the actor, whose
      dist_entropy is finished by a one-thread launch);
  (B) the same formulas as torch.nn modules on the device under torch.no_grad(): torch.cat, nn.LayerNorm,
      nn.Linear, nn.GRU (MIOpen) over the sequence, one step per call with h * masks[l] before it,
      torch.distributions.Categorical's log_prob and entropy and the weighted mean for the actor, v_out for
      the critic.

Shapes: the recurrent minibatch of tools/recurrent_bench.py -- 4096 envs x 8 agents x 250 steps in chunks
of 10, 16 minibatches: C = 51200 chunks of T = 10 steps, 512000 rows -- with hidden 64, layer_N 1,
recurrent_N 1; and one feed-forward minibatch of the same 512000 rows (T = 1, recurrent_N 0). The actor
reads obs (6) + the encoder's 16 columns and evaluates one of 25 stored actions; the critic reads the
encoder's 16 columns alone. Inputs and weights are seeded; 2 % of the masks are zero.

Method: both sides are run once and checked first, by the tests' criterion on the first 512 chunks (as a
minibatch of their own): the same modules in float64 are the truth, e32 is the float32 modules' error
against it, and a fused error above 4 * e32 + 4 * 2^-23 * max|truth| on the features, the final state, the
values, the log-probabilities or the entropy ends the run. Then a warm-up, HIP events on the stream around
`reps` back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds' means
(tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/evaluate_bench.py [--out FILE] [--quick]
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
ROWS, CHUNK = 512000, 10           # 4096 * 8 * 250 / 16 rows per minibatch; data_chunk_length 10
CHECK_CHUNKS = 512


def torch_evaluate(mod, cfg, x0, x1, states, masks, actions, active, C, T):
    """The sequence form from policy_bench's modules (the reference's MLPBase, RNNLayer, ACTLayer / v_out)."""
    import torch
    x = x1 if x0 is None else torch.cat([x0, x1], dim=1)
    if mod.feature_norm is not None:
        x = mod.feature_norm(x)
    for seq in mod.fc:
        x = seq(x)
    new = None
    if mod.rnn is not None:
        h = states.transpose(0, 1).contiguous()
        mk = masks.view(T, C)
        tops = []
        for l in range(T):
            h = h * mk[l].view(1, C, 1)
            y, h = mod.rnn(x[l * C:(l + 1) * C].unsqueeze(0), h)
            tops.append(y.squeeze(0))
        new = h.transpose(0, 1)
        x = mod.norm(torch.cat(tops, dim=0))
    if cfg.kind == "critic":
        return {"values": mod.out(x), "features": x, "rnn_states": new}
    x = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    dist = torch.distributions.Categorical(logits=mod.out(x))
    ent = dist.entropy()
    w = active.view(-1)
    return {"features": x, "rnn_states": new, "action_log_probs": dist.log_prob(actions.view(-1).long()).unsqueeze(1),
            "entropy": ent, "dist_entropy": (ent * w).sum() / w.sum()}


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
    mod32, mod64 = torch_head(cfg, sd, torch.float32), torch_head(cfg, sd, torch.float64)
    g = torch.Generator(device=DEV).manual_seed(7)
    x0 = torch.randn((ROWS, OBS), generator=g, device=DEV) if cfg.in0 else None
    x1 = torch.randn((ROWS, ENC), generator=g, device=DEV)
    st = 0.5 * torch.randn((C, 1, HIDDEN), generator=g, device=DEV) if rn else None
    masks = (torch.rand((ROWS, 1), generator=g, device=DEV) > 0.02).float() if rn else None
    actions = torch.randint(0, ACTIONS, (ROWS, 1), generator=g, device=DEV).float()
    active = (torch.rand((ROWS, 1), generator=g, device=DEV) > 0.1).float()

    def fused():
        return head.evaluate(x0, x1, st, masks, T, actions=actions, active_masks=active)

    def plain():
        with torch.no_grad():
            return torch_evaluate(mod32, cfg, x0, x1, st, masks, actions, active, C, T)

    # the tests' criterion on the first chunks as a minibatch of their own, against the modules in float64
    nb = CHECK_CHUNKS
    part = lambda t, rows: None if t is None else t.view(rows, C, -1)[:, :nb].reshape(rows * nb, -1).contiguous()
    s0, s1, sm, sa, sw = part(x0, T), part(x1, T), part(masks, T), part(actions, T), part(active, T)
    ss = None if st is None else st[:nb].contiguous()
    a = {k: v.clone() for k, v in head.evaluate(s0, s1, ss, sm, T, actions=sa, active_masks=sw).items()
         if not k.startswith("_")}
    dbl = lambda t: None if t is None else t.double()
    with torch.no_grad():
        b = torch_evaluate(mod32, cfg, s0, s1, ss, sm, sa, sw, nb, T)
        r = torch_evaluate(mod64, cfg, dbl(s0), dbl(s1), dbl(ss), dbl(sm), sa, dbl(sw), nb, T)
    names = ["features"] + (["rnn_states"] if rn else [])
    names += ["action_log_probs", "entropy", "dist_entropy"] if role == "actor" else ["values"]
    # the tests' rule for dist_entropy: the entropy's tolerance plus one rounding of the value
    mean_rule = lambda checks, truth: checks["entropy"]["tolerance"] + 2.0 ** -23 * float(truth.abs().item())
    checks = criterion(a, b, r, names, role, special={"dist_entropy": mean_rule})
    sides = {"fused": (fused, 5 if quick else 20), "torch": (plain, 2 if quick else 5)}
    for fn, _ in sides.values():   # warm-up
        fn()
    t = alternated(sides)
    res = dict(t, role=role, form="recurrent" if recurrent else "feed_forward", C=C, T=T, rows=ROWS, in0=cfg.in0,
               in1=cfg.in1, hidden=HIDDEN, recurrent_N=rn, checked_chunks=nb, checks=checks,
               ratio_torch_over_fused=t["torch"]["median"] / t["fused"]["median"])
    print("%s %s: fused %.3f ms, torch %.3f ms (x%.2f)" % (role, res["form"], t["fused"]["median"], t["torch"]["median"],
                                                          res["ratio_torch_over_fused"]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    a = ap.parse_args()
    runs = [bench_head(role, rec, a.quick) for rec in (True, False) for role in ("actor", "critic")]
    emit({"evaluate_bench": runs}, a.out)


if __name__ == "__main__":
    main()
