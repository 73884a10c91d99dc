"""Device time of one GR_MAPPO.train -- advantages, ppo_epoch x num_mini_batch updates, train_info -- at the
reference's default network sizes, on a buffer a DevicePolicy collected:

  (A) trainer        lsm.trainer.DeviceTrainer.train: the scalars of every update added on the device
                     (csrc/lsm_train_info.hip, one launch per update), no host read;
  (B) by_hand_text   the same loop written on the pieces (advantages, recurrent_generator, DevicePolicy.ppo_update)
                     with the reference's own accumulation (graph_mappo.py:303-308) taken literally: value_loss,
                     policy_loss and dist_entropy through .item(), the two grad norms and imp_weights.mean() added
                     as device tensors and read once at the end;
  (C) by_hand_reads  the same with all six scalars read per minibatch, which is what that text costs a caller who
                     keeps Python floats (DevicePolicy's grad norms are device tensors; the reference's are too).

Shapes: `default`, the reference's default learner shape (128 envs x 3 agents, T = 25, chunks of 10, ppo_epoch 10,
one minibatch: 10 updates of 9600 rows), and `headline` (4096 envs x 8 agents, T = 25, chunks of 10, one epoch of
25 minibatches: 25 updates of 32760 rows, the batch at which the encoders' backward passes were measured).

Method: A and B/C each own a policy, optimisers and a value normaliser built from the same state dicts and train
on the same buffer. First one train() of A against C from a seeded generator: train_info must agree to the bit
(tests/test_gpu_trainer.py's assertion, here at the bench's shapes). Then a warm-up, HIP events around `reps`
back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds' means
(alternated()). B and C contain host waits; the events span them because the next update's device work is queued
only after the read returns. No ratio is asserted: the figures are recorded as found.

    python layered-safe-marl_amd/tools/train_bench.py [--out FILE] [--quick] [--shapes default,headline]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, emit  # noqa: E402
from gnn_bench import seeded_state_dict  # noqa: E402
from policy_bench import seeded_state_dict as head_state_dict  # noqa: E402

DEV = "cuda:0"
PROFILE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "train_bench.json")
SHAPES = {
    "default": dict(envs=128, agents=3, T=25, L=10, ppo_epoch=10, num_mini_batch=1, reps=5),
    "headline": dict(envs=4096, agents=8, T=25, L=10, ppo_epoch=1, num_mini_batch=25, reps=1),
}


class Side:
    """One learner of the reference's default sizes on env: the same weights for every Side."""

    def __init__(self, env):
        from lsm import gnn, optim, policy
        from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss
        N, OBS, F = env.N, env.OBS, env.F
        acfg, ccfg = gnn.GnnConfig(F=F, aggr="node"), gnn.GnnConfig(F=F, aggr="global_mean")
        ah = policy.HeadConfig(kind="actor", in0=OBS, in1=16, num_actions=25)
        ch = policy.HeadConfig(kind="critic", in0=N * OBS, in1=16)
        self.pol = policy.DevicePolicy(
            gnn.GraphEncoder(acfg, gnn.pack_weights(seeded_state_dict(acfg), acfg, prefix=""), DEV),
            policy.PolicyHead(ah, policy.pack_head_weights(head_state_dict(ah, 1), ah), DEV),
            gnn.GraphEncoder(ccfg, gnn.pack_weights(seeded_state_dict(ccfg), ccfg, prefix=""), DEV),
            policy.PolicyHead(ch, policy.pack_head_weights(head_state_dict(ch, 2), ch), DEV))
        self.vn, self.loss = DeviceValueNorm(DEV), PPOLoss(LossConfig(num_actions=25), DEV)
        cfg = optim.AdamConfig(lr=7e-4)
        self.aopt = optim.DeviceAdam(cfg, [self.pol.actor_encoder, self.pol.actor_head], DEV)
        self.copt = optim.DeviceAdam(cfg, [self.pol.critic_encoder, self.pol.critic_head], DEV)


def collect(env, pol, T):
    import torch
    from lsm.buffer import DeviceGraphBuffer
    buf = DeviceGraphBuffer(env, episode_length=T, policy_rows=dict(hidden_size=64, recurrent_N=1, act_dim=1,
                                                                    num_actions=None))
    buf.warmup(0)
    g = torch.Generator(device=DEV).manual_seed(5)
    for t in range(T):
        out = pol.get_actions(env, buf.rnn_states[t], buf.rnn_states_critic[t], buf.masks[t], generator=g, buffer=buf)
        buf.insert_step(out["actions_env"], 0, value_preds=out["values"],
                        policy={k: out[k] for k in ("actions", "action_log_probs", "rnn_states", "rnn_states_critic")})
    return buf


def by_hand(side, buf, cfg, generator=None, reads=6):
    """GR_MAPPO.train on the pieces. reads=3: graph_mappo.py:303-308 as written (three .item(), three device
    adds); reads=6: every scalar through .item()."""
    adv, _ = buf.advantages(side.vn)
    info = dict.fromkeys(("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm", "critic_grad_norm", "ratio"), 0)
    for _ in range(cfg.ppo_epoch):
        for mb in buf.recurrent_generator(adv, cfg.num_mini_batch, cfg.data_chunk_length, generator=generator):
            r = side.pol.ppo_update(mb, side.loss, side.vn, side.aopt, side.copt, data_chunk_length=cfg.data_chunk_length)
            info["value_loss"] += r["value_loss"].item()
            info["policy_loss"] += r["policy_loss"].item()
            info["dist_entropy"] += r["dist_entropy"].item()
            if reads == 6:
                info["actor_grad_norm"] += r["actor_grad_norm"].item()
                info["critic_grad_norm"] += r["critic_grad_norm"].item()
                info["ratio"] += r["policy_loss"]._base[3].item()   # the loss's own mean of imp_weights
            else:
                info["actor_grad_norm"] += r["actor_grad_norm"]
                info["critic_grad_norm"] += r["critic_grad_norm"]
                info["ratio"] += r["imp_weights"].mean()
    return {k: float(v) / cfg.num_updates for k, v in info.items()}


def bench_shape(name, quick):
    import numpy as np
    import torch
    from lsm import hj_tables
    from lsm.config import EnvArgs
    from lsm.trainer import REFERENCE_KEYS, DeviceTrainer, TrainConfig
    from lsm.vec_env import GpuGraphVecEnv
    s = SHAPES[name]
    args = EnvArgs(num_agents=s["agents"], episode_length=s["T"], num_env_steps=s["T"] * 4, use_safety_filter=True, seed=0)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    env = GpuGraphVecEnv(args, num_envs=s["envs"], device=DEV, value_table=vt, return_numpy=False, build_infos=False)
    cfg = TrainConfig(ppo_epoch=s["ppo_epoch"], num_mini_batch=s["num_mini_batch"], data_chunk_length=s["L"])
    A, B, Cs = Side(env), Side(env), Side(env)
    tr = DeviceTrainer(A.pol, A.loss, A.vn, A.aopt, A.copt, cfg)
    buf = collect(env, A.pol, s["T"])
    tr.compute(env, buf, gamma=0.99, gae_lambda=0.95)

    # the check, which is also the warm-up: the same permutations, the same bits
    seed = lambda: torch.Generator(device=DEV).manual_seed(7)
    got = tr.train(buf, generator=seed())
    host = tr.train_info_host(got)
    want = by_hand(Cs, buf, cfg, generator=seed(), reads=6)
    text = by_hand(B, buf, cfg, generator=seed(), reads=3)
    for k in REFERENCE_KEYS:
        if np.float32(host[k]) != np.float32(want[k]):
            raise SystemExit("%s: train_info[%s] = %r, the loop by hand gives %r" % (name, k, host[k], want[k]))
    if not torch.equal(A.pol.actor_head.weights, Cs.pol.actor_head.weights):
        raise SystemExit("%s: the trainer's weights differ from the loop's by hand" % name)

    reps = max(1, s["reps"] // 2) if quick else s["reps"]
    sides = {"trainer": (lambda: tr.train(buf), reps),
             "by_hand_text": (lambda: by_hand(B, buf, cfg, reads=3), reps),
             "by_hand_reads": (lambda: by_hand(Cs, buf, cfg, reads=6), reps)}
    t = alternated(sides)
    last = tr.train_info_host()
    rows = (s["envs"] * s["agents"] * s["T"] // s["L"] // s["num_mini_batch"]) * s["L"]
    out = dict(t, shape={k: v for k, v in s.items() if k != "reps"}, updates_per_train=cfg.num_updates,
               rows_per_update=rows, train_info_first=host, train_info_text_first=text, train_info_last=last,
               first_nonfinite_last=int(tr.last["first_nonfinite"]),
               ms_per_update={k: t[k]["median"] / cfg.num_updates for k in sides},
               ratio_text_over_trainer=t["by_hand_text"]["median"] / t["trainer"]["median"],
               ratio_reads_over_trainer=t["by_hand_reads"]["median"] / t["trainer"]["median"])
    print("%s: train() %.3f ms [%.3f, %.3f]; by hand, the reference's text %.3f ms (x%.3f); six reads per minibatch "
          "%.3f ms (x%.3f); %d updates of %d rows"
          % (name, t["trainer"]["median"], t["trainer"]["min"], t["trainer"]["max"], t["by_hand_text"]["median"],
             out["ratio_text_over_trainer"], t["by_hand_reads"]["median"], out["ratio_reads_over_trainer"],
             cfg.num_updates, rows), file=sys.stderr, flush=True)
    buf.detach()
    env.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PROFILE)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    ap.add_argument("--shapes", default="default,headline")
    a = ap.parse_args()
    emit({"train_bench": {name: bench_shape(name, a.quick) for name in a.shapes.split(",")}}, a.out)


if __name__ == "__main__":
    main()
