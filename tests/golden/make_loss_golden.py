#!/usr/bin/env python
"""Record the PPO loss and its gradients FROM THE REFERENCE ITSELF (build container only).

Imports the reference's own ``GR_MAPPO`` (onpolicy/algorithms/graph_mappo.py: ``ppo_update`` and
``cal_value_loss``, with its ``huber_loss`` / ``mse_loss`` and ``ValueNorm``) with ``oracle/ref_stubs`` first on
the path and bytecode writing off, and drives ``ppo_update`` in float64 with a stub policy: its
``evaluate_actions`` returns tensors built from a leaf ``logits`` -- through the reference's
``FixedCategorical``, after the masking assignment, weighted as ``ACTLayer.evaluate_actions`` weights the
entropy -- and a leaf ``values``; its optimisers do nothing. (``GR_MAPPOPolicy`` and ``GraphReplayBuffer``,
which graph_mappo.py imports for its annotations, are replaced by empty classes.) After the call the
leaves' ``.grad`` are the gradients at the heads' outputs. One file per case under ``tests/golden/loss/`` (data only):

  config   num_actions, clip_param, huber_delta, value_loss_coef, entropy_coef, vn_beta and the five flags
  inputs   logits [M, A], actions [M], avail [M, A], old [M], adv [M], active [M], values [M], vpreds [M],
           returns [M], vn_state [3] (float32 values)
  outputs  dlogits [M, A], dvalues [M], imp_weights [M], stats [4] = policy_loss, value_loss, dist_entropy,
           mean imp_weight, vn_state_out [3], denorm [2] (float64)

Two cases, M = 40, A = 5: 'all_on' (ValueNorm, Huber, the clipped value loss, both active masks, some
unavailable actions) and 'all_off' (none of them). Every scalar of the config is exactly representable in
float32 (clip 0.25, delta 1, coefficients 0.5 and 2^-6, beta 0.75), so the float64 run has the constants of
the float32 struct; the normaliser's two clamps are not active (its state has seen data).

Usage:  python tests/golden/make_loss_golden.py
"""
from __future__ import annotations

import argparse
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import ref_harness  # noqa: E402

OUT = os.path.join(HERE, "loss")
M, A = 40, 5
FLAGS = ("use_clipped_value_loss", "use_huber_loss", "use_value_active_masks", "use_policy_active_masks",
         "use_valuenorm")


class _Params:
    def __init__(self, leaf):
        self.leaf = leaf

    def parameters(self):
        return [self.leaf]


class _NoOptimiser:
    def zero_grad(self):
        pass

    def step(self):
        pass


def record(name, on, seed):
    import types
    import torch
    # graph_mappo.py names these two classes in annotations only; their modules pull in the graph encoder's
    # dependencies, which the loss does not need
    for mod, cls in (("onpolicy.algorithms.graph_MAPPOPolicy", "GR_MAPPOPolicy"),
                     ("onpolicy.utils.graph_buffer", "GraphReplayBuffer")):
        if mod not in sys.modules:
            sys.modules[mod] = types.ModuleType(mod)
            setattr(sys.modules[mod], cls, type(cls, (), {}))
    from onpolicy.algorithms.graph_mappo import GR_MAPPO
    from onpolicy.algorithms.utils.distributions import FixedCategorical
    import loss_cases as lc
    import loss_model as lm
    from lsm.loss import LossConfig
    cfg = LossConfig(num_actions=A, clip_param=0.25, huber_delta=1.0, value_loss_coef=0.5, entropy_coef=2.0 ** -6,
                     vn_beta=0.75, **{f: on for f in FLAGS})
    inp, _ = lc.random_inputs(cfg, M, seed=seed, avail="some" if on else None, active="some")
    if on:   # this fixture keeps at least one action in every row, and the stored ones available
        inp["avail"][2, int(inp["actions"][2])] = 1.0
        inp["avail"][3, int(inp["actions"][3])] = 1.0
        inp, _ = lc.redraw(cfg, inp, seed)
    f64 = torch.float64
    t = lambda k: torch.tensor(np.asarray(inp[k]), dtype=f64)

    class Stub:
        def __init__(self):
            self.logits = t("logits").requires_grad_(True)
            self.values = t("values").reshape(M, 1).requires_grad_(True)
            self.actor, self.critic = _Params(self.logits), _Params(self.values)
            self.actor_optimizer = self.critic_optimizer = _NoOptimiser()

        def evaluate_actions(self, share_obs, obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic,
                             actions, masks, available_actions, active_masks):
            x = self.logits
            if available_actions is not None:
                x = self.logits.clone()
                x[available_actions == 0] = lm.FLT_MIN        # the masking assignment, the project's constant
            dist = FixedCategorical(logits=x)
            logp = dist.log_probs(actions)
            if on:   # ACTLayer.evaluate_actions with active masks, GR_Actor passing them with the policy flag
                ent = (dist.entropy() * active_masks.squeeze(-1)).sum() / active_masks.sum()
            else:
                ent = dist.entropy().mean()
            return self.values, logp, ent

    args = argparse.Namespace(clip_param=cfg.clip_param, ppo_epoch=1, num_mini_batch=1, data_chunk_length=1,
                              value_loss_coef=cfg.value_loss_coef, entropy_coef=cfg.entropy_coef, max_grad_norm=10.0,
                              huber_delta=cfg.huber_delta, use_recurrent_policy=False, use_naive_recurrent_policy=False,
                              use_max_grad_norm=False, use_popart=False, **{f: on for f in FLAGS})
    pol = Stub()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        trainer = GR_MAPPO(args, pol)
        trainer.tpdv = dict(dtype=f64, device=torch.device("cpu"))
        if on:
            vn = trainer.value_normalizer
            vn.tpdv = dict(trainer.tpdv)
            vn.beta = cfg.vn_beta
            vn.double()
            with torch.no_grad():
                vn.running_mean.copy_(t("vn_state")[0:1])
                vn.running_mean_sq.copy_(t("vn_state")[1:2])
                vn.debiasing_term.copy_(t("vn_state")[2])
        col = lambda k: t(k).reshape(M, 1)
        sample = (None, None, None, None, None, None, None, None, col("actions").long(), col("vpreds"), col("returns"),
                  None, col("active"), col("old"), col("adv"), t("avail") if on else None)
        res = trainer.ppo_update(sample, True)
    value_loss, _, policy_loss, dist_entropy, _, imp = res[:6]
    out = dict(dlogits=pol.logits.grad.numpy(), dvalues=pol.values.grad.reshape(M).numpy(),
               imp_weights=imp.detach().reshape(M).numpy(),
               stats=np.array([float(policy_loss.detach()), float(value_loss.detach()), float(dist_entropy.detach()),
                               float(imp.detach().mean())]))
    if on:
        mean, var = vn.running_mean_var()
        assert float(vn.debiasing_term) > 1e-5 and float(var) > 1e-2
        out["vn_state_out"] = np.array([float(vn.running_mean), float(vn.running_mean_sq), float(vn.debiasing_term)])
        out["denorm"] = np.array([float(torch.sqrt(var)), float(mean)])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    conf = {k: np.float64(getattr(cfg, k)) for k in ("clip_param", "huber_delta", "value_loss_coef", "entropy_coef",
                                                     "vn_beta")}
    conf.update({f: np.int32(on) for f in FLAGS}, num_actions=np.int32(A))
    ins = {k: np.asarray(v, np.float32) for k, v in inp.items() if v is not None}
    np.savez_compressed(path, **conf, **{"in_" + k: v for k, v in ins.items()}, **out)
    return path


def main():
    if not os.path.isdir(os.path.join(ref_harness.REF_ROOT, "onpolicy")):
        raise SystemExit("reference not available here")
    ref_harness._install_paths()
    sys.path.insert(0, os.path.join(REPO, "tests"))
    sys.path.insert(0, os.path.join(REPO, "layered-safe-marl_amd"))
    total = 0
    for name, on, seed in (("all_on", True, 51), ("all_off", False, 52)):
        total += os.path.getsize(record(name, on, seed))
    print("wrote 2 files under", OUT, total // 1024, "KB")


if __name__ == "__main__":
    main()
