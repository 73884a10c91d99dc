"""``GR_MAPPO.train`` and ``GMPERunner.compute`` on the device (``onpolicy/algorithms/graph_mappo.py:244-319``,
``graph_mpe_runner.py``): the normalised advantages, ``ppo_epoch`` x ``num_mini_batch`` generator minibatches
through ``DevicePolicy.ppo_update``, and ``train_info`` -- six means and two skip counts -- accumulated where each
update left its scalars (``csrc/lsm_train_info.hip`` through ``include/lsm_train_info.h``) and divided once after
the last update.

``DeviceTrainer.train(buffer)`` makes no host read and no synchronisation; ``train_info_host`` is the one
device-to-host copy a caller who wants Python floats pays, once per ``train()``. Everything on the path besides the
accumulator is the existing pieces, used as they are: ``DeviceGraphBuffer.advantages`` and its generators,
``DevicePolicy.ppo_update``. There is no CPU fallback, as elsewhere in the project.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import capi
from ._device import DeviceOp
from .loss import STATS
from .policy import PolicyError

SLOTS = capi.TRAIN_INFO_SLOTS
# the slots GR_MAPPO.train's dict holds, and the two counts it does not
REFERENCE_KEYS, COUNT_KEYS = SLOTS[:capi.LSM_TRAIN_INFO_MEANS], SLOTS[capi.LSM_TRAIN_INFO_MEANS:]


class TrainerError(RuntimeError):
    pass


@dataclass(frozen=True)
class TrainConfig:
    """What GR_MAPPO.train reads of all_args. The defaults are the reference's (onpolicy/config.py)."""
    ppo_epoch: int = 15
    num_mini_batch: int = 1
    data_chunk_length: int = 10
    use_recurrent_policy: bool = True

    def __post_init__(self):
        if int(self.ppo_epoch) < 1 or int(self.num_mini_batch) < 1 or int(self.data_chunk_length) < 1:
            raise TrainerError("ppo_epoch, num_mini_batch and data_chunk_length must be >= 1")

    @classmethod
    def from_args(cls, all_args) -> "TrainConfig":
        """From the reference's argument names. use_naive_recurrent_policy is refused: the reference's own
        naive_recurrent_generator raises IndexError for any n_rollout_threads * num_agents > 1 (DESIGN, "Out of
        scope"), so there is nothing to reproduce."""
        if bool(getattr(all_args, "use_naive_recurrent_policy", False)):
            raise TrainerError("use_naive_recurrent_policy is not supported: the reference's "
                               "naive_recurrent_generator raises IndexError for more than one env or agent; use "
                               "use_recurrent_policy")
        return cls(ppo_epoch=int(all_args.ppo_epoch), num_mini_batch=int(all_args.num_mini_batch),
                   data_chunk_length=int(all_args.data_chunk_length),
                   use_recurrent_policy=bool(all_args.use_recurrent_policy))

    @property
    def num_updates(self) -> int:
        return int(self.ppo_epoch) * int(self.num_mini_batch)


def update_scalars(res):
    """The eight float32 0-dim device tensors (None: absent) of one DevicePolicy.ppo_update dict, in the slots'
    order. ppo_update returns imp_weights, not their mean: ratio is the loss's own stats entry, which sits in the
    stats row policy_loss is a view of (lsm.loss.STATS)."""
    pl = res.get("policy_loss")
    ratio = None
    if pl is not None:
        stats = pl._base
        if stats is None or stats.numel() != len(STATS) or pl.storage_offset() != STATS.index("policy_loss"):
            raise TrainerError("policy_loss is not a view of the loss's stats row")
        ratio = stats[STATS.index("ratio")]
    sk = res["skipped"]
    return (res.get("value_loss"), pl, res.get("dist_entropy"), res.get("actor_grad_norm"),
            res.get("critic_grad_norm"), ratio, sk.get("actor"), sk.get("critic"))


class DeviceTrainer(DeviceOp):
    """GR_MAPPO.train for one DevicePolicy: policy, loss (lsm.loss.PPOLoss), value_norm (DeviceValueNorm, or None
    without use_valuenorm), actor_opt / critic_opt (lsm.optim.DeviceAdam over [actor_encoder, actor_head] /
    [critic_encoder, critic_head] of this policy) and cfg (TrainConfig). The accumulator's state, the means and the
    feed-forward minibatches' policy rows are allocated once per trainer and stream and reused."""

    def __init__(self, policy, loss, value_norm, actor_opt, critic_opt, cfg: TrainConfig):
        if not isinstance(cfg, TrainConfig):
            raise TrainerError("cfg must be a TrainConfig")
        policy._check_optimisers(actor_opt, critic_opt, True)
        rnn = policy.actor_head.cfg.recurrent_N > 0
        if rnn and not cfg.use_recurrent_policy:
            raise TrainerError("the heads have an RNN and use_recurrent_policy is off: feed-forward minibatches "
                               "carry no recurrent states")
        super().__init__(policy.actor_head.device, TrainerError, "DeviceTrainer", "trainer")
        self.policy, self.loss, self.value_norm = policy, loss, value_norm
        self.actor_opt, self.critic_opt, self.cfg = actor_opt, critic_opt, cfg
        self._held = {}   # stream -> (state int64 [18], out float32 [8])
        self._rows = {}   # (stream, minibatch size) -> the feed-forward minibatch's policy rows
        self.last = None   # the dict of the last train()

    # ---- the accumulator -----------------------------------------------------------------------------------------

    def _buffers(self, sh):
        held = self._held.get(sh)
        if held is None:
            torch = self._torch
            held = self._held[sh] = (
                torch.empty(capi.LSM_TRAIN_INFO_STATE_WORDS, dtype=torch.int64, device=self.device),
                torch.empty(capi.LSM_TRAIN_INFO_SLOTS, dtype=torch.float32, device=self.device))
        return held

    def _add(self, state, res, first, sh):
        src = capi.LsmTrainInfoSrc()
        for k, t in enumerate(update_scalars(res)):
            src.value[k] = None if t is None else t.data_ptr()
        rc = self.lib.lsm_train_info_add(C.c_void_p(state.data_ptr()), src, int(first), C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_train_info_last_error, False, "")

    # ---- GR_MAPPO.train ------------------------------------------------------------------------------------------

    def _policy_rows(self, buffer, mb, sh):
        """A feed-forward minibatch with the policy-side rows the generator leaves to the learner: actions,
        action_log_probs and, when the buffer has them, available_actions, gathered with the yielded indices."""
        torch = self._torch
        idx = mb["indices"]
        B = idx.numel()
        samples = buffer.T * buffer.env.num_envs * buffer.env.N
        fields = [("actions", buffer.actions), ("action_log_probs", buffer.action_log_probs)]
        if buffer.available_actions is not None:
            fields.append(("available_actions", buffer.available_actions[:-1]))
        rows = self._rows.get((sh, B))
        if rows is None:
            rows = self._rows[(sh, B)] = {k: torch.empty((B, t.shape[-1]), dtype=t.dtype, device=self.device)
                                          for k, t in fields}
        for k, t in fields:
            torch.index_select(t.reshape(samples, t.shape[-1]), 0, idx, out=rows[k])
        return dict(mb, **rows)

    def train(self, buffer, update_actor: bool = True, generator=None, permutations=None):
        """GR_MAPPO.train on buffer (a DeviceGraphBuffer with policy_rows, after compute_returns):
        buffer.advantages(value_norm) once; per epoch a fresh recurrent_generator(adv, num_mini_batch,
        data_chunk_length) -- feed_forward_generator(adv, num_mini_batch) without use_recurrent_policy, with the
        policy rows gathered by three index_select calls --; per minibatch DevicePolicy.ppo_update and one
        lsm_train_info_add on the scalars it left; after the last update one lsm_train_info_mean with
        ppo_epoch * num_mini_batch, the reference's divisor whatever the generators yielded.

        generator: the torch.Generator of the epochs' permutations; train() draws one randperm per epoch and
        nothing else. permutations: instead, a list of ppo_epoch int64 permutations handed to the generators'
        chunks= / indices= -- for tests and for reproducing a run; the generators validate each with a check that
        synchronises. By default nothing in train() synchronises with the host or reads from the device.

        update_actor=False: the critic alone, as ppo_update's flag; the actor's slots (policy_loss, dist_entropy,
        actor_grad_norm, ratio, actor_skipped) take no value and report 0. (The reference still reports
        policy_loss there; this follows ppo_loss, which does not compute it.)

        Returns device tensors, valid until the next train() on this stream: train_info float32 [8] and its eight
        0-dim views under the slots' names (capi.TRAIN_INFO_SLOTS: the reference's six means, then actor_skipped
        and critic_skipped, the counts of updates a non-finite gradient skipped); advantage_stats, the float64 [3]
        of advantages(); first_nonfinite (the 0-based update that first added a non-finite scalar, -1: none) and
        updates, int64 0-dim views of the accumulator's state, and counts, its int64 [8] view of how many values
        each slot took."""
        cfg = self.cfg
        if buffer.policy_rows is None:
            raise TrainerError("the buffer has no policy_rows: train() reads the stored actions, log-probs and "
                               "recurrent states from it")
        if buffer.env.device != self.device:
            raise TrainerError("the buffer is on %s, the trainer on %s" % (buffer.env.device, self.device))
        if permutations is not None:
            permutations = list(permutations)
            if len(permutations) != cfg.ppo_epoch:
                raise TrainerError("permutations must hold ppo_epoch = %d permutations, got %d"
                                   % (cfg.ppo_epoch, len(permutations)))
        self.policy._check_optimisers(self.actor_opt, self.critic_opt, update_actor)
        sh = self._stream()
        state, out = self._buffers(sh)
        adv, adv_stats = buffer.advantages(self.value_norm)
        L = int(cfg.data_chunk_length) if cfg.use_recurrent_policy else None
        first = True
        for epoch in range(cfg.ppo_epoch):
            perm = None if permutations is None else permutations[epoch]
            if cfg.use_recurrent_policy:
                batches = buffer.recurrent_generator(adv, cfg.num_mini_batch, L, chunks=perm, generator=generator)
            else:
                batches = buffer.feed_forward_generator(adv, cfg.num_mini_batch, indices=perm, generator=generator)
            for mb in batches:
                if L is None:
                    mb = self._policy_rows(buffer, mb, sh)
                res = self.policy.ppo_update(mb, self.loss, self.value_norm, self.actor_opt, self.critic_opt,
                                             data_chunk_length=L, update_actor=update_actor)
                self._add(state, res, first, sh)
                first = False
        rc = self.lib.lsm_train_info_mean(C.c_void_p(state.data_ptr()), cfg.num_updates, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_train_info_last_error, False, "")
        W = capi.LSM_TRAIN_INFO_SLOTS
        result = {"train_info": out, "advantage_stats": adv_stats, "counts": state[W:2 * W],
                  "updates": state[2 * W], "first_nonfinite": state[2 * W + 1]}
        result.update({name: out[k] for k, name in enumerate(SLOTS)})
        self.last = result
        return result

    def train_info_host(self, out=None):
        """GR_MAPPO.train's dict as Python floats, plus the two counts as ints, from one device-to-host copy of
        train_info: the only read. out: the dict train() returned (default: the last one)."""
        out = self.last if out is None else out
        if out is None:
            raise TrainerError("train_info_host follows train()")
        host = out["train_info"].cpu()
        info = {k: float(host[i]) for i, k in enumerate(REFERENCE_KEYS)}
        info.update({k: int(host[capi.LSM_TRAIN_INFO_MEANS + i]) for i, k in enumerate(COUNT_KEYS)})
        return info

    # ---- GMPERunner.compute --------------------------------------------------------------------------------------

    def compute(self, env, buffer, rnn_states_critic=None, masks=None, **returns_kwargs):
        """GMPERunner.compute: the critic's values of the last row (DevicePolicy.get_values(..., buffer=buffer,
        row=-1)), then buffer.compute_returns(next_value, value_norm, **returns_kwargs) (gamma, gae_lambda,
        use_gae, use_proper_time_limits). rnn_states_critic / masks: by default the buffer's last rows. No host
        read. Returns next_value [M, 1], valid until the critic head's next call."""
        if rnn_states_critic is None:
            rnn_states_critic = buffer.rnn_states_critic[-1] if buffer.rnn_states_critic is not None else None
        if masks is None:
            masks = buffer.masks[-1]
        next_value = self.policy.get_values(env, rnn_states_critic, masks, buffer=buffer, row=-1)
        buffer.compute_returns(next_value, self.value_norm, **returns_kwargs)
        return next_value


__all__ = ["TrainConfig", "DeviceTrainer", "TrainerError", "PolicyError", "update_scalars", "SLOTS",
           "REFERENCE_KEYS", "COUNT_KEYS"]
