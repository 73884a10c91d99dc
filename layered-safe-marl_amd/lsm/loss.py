"""The PPO loss and its gradient at the heads' outputs (``csrc/lsm_loss.hip`` through ``include/lsm_loss.h``):
the lines of ``GR_MAPPO.ppo_update`` and ``cal_value_loss`` (``onpolicy/algorithms/graph_mappo.py``) between
``evaluate_actions`` and ``backward()`` -- the clipped surrogate, the clipped Huber value loss, ``ValueNorm``'s
update and normalisation of the returns, the active-mask weighting -- in four launches on device tensors.

``PPOLoss.forward`` returns the four scalars and ``dlogits`` / ``dvalues``: the seeds of
``torch.autograd.backward([logits, values], [dlogits, dvalues])`` for a learner that keeps torch modules for
the backward pass. ``DeviceValueNorm`` keeps ``ValueNorm``'s running statistics on the device, where the loss
updates them, and hands ``DeviceGraphBuffer.compute_returns`` / ``.advantages`` the pair they take without an
upload. The heads' backward pass from these seeds is ``lsm.policy.PolicyHead.backward`` /
``DevicePolicy.heads_backward``. No gradient clipping and no optimiser; float32 throughout (the
reference's autocast and GradScaler are not imitated); PopArt is refused; no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import capi
from ._device import DeviceOp, OutputCache, _torch, ptr

STATS = ("policy_loss", "value_loss", "dist_entropy", "ratio")
VN_KEYS = ("running_mean", "running_mean_sq", "debiasing_term")


class LossError(RuntimeError):
    pass


@dataclass(frozen=True)
class LossConfig:
    """The fields of ``lsm_loss_config``; the defaults are the reference's (onpolicy/config.py)."""
    num_actions: int
    clip_param: float = 0.2
    huber_delta: float = 10.0
    value_loss_coef: float = 1.0
    entropy_coef: float = 0.01
    vn_beta: float = 0.99999
    use_clipped_value_loss: bool = True
    use_huber_loss: bool = True
    use_value_active_masks: bool = True
    use_policy_active_masks: bool = True
    use_valuenorm: bool = True

    @classmethod
    def from_args(cls, all_args, num_actions: int) -> "LossConfig":
        """From the reference's argument names. use_popart is refused: PopArt rescales v_out's weights."""
        if bool(getattr(all_args, "use_popart", False)):
            raise LossError("use_popart is not supported: PopArt rescales v_out's weights; use use_valuenorm")
        return cls(num_actions=int(num_actions), clip_param=float(all_args.clip_param),
                   huber_delta=float(all_args.huber_delta), value_loss_coef=float(all_args.value_loss_coef),
                   entropy_coef=float(all_args.entropy_coef),
                   use_clipped_value_loss=bool(all_args.use_clipped_value_loss),
                   use_huber_loss=bool(all_args.use_huber_loss),
                   use_value_active_masks=bool(all_args.use_value_active_masks),
                   use_policy_active_masks=bool(all_args.use_policy_active_masks),
                   use_valuenorm=bool(all_args.use_valuenorm))

    def struct(self) -> capi.LsmLossConfig:
        return capi.LsmLossConfig(vn_beta=float(self.vn_beta), clip_param=self.clip_param, huber_delta=self.huber_delta,
                                  value_loss_coef=self.value_loss_coef, entropy_coef=self.entropy_coef,
                                  use_clipped_value_loss=int(self.use_clipped_value_loss),
                                  use_huber_loss=int(self.use_huber_loss),
                                  use_value_active_masks=int(self.use_value_active_masks),
                                  use_policy_active_masks=int(self.use_policy_active_masks),
                                  use_valuenorm=int(self.use_valuenorm), num_actions=int(self.num_actions))


class DeviceValueNorm:
    """``ValueNorm(1)``'s statistics on the device: ``state`` float32 [3] = running_mean, running_mean_sq,
    debiasing_term, which ``lsm_ppo_loss`` updates in place, and ``denorm`` float32 [2] = {sqrt(var), mean}
    after the last update. ``DeviceGraphBuffer.compute_returns`` and ``.advantages`` take it as they take a
    ``ValueNorm``: through ``running_mean_var()``, here 1-element device tensors, so nothing is uploaded.
    ValueNorm's beta is the loss's (``LossConfig.vn_beta``)."""

    def __init__(self, device):
        torch = _torch()
        self.device = torch.device(device)
        self.epsilon = 1e-5
        self.state = torch.zeros(3, dtype=torch.float32, device=self.device)
        self.denorm = torch.tensor([0.1, 0.0], dtype=torch.float32, device=self.device)   # of the zero state

    def running_mean_var(self):
        """ValueNorm.running_mean_var on the device state: (mean [1], var [1])."""
        rm, rms, db = self.state[0:1], self.state[1:2], self.state[2:3]
        den = db.clamp(min=self.epsilon)
        mean = rm / den
        return mean, (rms / den - mean ** 2).clamp(min=1e-2)

    def state_dict(self):
        """The reference's keys: running_mean [1], running_mean_sq [1], debiasing_term (0-dim)."""
        return {"running_mean": self.state[0:1].clone(), "running_mean_sq": self.state[1:2].clone(),
                "debiasing_term": self.state[2].clone()}

    def load_state_dict(self, sd):
        torch = _torch()
        missing = [k for k in VN_KEYS if k not in sd]
        if missing:
            raise LossError("load_state_dict: missing %s" % ", ".join(missing))
        vals = [torch.as_tensor(sd[k], dtype=torch.float32).reshape(-1) for k in VN_KEYS]
        if any(v.numel() != 1 for v in vals):
            raise LossError("load_state_dict: every entry must hold one element (ValueNorm(1))")
        self.state.copy_(torch.cat([v.to(self.device) for v in vals]))
        mean, var = self.running_mean_var()
        self.denorm.copy_(torch.cat([torch.sqrt(var), mean]))


class PPOLoss(DeviceOp):
    """The loss on the GPU for one config. forward() returns a dict of device tensors preallocated per
    (M, stream), valid until the next call with that M on that stream."""

    def __init__(self, cfg: LossConfig, device):
        self.cfg = cfg
        super().__init__(device, LossError, "PPOLoss", "loss")
        self._struct = cfg.struct()
        self._out = OutputCache()

    def _outputs(self, M):
        torch = _torch()
        dev, f32, A = self.device, torch.float32, self.cfg.num_actions
        nbytes = int(self.lib.lsm_ppo_loss_scratch_bytes(M))
        return {"dlogits": torch.empty((M, A), dtype=f32, device=dev),
                "dvalues": torch.empty((M, 1), dtype=f32, device=dev),
                "imp_weights": torch.empty((M, 1), dtype=f32, device=dev),
                "stats": torch.empty(4, dtype=f32, device=dev),
                "_scratch": torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)}

    def forward(self, logits, values, actions=None, old_log_probs=None, advantages=None, value_preds=None,
                returns=None, active_masks=None, available_actions=None, value_norm=None, check: bool = False):
        """logits [M, A] (None: the critic half alone, update_actor=False) and values [M, 1] (None: the actor
        half alone) as the heads' sequence form leaves them; actions, old_log_probs, advantages, value_preds,
        returns, active_masks [M, 1] or [M]; available_actions [M, A]; value_norm: the DeviceValueNorm that
        use_valuenorm updates. Returns {policy_loss, value_loss, dist_entropy, ratio (0-dim views of stats
        [4]), imp_weights [M, 1], dlogits [M, A], dvalues [M, 1]}; a skipped half's entries are absent.
        Stream-ordered, no host synchronisation (check=True reads the bad-action word: one)."""
        cfg = self.cfg
        actor, critic = logits is not None, values is not None
        if not actor and not critic:
            raise LossError("logits and values are both None: nothing to do")
        M = (logits.numel() // cfg.num_actions) if actor else values.numel()
        need = lambda t, name, n=M: self._tensor(t, name, n, detach=True) if t is not None else None
        if actor:
            logits = self._tensor(logits, "logits", M * cfg.num_actions, detach=True)
            for name, t in (("actions", actions), ("old_log_probs", old_log_probs), ("advantages", advantages)):
                if t is None:
                    raise LossError("the actor half needs %s" % name)
            available_actions = need(available_actions, "available_actions", M * cfg.num_actions)
        if critic:
            for name, t in (("value_preds", value_preds), ("returns", returns)):
                if t is None:
                    raise LossError("the critic half needs %s" % name)
            if cfg.use_valuenorm and not isinstance(value_norm, DeviceValueNorm):
                raise LossError("use_valuenorm needs value_norm, a DeviceValueNorm")
            if cfg.use_valuenorm and value_norm.device != self.device:
                raise LossError("value_norm is on %s, the loss on %s" % (value_norm.device, self.device))
        vn = value_norm if critic and cfg.use_valuenorm else None
        sh = self._stream()
        out = self._out.get((M, sh), lambda: self._outputs(M))
        io = capi.LsmLossIo(logits=ptr(logits), actions=ptr(need(actions, "actions")),
                            available_actions=ptr(available_actions) if actor else None,
                            old_log_probs=ptr(need(old_log_probs, "old_log_probs")),
                            advantages=ptr(need(advantages, "advantages")),
                            active_masks=ptr(need(active_masks, "active_masks")),
                            values=ptr(need(values, "values")), value_preds=ptr(need(value_preds, "value_preds")),
                            returns=ptr(need(returns, "returns")),
                            vn_state=ptr(vn.state) if vn else None, denorm=ptr(vn.denorm) if vn else None,
                            dlogits=ptr(out["dlogits"]), dvalues=ptr(out["dvalues"]),
                            imp_weights=ptr(out["imp_weights"]), stats=ptr(out["stats"]),
                            scratch=ptr(out["_scratch"]), bad=self.bad.data_ptr())
        rc = self.lib.lsm_ppo_loss(self._struct, C.byref(io), M, C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_loss_last_error, check,
                     "a stored action that is not an integer in [0, num_actions) reached the loss")
        res = {"stats": out["stats"]}
        if actor:
            res.update(policy_loss=out["stats"][0], dist_entropy=out["stats"][2], ratio=out["stats"][3],
                       imp_weights=out["imp_weights"], dlogits=out["dlogits"])
        if critic:
            res.update(value_loss=out["stats"][1], dvalues=out["dvalues"])
        return res

    __call__ = forward
