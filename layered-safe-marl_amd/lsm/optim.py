"""The end of ``GR_MAPPO.ppo_update`` on the device (``csrc/lsm_optim.hip`` through ``include/lsm_optim.h``):
``clip_grad_norm_`` (or ``get_gard_norm``), ``torch.optim.Adam.step()`` and ``GradScaler.step``'s skip of a
non-finite gradient, on the packed weight blobs of ``lsm.gnn.GraphEncoder`` and ``lsm.policy.PolicyHead`` and
on the gradients their ``backward()`` left in the blobs' own layout.

``DeviceAdam(cfg, [encoder, head], device)`` is what the reference gives one ``torch.optim.Adam`` and one
``clip_grad_norm_`` call: one parameter group with its own norm, coefficient, step count and learning rate.
``step()`` updates the blobs in place -- three launches, no host synchronisation -- so the modules' next forward
call reads the new weights with no ``state_dict() -> pack -> upload``. ``DeviceAdam.step_many`` puts several
optimisers (the actor's and the critic's) into the same three launches. The differences from torch are the
header's: a float64 norm in a fixed order, the clipped gradient used but not written back, running products for
the bias corrections. There is no CPU fallback, as elsewhere in the project.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from . import capi
from ._device import DeviceOp, _torch
from .gnn import GraphEncoder, weight_entries
from .policy import PolicyHead, head_weight_entries


class OptimError(RuntimeError):
    pass


@dataclass(frozen=True)
class AdamConfig:
    """One group's hyperparameters. The defaults are the reference's (onpolicy/config.py: opti_eps,
    weight_decay, max_grad_norm, use_max_grad_norm); skip_nonfinite is GradScaler.step's behaviour."""
    lr: float
    eps: float = 1e-5
    weight_decay: float = 0.0
    betas: Tuple[float, float] = (0.9, 0.999)
    max_grad_norm: float = 10.0
    use_max_grad_norm: bool = True
    skip_nonfinite: bool = True

    @classmethod
    def from_args(cls, all_args, critic: bool = False) -> "AdamConfig":
        """From the reference's argument names: lr or critic_lr, opti_eps, weight_decay, max_grad_norm,
        use_max_grad_norm."""
        return cls(lr=float(all_args.critic_lr if critic else all_args.lr), eps=float(all_args.opti_eps),
                   weight_decay=float(all_args.weight_decay), max_grad_norm=float(all_args.max_grad_norm),
                   use_max_grad_norm=bool(all_args.use_max_grad_norm))


def _entries(module, prefix):
    """[(state-dict name, offset, floats, is a parameter)] of a module's blob, and the prefix used."""
    if isinstance(module, GraphEncoder):
        entries, off, marker = weight_entries(module.cfg), not module.cfg.layer_norm, ".layer_norm."
        prefix = "gnn." if prefix is None else prefix
    elif isinstance(module, PolicyHead):
        entries, off, marker = head_weight_entries(module.cfg), not module.cfg.feature_norm, "base.feature_norm."
        prefix = "" if prefix is None else prefix
    else:
        raise OptimError("DeviceAdam takes GraphEncoder and PolicyHead objects, got %s" % type(module).__name__)
    out, o = [], 0
    for name, shape in entries:
        n = int(np.prod(shape))
        out.append((prefix + name, o, n, not (off and marker in name)))   # the blob's unread 1 / 0 are no parameters
        o += n
    return out


class DeviceAdam(DeviceOp):
    """Adam with gradient clipping over the blobs of `modules` (GraphEncoder / PolicyHead objects): one
    parameter group. exp_avg / exp_avg_sq are one zeroed tensor per module in the blob's own layout. The entries
    that are no parameters -- the encoder's layer_norm entries with layer_norm=False, the head's feature_norm
    entries with feature_norm=False -- are left out of the segments: they stay 1 / 0 and count in neither the
    norm nor the step. prefixes: each module's state-dict prefix in state_dict() (default: 'gnn.' for an
    encoder, '' for a head, as their own state_dict())."""

    def __init__(self, cfg: AdamConfig, modules, device, prefixes=None):
        super().__init__(device, OptimError, "DeviceAdam", "optimiser")
        torch = self._torch
        self.cfg = cfg
        self.lr = float(cfg.lr)
        self.modules = list(modules)
        if not self.modules:
            raise OptimError("DeviceAdam needs at least one module")
        prefixes = list(prefixes) if prefixes is not None else [None] * len(self.modules)
        if len(prefixes) != len(self.modules):
            raise OptimError("prefixes must name every module")
        self._entries, self._runs = [], []
        names = set()
        for mod, prefix in zip(self.modules, prefixes):
            ent = _entries(mod, prefix)
            if mod.device != self.device:
                raise OptimError("a module is on %s, the optimiser on %s" % (mod.device, self.device))
            for name, _, _, is_param in ent:
                if is_param and name in names:
                    raise OptimError("two modules name a parameter %s: give them prefixes" % name)
                names.add(name)
            runs = []   # the parameter entries, merged into runs of consecutive floats: the segments
            for _, o, n, is_param in ent:
                if not is_param or n == 0:
                    continue
                if runs and runs[-1][0] + runs[-1][1] == o:
                    runs[-1][1] += n
                else:
                    runs.append([o, n])
            self._entries.append(ent)
            self._runs.append(runs)
        if sum(len(r) for r in self._runs) > capi.LSM_OPT_MAX_SEGMENTS:
            raise OptimError("the modules need more than %d segments" % capi.LSM_OPT_MAX_SEGMENTS)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.exp_avg = [torch.zeros(m.weights.numel(), **f32) for m in self.modules]
        self.exp_avg_sq = [torch.zeros(m.weights.numel(), **f32) for m in self.modules]
        self.state = torch.tensor([0.0, 1.0, 1.0, 0.0], dtype=torch.float64, device=self.device)
        self.info = torch.zeros(4, **f32)
        self._ws = {}   # stream -> the workspace of the calls this optimiser leads (step, step_many's first)

    def segments(self):
        """[(index into modules, float offset in its blob, floats)]: the group's segments, in the call's order --
        the runs of consecutive parameter entries of each blob."""
        return [(i, o, n) for i, runs in enumerate(self._runs) for o, n in runs]

    # ---- the call ------------------------------------------------------------------------------------------------

    def _grads(self):
        out = []
        for mod in self.modules:
            g = mod._last_dweights
            if g is None:
                raise OptimError("a %s has no gradient: step() follows its backward()" % type(mod).__name__)
            if isinstance(mod, GraphEncoder) and not mod._last_embed:
                raise OptimError("the encoder's last backward ran without embed=True: its EmbedConv range is "
                                 "zeros, not a gradient")
            out.append(g)
        return out

    def _fill(self, group, lr):
        cfg = self.cfg
        si = 0
        for mod, g, m, v, runs in zip(self.modules, self._grads(), self.exp_avg, self.exp_avg_sq, self._runs):
            for o, n in runs:
                s = group.segments[si]
                s.weights, s.grads = mod.weights.data_ptr() + 4 * o, g.data_ptr() + 4 * o
                s.exp_avg, s.exp_avg_sq, s.n = m.data_ptr() + 4 * o, v.data_ptr() + 4 * o, n
                si += 1
        group.n_segments = si
        group.use_max_grad_norm, group.skip_nonfinite = int(cfg.use_max_grad_norm), int(cfg.skip_nonfinite)
        group.lr = self.lr if lr is None else float(lr)
        group.beta1, group.beta2 = float(cfg.betas[0]), float(cfg.betas[1])
        group.eps, group.weight_decay, group.max_grad_norm = float(cfg.eps), float(cfg.weight_decay), float(cfg.max_grad_norm)
        group.state, group.info = self.state.data_ptr(), self.info.data_ptr()

    def _result(self):
        return {"grad_norm": self.info[0], "clip_coef": self.info[1], "skipped": self.info[2]}

    @staticmethod
    def step_many(optimisers, lr=None):
        """One lsm_optim_step call -- three launches on the current stream -- over several optimisers, one
        group each, in their order. lr: None, or one learning rate per optimiser (None: its own). Returns each
        optimiser's step() dict."""
        opts = list(optimisers)
        if not opts:
            return []
        if len(opts) > capi.LSM_OPT_MAX_GROUPS:
            raise OptimError("at most %d optimisers in one call" % capi.LSM_OPT_MAX_GROUPS)
        first = opts[0]
        lrs = list(lr) if lr is not None else [None] * len(opts)
        if len(lrs) != len(opts):
            raise OptimError("lr must name every optimiser")
        tab = (capi.LsmOptimGroup * len(opts))()
        for i, (o, l) in enumerate(zip(opts, lrs)):
            if not isinstance(o, DeviceAdam) or o.device != first.device:
                raise OptimError("step_many takes DeviceAdam objects of one device")
            o._fill(tab[i], l)
        lib, torch = first.lib, first._torch
        need = int(lib.lsm_optim_workspace_bytes(tab, len(opts)))
        if need == 0:
            raise OptimError(lib.lsm_optim_last_error().decode())
        sh = first._stream()
        ws = first._ws.get(sh)   # scratch of one call: the first optimiser's, one per stream, grown to the need
        if ws is None or ws.numel() * 8 < need:
            ws = first._ws[sh] = torch.empty(need // 8, dtype=torch.float64, device=first.device)
        rc = lib.lsm_optim_step(tab, len(opts), C.c_void_p(ws.data_ptr()), C.c_void_p(sh))
        first._finish(rc, lib.lsm_optim_last_error, False, "")
        return [o._result() for o in opts]

    def step(self, lr=None):
        """One step on each module's last backward()'s dweights (an encoder's: backward(embed=True)). lr: this
        call's learning rate instead of self.lr. Returns {'grad_norm', 'clip_coef', 'skipped'}: 0-dim device
        views of the group's info, overwritten by the next step."""
        return DeviceAdam.step_many([self], None if lr is None else [lr])[0]

    def lr_decay(self, episode, episodes):
        """The reference's update_linear_schedule: lr = cfg.lr - cfg.lr * (episode / episodes)."""
        self.lr = self.cfg.lr - (self.cfg.lr * (episode / float(episodes)))
        return self.lr

    # ---- checkpoints ---------------------------------------------------------------------------------------------

    def state_dict(self):
        """{'step': executed steps, 'exp_avg': {name: tensor}, 'exp_avg_sq': {name: tensor}} under the
        parameters' state-dict names: host copies (one download per module and moment)."""
        out = {"step": int(self.state[0].item()), "exp_avg": {}, "exp_avg_sq": {}}
        for which, blobs in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for ent, blob in zip(self._entries, blobs):
                host = blob.cpu()
                for name, o, n, is_param in ent:
                    if is_param:
                        out[which][name] = host[o:o + n].clone()
        return out

    def load_state_dict(self, sd):
        """The inverse: the moments by name, and the step count with the bias corrections' running products
        rebuilt by the same float64 multiplications, so that the optimiser continues bit-identically."""
        torch = self._torch
        step = int(sd["step"])
        if step < 0:
            raise OptimError("step must be >= 0")
        for which, blobs in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            for ent, blob in zip(self._entries, blobs):
                host = torch.zeros(blob.numel(), dtype=torch.float32)
                for name, o, n, is_param in ent:
                    if not is_param:
                        continue
                    if name not in sd[which]:
                        raise OptimError("%s: %s is missing from the state dict" % (which, name))
                    t = torch.as_tensor(sd[which][name], dtype=torch.float32).reshape(-1)
                    if t.numel() != n:
                        raise OptimError("%s: %s holds %d floats, the config needs %d" % (which, name, t.numel(), n))
                    host[o:o + n] = t
                blob.copy_(host)
        p1 = p2 = 1.0
        b1, b2 = float(self.cfg.betas[0]), float(self.cfg.betas[1])
        for _ in range(step):
            p1 *= b1
            p2 *= b2
        self.state.copy_(torch.tensor([float(step), p1, p2, 0.0], dtype=torch.float64))


def optimizer_step(actor_opt: Optional[DeviceAdam], critic_opt: DeviceAdam, update_actor: bool = True):
    """One lsm_optim_step call with the actor's and the critic's group; update_actor=False: the critic's
    alone. Returns {'actor': step() dict or None, 'critic': step() dict}."""
    if update_actor:
        a, c = DeviceAdam.step_many([actor_opt, critic_opt])
        return {"actor": a, "critic": c}
    return {"actor": None, "critic": DeviceAdam.step_many([critic_opt])[0]}
