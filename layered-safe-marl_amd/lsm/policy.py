"""The rest of ``GR_Actor.forward`` / ``GR_Critic.forward`` after the graph encoder
(``onpolicy/algorithms/graph_actor_critic.py:162-172, 406-418``) as one kernel launch per network
(``csrc/lsm_policy.hip`` through ``include/lsm_policy.h``): the virtual ``cat([obs, nbd_features])``,
``MLPBase``, the GRU ``RNNLayer``, ``ACTLayer``'s ``Categorical`` (sample or mode, log-probability) and the
critic's ``v_out``.

``PolicyHead.forward`` runs one head on device tensors; ``DevicePolicy.get_actions`` chains the two encoders
(``lsm.gnn.GraphEncoder``) and the two heads on what the step left on the device and returns what
``GR_MAPPOPolicy.get_actions`` returns, plus int32 ``[n, N]`` actions for ``step_async``: no host
synchronisation and, with a replay buffer, no torch op besides the draw of the uniforms.
``DevicePolicy.get_values`` and ``DevicePolicy.act`` are its two halves (``GMPERunner.compute``, the
evaluation loop). ``PolicyHead.evaluate`` and ``DevicePolicy.evaluate_actions`` are the sequence form
(``csrc/lsm_evaluate.hip`` through ``include/lsm_evaluate.h``): on a minibatch of ``recurrent_generator`` or
``feed_forward_generator`` the GRU state is carried through each chunk's steps, and the log-probability of
the stored action, the entropy and the values come back. ``DevicePolicy.ppo_loss`` adds the PPO loss and its
gradient at the logits and the values (``lsm.loss``). ``PolicyHead.backward`` and
``DevicePolicy.heads_backward`` carry those two gradients back through the heads (``csrc/lsm_backward.hip``
through ``include/lsm_backward.h``): the gradient of every packed head weight (``PolicyHead.gradients``) and
the gradient at the encoder's output; ``DevicePolicy.encoders_backward`` continues through the encoders,
``DevicePolicy.optimizer_step`` clips and steps both networks on the device (``lsm.optim``), and
``DevicePolicy.ppo_update`` chains the whole update without a host read. Discrete action spaces only, and no CPU
fallback, as elsewhere in the project.

Sampling is ``Categorical.sample`` as a distribution -- the inverse CDF of ``torch.rand`` uniforms -- not
torch's generator stream: the same seed does not reproduce ``torch.multinomial``'s actions.

Weights travel as one packed float32 blob per head (layout: ``include/lsm_policy.h``).
``pack_head_weights`` builds it from a ``GR_Actor`` / ``GR_Critic`` state dict, checking every shape against
the config; ``PolicyHead.load`` refreshes the device copy after an optimiser step.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import capi
from ._device import DeviceOp, OutputCache, _torch, pack_entries, ptr, unpack_entries

KINDS = {"actor": capi.LSM_HEAD_ACTOR, "critic": capi.LSM_HEAD_CRITIC}


class PolicyError(RuntimeError):
    pass


@dataclass(frozen=True)
class HeadConfig:
    """One head's shape: the fields of ``lsm_head_config``. kind: 'actor' or 'critic'; in0 / in1: the
    widths of the two input blocks (obs or cent_obs, the encoder's output); recurrent_N = 0: no RNN. The
    defaults are the reference's (onpolicy/config.py)."""
    kind: str
    in0: int
    in1: int
    hidden: int = 64
    layer_N: int = 1
    relu: bool = True
    feature_norm: bool = True
    recurrent_N: int = 1
    num_actions: Optional[int] = None

    @classmethod
    def from_args(cls, all_args, kind: str, in0: int, in1: int, num_actions: Optional[int] = None) -> "HeadConfig":
        """From the reference's argument names (recurrent_N counts only with use_recurrent_policy or
        use_naive_recurrent_policy)."""
        rnn = bool(all_args.use_recurrent_policy) or bool(all_args.use_naive_recurrent_policy)
        return cls(kind=kind, in0=int(in0), in1=int(in1), hidden=int(all_args.hidden_size),
                   layer_N=int(all_args.layer_N), relu=bool(all_args.use_ReLU),
                   feature_norm=bool(all_args.use_feature_normalization),
                   recurrent_N=int(all_args.recurrent_N) if rnn else 0,
                   num_actions=None if num_actions is None else int(num_actions))

    @property
    def out_rows(self) -> int:
        """Rows of the output Linear: num_actions (actor) or 1 (critic)."""
        return int(self.num_actions) if self.kind == "actor" else 1

    def struct(self) -> capi.LsmHeadConfig:
        if self.kind not in KINDS:
            raise ValueError("kind must be 'actor' or 'critic', got %r" % (self.kind,))
        if self.kind == "actor" and self.num_actions is None:
            raise ValueError("an actor head needs num_actions")
        return capi.LsmHeadConfig(in0=self.in0, in1=self.in1, hidden=self.hidden, layer_N=self.layer_N,
                                  relu=int(self.relu), feature_norm=int(self.feature_norm),
                                  recurrent_N=self.recurrent_N, kind=KINDS[self.kind],
                                  num_actions=int(self.num_actions or 0))


def head_weight_entries(cfg: HeadConfig):
    """[(state-dict name without prefix, shape)] in the blob's order (include/lsm_policy.h)."""
    n, Hd = cfg.in0 + cfg.in1, cfg.hidden
    out = [("base.feature_norm.weight", (n,)), ("base.feature_norm.bias", (n,)),
           ("base.mlp.fc1.0.weight", (Hd, n)), ("base.mlp.fc1.0.bias", (Hd,)),
           ("base.mlp.fc1.2.weight", (Hd,)), ("base.mlp.fc1.2.bias", (Hd,))]
    for i in range(cfg.layer_N):
        out += [("base.mlp.fc2.%d.0.weight" % i, (Hd, Hd)), ("base.mlp.fc2.%d.0.bias" % i, (Hd,)),
                ("base.mlp.fc2.%d.2.weight" % i, (Hd,)), ("base.mlp.fc2.%d.2.bias" % i, (Hd,))]
    for k in range(cfg.recurrent_N):
        out += [("rnn.rnn.weight_ih_l%d" % k, (3 * Hd, Hd)), ("rnn.rnn.weight_hh_l%d" % k, (3 * Hd, Hd)),
                ("rnn.rnn.bias_ih_l%d" % k, (3 * Hd,)), ("rnn.rnn.bias_hh_l%d" % k, (3 * Hd,))]
    if cfg.recurrent_N > 0:
        out += [("rnn.norm.weight", (Hd,)), ("rnn.norm.bias", (Hd,))]
    last = "act.action_out.linear" if cfg.kind == "actor" else "v_out"
    out += [(last + ".weight", (cfg.out_rows, Hd)), (last + ".bias", (cfg.out_rows,))]
    return out


def head_weights_floats(cfg: HeadConfig) -> int:
    """lsm_head_weights_floats(cfg); raises for a config the library refuses."""
    lib = capi.load_library()
    n = int(lib.lsm_head_weights_floats(cfg.struct()))
    if n == 0:
        raise PolicyError(lib.lsm_policy_last_error().decode())
    return n


def pack_head_weights(state_dict, cfg: HeadConfig, prefix: str = "") -> np.ndarray:
    """The packed float32 blob of a GR_Actor / GR_Critic state dict (tensors or arrays). Every entry's
    shape is checked against cfg; a missing or mis-shaped one is refused by name. Without feature
    normalisation the state dict has no base.feature_norm entries and the blob's unread gamma / beta are
    1 / 0. Entries the forward pass does not use (base.mlp.fc_h.*, gnn_base.*, PopArt's statistics) are
    ignored."""
    return pack_entries(state_dict, head_weight_entries(cfg), prefix,
                        None if cfg.feature_norm else "base.feature_norm.", lambda: head_weights_floats(cfg),
                        PolicyError, "pack_head_weights")


def unpack_head_weights(blob, cfg: HeadConfig, prefix: str = ""):
    """The inverse of pack_head_weights: {name: float32 array} (feature_norm entries only with it on)."""
    return unpack_entries(blob, head_weight_entries(cfg), prefix,
                          None if cfg.feature_norm else "base.feature_norm.", lambda: head_weights_floats(cfg),
                          PolicyError, "unpack_head_weights")


class PolicyHead(DeviceOp):
    """One head on the GPU for one config and one weight blob.

    forward() returns a dict of output tensors preallocated per (M, stream), valid until the next call
    with that M on that stream. check=True reads the call's bad-input word (one synchronisation) and
    raises when a uniform was not in [0, 1); by default the word is not read."""

    def __init__(self, cfg: HeadConfig, weights, device):
        self.cfg = cfg
        super().__init__(device, PolicyError, "PolicyHead", "head")
        self._struct = cfg.struct()
        self._out = OutputCache()
        self._eval_out = OutputCache()
        self._bwd_out = OutputCache()
        self._bwd_ws = {}   # stream -> the backward's workspace
        self._last_dweights = None
        self._alloc_weights(head_weights_floats(cfg), weights)

    def load(self, state_dict, prefix: str = ""):
        """Refresh the blob from a GR_Actor / GR_Critic state dict (after each optimiser step)."""
        self._set(pack_head_weights(state_dict, self.cfg, prefix))

    def state_dict(self, prefix: str = ""):
        """The current device blob as {name: float32 tensor}, the inverse of load (unpack_head_weights; one
        download): a checkpoint after lsm.optim.DeviceAdam's steps needs no torch module."""
        torch = _torch()
        blob = self.weights.cpu().numpy()
        return {k: torch.from_numpy(v) for k, v in unpack_head_weights(blob, self.cfg, prefix).items()}

    def _inputs(self, x0, x1, rnn_states, masks, T, shape, who):
        """forward's and evaluate's (R, x0, x1, rnn_states, masks) after their checks: R rows, taken from x1,
        in chunks of T steps (forward: 1) with one row of GRU state each. shape and who are the caller's
        words in the refusals."""
        cfg = self.cfg
        if not isinstance(x1, self._torch.Tensor) or x1.dim() < 1:
            raise PolicyError("x1 must be a CUDA (HIP) tensor %s; there is no CPU fallback" % shape)
        if cfg.in1 < 1:
            raise PolicyError("%s takes the row count from x1: the config needs in1 >= 1" % who)
        R = x1.numel() // cfg.in1
        if T < 1 or R % T:
            raise PolicyError("%d rows are not chunks of T = %d steps" % (R, T))
        x1 = self._tensor(x1, "x1", R * cfg.in1)
        if cfg.in0:
            if x0 is None:
                raise PolicyError("the head was built with in0 = %d: x0 is needed" % cfg.in0)
            x0 = self._tensor(x0, "x0", R * cfg.in0)
        else:
            x0 = None
        if cfg.recurrent_N:
            if rnn_states is None or masks is None:
                raise PolicyError("a recurrent head needs rnn_states and masks")
            rnn_states = self._tensor(rnn_states, "rnn_states", R // T * cfg.recurrent_N * cfg.hidden)
            masks = self._tensor(masks, "masks", R)
        else:
            rnn_states = masks = None
        return R, x0, x1, rnn_states, masks

    def _outputs(self, M):
        torch = _torch()
        cfg, dev, f32 = self.cfg, self.device, torch.float32
        out = {"features": torch.empty((M, cfg.hidden), dtype=f32, device=dev)}
        if cfg.recurrent_N:
            out["rnn_states"] = torch.empty((M, cfg.recurrent_N, cfg.hidden), dtype=f32, device=dev)
        if cfg.kind == "actor":
            out["actions_env"] = torch.empty((M,), dtype=torch.int32, device=dev)
            out["actions"] = torch.empty((M, 1), dtype=f32, device=dev)
            out["action_log_probs"] = torch.empty((M, 1), dtype=f32, device=dev)
        else:
            out["values"] = torch.empty((M, 1), dtype=f32, device=dev)
        return out

    def forward(self, x0, x1, rnn_states=None, masks=None, u=None, available_actions=None, check: bool = False):
        """x0 [M, in0] (None when in0 == 0), x1 [M, in1], rnn_states [M, recurrent_N, hidden], masks [M, 1]
        or [M], u [M] uniforms in [0, 1) (None: the mode), available_actions [M, num_actions] float32.
        Actor: {actions_env int32 [M], actions [M, 1], action_log_probs [M, 1], features, rnn_states};
        critic: {values [M, 1], features, rnn_states} (rnn_states only with an RNN)."""
        cfg = self.cfg
        M, x0, x1, rnn_states, masks = self._inputs(x0, x1, rnn_states, masks, 1, "[M, in1]", "PolicyHead.forward")
        actor = cfg.kind == "actor"
        if actor and u is not None:
            u = self._tensor(u, "u", M)
        if actor and available_actions is not None:
            available_actions = self._tensor(available_actions, "available_actions", M * cfg.num_actions)
        sh = self._stream()
        out = self._out.get((M, sh), lambda: self._outputs(M))
        io = capi.LsmHeadIo(x0=ptr(x0), x1=ptr(x1), rnn_states=ptr(rnn_states), masks=ptr(masks),
                            u=ptr(u) if actor else None, available_actions=ptr(available_actions) if actor else None,
                            actions_i32=ptr(out.get("actions_env")), actions_f32=ptr(out.get("actions")),
                            log_probs=ptr(out.get("action_log_probs")), logits=None, values=ptr(out.get("values")),
                            features=ptr(out["features"]), rnn_out=ptr(out.get("rnn_states")),
                            bad=self.bad.data_ptr())
        rc = self.lib.lsm_head_forward(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), M,
                                       C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_policy_last_error, check, "a uniform outside [0, 1) reached the sampler")
        return out

    __call__ = forward

    def _eval_outputs(self, Cn, T):
        torch = _torch()
        cfg, dev, f32, R = self.cfg, self.device, torch.float32, Cn * T
        out = {"features": torch.empty((R, cfg.hidden), dtype=f32, device=dev)}
        if cfg.recurrent_N:
            out["rnn_states"] = torch.empty((Cn, cfg.recurrent_N, cfg.hidden), dtype=f32, device=dev)
        if cfg.kind == "actor":
            out["action_log_probs"] = torch.empty((R, 1), dtype=f32, device=dev)
            out["entropy"] = torch.empty((R,), dtype=f32, device=dev)
            out["dist_entropy"] = torch.empty((), dtype=f32, device=dev)
            nbytes = int(self.lib.lsm_head_evaluate_scratch_bytes(Cn, T))
            out["_scratch"] = torch.empty((max(nbytes, 8) // 8,), dtype=torch.float64, device=dev)
        else:
            out["values"] = torch.empty((R, 1), dtype=f32, device=dev)
        return out

    def evaluate(self, x0, x1, rnn_states, masks, T, actions=None, available_actions=None, active_masks=None,
                 check: bool = False, logits: bool = False):
        """The sequence form (include/lsm_evaluate.h) on a time-major minibatch of C chunks of T steps, as
        recurrent_generator yields it: x0 [T*C, in0] (None when in0 == 0), x1 [T*C, in1], rnn_states
        [C, recurrent_N, hidden] (each chunk's state at its first step), masks [T*C, 1] or [T*C], actions
        [T*C, 1] float32 (actor), available_actions [T*C, num_actions], active_masks [T*C, 1] (the weights of
        dist_entropy; None: the mean). T=None: feed-forward rows (T = 1). Returns preallocated device
        tensors, cached per (C, T, stream) and valid until the next call with them:
        actor {action_log_probs [T*C, 1], entropy [T*C], dist_entropy (0-dim), features, rnn_states};
        critic {values [T*C, 1], features, rnn_states} (rnn_states [C, recurrent_N, hidden]: the state
        after the last step, only with an RNN). logits=True (actor): the dict also holds 'logits' [T*C,
        num_actions], the rows after the availability mask -- what lsm.loss.PPOLoss takes; every other output is
        the same bytes. check=True reads the bad-input word (one synchronisation) and raises when a stored
        action was not an integer in [0, num_actions)."""
        cfg = self.cfg
        T = 1 if T is None else int(T)
        R, x0, x1, rnn_states, masks = self._inputs(x0, x1, rnn_states, masks, T, "[T*C, in1]", "PolicyHead.evaluate")
        Cn = R // T
        actor = cfg.kind == "actor"
        if actor:
            if actions is None:
                raise PolicyError("the actor evaluates stored actions: actions is needed")
            actions = self._tensor(actions, "actions", R)
            if available_actions is not None:
                available_actions = self._tensor(available_actions, "available_actions", R * cfg.num_actions)
            if active_masks is not None:
                active_masks = self._tensor(active_masks, "active_masks", R)
        else:
            actions = available_actions = active_masks = None
        sh = self._stream()
        out = self._eval_out.get((Cn, T, sh), lambda: self._eval_outputs(Cn, T))
        keep_logits = bool(logits) and actor
        if keep_logits and "_logits" not in out:
            torch = _torch()
            out["_logits"] = torch.empty((R, cfg.num_actions), dtype=torch.float32, device=self.device)
        io = capi.LsmEvalIo(x0=ptr(x0), x1=ptr(x1), rnn_states=ptr(rnn_states), masks=ptr(masks), actions=ptr(actions),
                            available_actions=ptr(available_actions), active_masks=ptr(active_masks),
                            log_probs=ptr(out.get("action_log_probs")), entropy=ptr(out.get("entropy")),
                            dist_entropy=ptr(out.get("dist_entropy")),
                            logits=ptr(out["_logits"]) if keep_logits else None, values=ptr(out.get("values")),
                            features=ptr(out["features"]), rnn_out=ptr(out.get("rnn_states")),
                            scratch=ptr(out.get("_scratch")), bad=self.bad.data_ptr())
        rc = self.lib.lsm_head_evaluate(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), Cn, T,
                                        C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_policy_last_error, check,
                     "a stored action that is not an integer in [0, num_actions) reached evaluate")
        return dict(out, logits=out["_logits"]) if keep_logits else out

    def _bwd_outputs(self, Cn, T):
        torch = _torch()
        cfg, dev, f32, R = self.cfg, self.device, torch.float32, Cn * T
        return {"dweights": torch.empty((self._n,), dtype=f32, device=dev),
                "dx0": torch.empty((R, cfg.in0), dtype=f32, device=dev) if cfg.in0 else None,
                "dx1": torch.empty((R, cfg.in1), dtype=f32, device=dev)}

    def _bwd_workspace(self, Cn, T, sh):
        """The stream's one workspace, grown to the largest need seen on it (never one per minibatch size: it
        is 6.8 KB per row at the reference's defaults, 3.5 GB at 512000 rows)."""
        nbytes = int(self.lib.lsm_head_backward_workspace_bytes(self._struct, Cn, T))
        if nbytes == 0:
            raise PolicyError(self.lib.lsm_policy_last_error().decode())
        ws = self._bwd_ws.get(sh)
        if ws is None or ws.numel() * 8 < nbytes:
            self._bwd_ws.pop(sh, None)   # released first: the two need not be held together
            ws = None
            torch = _torch()
            ws = self._bwd_ws[sh] = torch.empty((nbytes // 8,), dtype=torch.float64, device=self.device)
        return ws

    def backward(self, x0, x1, rnn_states, masks, T, dlogits=None, dvalues=None, available_actions=None,
                 dx: bool = False):
        """The backward pass (include/lsm_backward.h) on evaluate's minibatch: x0, x1, rnn_states, masks and T
        as evaluate takes them, and the gradient at the head's output -- dlogits [T*C, num_actions] (actor;
        entries under available_actions == 0 are read as 0) or dvalues [T*C, 1] or [T*C] (critic), as
        lsm.loss.PPOLoss returns them. Four launches, no host synchronisation. Returns preallocated device
        tensors, cached per (C, T, stream) and valid until the next call with them: dweights [floats of the
        blob] -- the gradient of every packed weight in the blob's own layout, overwritten, not accumulated
        (gradients() names its entries) -- and, with dx=True, dx0 [T*C, in0] (None when in0 == 0) and dx1
        [T*C, in1], the gradient at the two input blocks; with dx=False they are not computed and come back
        as None. The workspace (lsm_head_backward_workspace_bytes: about 6.8 KB per row at the reference's
        defaults, 3.5 GB at 512000 rows) is held once per stream and grown to the largest call seen on it."""
        cfg = self.cfg
        T = 1 if T is None else int(T)
        R, x0, x1, rnn_states, masks = self._inputs(x0, x1, rnn_states, masks, T, "[T*C, in1]", "PolicyHead.backward")
        Cn = R // T
        if cfg.kind == "actor":
            if dlogits is None:
                raise PolicyError("the actor's backward starts from dlogits")
            dlogits = self._tensor(dlogits, "dlogits", R * cfg.num_actions)
            if available_actions is not None:
                available_actions = self._tensor(available_actions, "available_actions", R * cfg.num_actions)
            dvalues = None
        else:
            if dvalues is None:
                raise PolicyError("the critic's backward starts from dvalues")
            dvalues = self._tensor(dvalues, "dvalues", R)
            dlogits = available_actions = None
        sh = self._stream()
        out = self._bwd_out.get((Cn, T, sh), lambda: self._bwd_outputs(Cn, T))
        ws = self._bwd_workspace(Cn, T, sh)
        io = capi.LsmBwdIo(x0=ptr(x0), x1=ptr(x1), rnn_states=ptr(rnn_states), masks=ptr(masks),
                           available_actions=ptr(available_actions), dlogits=ptr(dlogits), dvalues=ptr(dvalues),
                           dweights=ptr(out["dweights"]), dx0=ptr(out["dx0"]) if dx else None,
                           dx1=ptr(out["dx1"]) if dx else None, workspace=ptr(ws))
        rc = self.lib.lsm_head_backward(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), Cn, T,
                                        C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_policy_last_error, False, "")
        self._last_dweights = out["dweights"]
        return {"dweights": out["dweights"], "dx0": out["dx0"] if dx else None, "dx1": out["dx1"] if dx else None}

    def gradients(self, prefix: str = ""):
        """{state-dict name: gradient}: views, without a copy, of the last backward()'s dweights in the
        parameters' shapes, under the names of head_weight_entries (feature_norm entries only with it on).
        They are that call's cached tensor: valid until the next backward() with its (C, T, stream)."""
        if self._last_dweights is None:
            raise PolicyError("gradients() follows a backward()")
        out, o = {}, 0
        for name, shape in head_weight_entries(self.cfg):
            n = int(np.prod(shape))
            if self.cfg.feature_norm or "base.feature_norm." not in name:
                out[prefix + name] = self._last_dweights[o:o + n].view(shape)
            o += n
        return out


class DevicePolicy:
    """GR_MAPPOPolicy's forward methods on the device. get_actions: the actor's and the critic's encoder and
    head, four launches on what the step left behind; act and get_values: its actor and critic halves;
    evaluate_actions: both encoders and the heads' sequence form on a minibatch of the buffer's generators.

    actor_encoder / critic_encoder: lsm.gnn.GraphEncoder; actor_head / critic_head: PolicyHead. The
    critic's 'node' aggregation (critic_graph_aggr == 'node': all agents' rows concatenated,
    gnn_out_dim * num_agents wide) is not what the encoder produces and is refused; the default 'global' works."""

    def __init__(self, actor_encoder, actor_head, critic_encoder, critic_head):
        if actor_head.cfg.kind != "actor" or critic_head.cfg.kind != "critic":
            raise PolicyError("DevicePolicy takes (actor_encoder, actor_head, critic_encoder, critic_head)")
        if critic_encoder.cfg.aggr == "node":
            raise PolicyError("the critic's 'node' aggregation concatenates every agent's encoder row "
                              "(gnn_out_dim * num_agents); the encoder does not produce that: use "
                              "critic_graph_aggr = 'global'")
        for enc, head, what in ((actor_encoder, actor_head, "actor"), (critic_encoder, critic_head, "critic")):
            if head.cfg.in1 != enc.cfg.out_dim:
                raise PolicyError("the %s head's in1 = %d, its encoder's out_dim = %d"
                                  % (what, head.cfg.in1, enc.cfg.out_dim))
        if actor_head.cfg.recurrent_N != critic_head.cfg.recurrent_N or actor_head.cfg.hidden != critic_head.cfg.hidden:
            raise PolicyError("the two heads differ in recurrent_N or hidden")
        self.actor_encoder, self.actor_head = actor_encoder, actor_head
        self.critic_encoder, self.critic_head = critic_encoder, critic_head
        self.last_actor = self.last_critic = None   # the heads' own output dicts of the last call (features too)
        self.last_head_inputs = None   # evaluate_actions' (x0, encoder output) per head, for heads_backward

    def get_actions(self, env, rnn_states, rnn_states_critic, masks, deterministic: bool = False, generator=None,
                    available_actions=None, buffer=None):
        """One collect step's policy outputs for env (a GpuGraphVecEnv with return_numpy=False). The
        inputs are read where the last step or reset wrote them: the env's own tensors, or, with
        buffer (a DeviceGraphBuffer bound to env, whose rings take the step's outputs instead), row
        buffer.step of the buffer. rnn_states / rnn_states_critic [M, recurrent_N, hidden] and masks [M, 1]
        (or their [n, N, ...] buffer rows) are ignored without an RNN.

        Returns device tensors: values [M, 1], actions [M, 1] float32, action_log_probs [M, 1], rnn_states
        and rnn_states_critic [M, recurrent_N, hidden] (the inputs themselves without an RNN), actions_env
        int32 [n, N]. They are valid until the next call."""
        src = self._step_inputs(env, buffer)
        cent = self._cent_obs(env, src)
        a = self._act(env, src, rnn_states, masks, deterministic, generator, available_actions)
        c = self._values(env, src, cent, rnn_states_critic, masks)
        return {"values": c["values"], "actions": a["actions"], "action_log_probs": a["action_log_probs"],
                "rnn_states": a.get("rnn_states", rnn_states),
                "rnn_states_critic": c.get("rnn_states", rnn_states_critic),
                "actions_env": a["actions_env"].view(env.num_envs, env.N)}

    def get_values(self, env, rnn_states_critic, masks, buffer=None, row=None):
        """GR_MAPPOPolicy.get_values: the critic half of get_actions alone (the critic's encoder and head,
        two launches), on the same inputs -- row buffer.step of buffer (or its row `row`), or the env's own
        tensors. GMPERunner.compute calls it on the last row before compute_returns: after the T-th
        insert_step buffer.step has wrapped to 0, so that call passes row=-1. Returns values [M, 1], valid
        until the critic head's next call."""
        src = self._step_inputs(env, buffer, row)
        return self._values(env, src, self._cent_obs(env, src), rnn_states_critic, masks)["values"]

    def act(self, env, rnn_states, masks, deterministic: bool = True, generator=None, available_actions=None,
            buffer=None):
        """GR_MAPPOPolicy.act: the actor half of get_actions alone (the actor's encoder and head, two
        launches), deterministic by default as in the evaluation loop. Returns {actions [M, 1] float32,
        actions_env int32 [n, N], rnn_states [M, recurrent_N, hidden] (the input itself without an RNN)}."""
        src = self._step_inputs(env, buffer)
        a = self._act(env, src, rnn_states, masks, deterministic, generator, available_actions)
        return {"actions": a["actions"], "actions_env": a["actions_env"].view(env.num_envs, env.N),
                "rnn_states": a.get("rnn_states", rnn_states)}

    def _step_inputs(self, env, buffer, row=None):
        """(obs, node_obs, adj, adj_mask, share_obs) where the last step or reset wrote them."""
        if env.return_numpy:
            raise PolicyError("DevicePolicy needs an env built with return_numpy=False")
        if buffer is None:
            obs, node, adj, adj_mask, share = env.t_obs, env.t_node, env.t_adj, env.t_adj_mask, None
        else:
            if buffer.env is not env:
                raise PolicyError("buffer belongs to another env")
            t = buffer.step if row is None else int(row)
            obs, node, adj, share = buffer.obs[t], buffer.node_obs[t], buffer.adj[t], buffer.share_obs[t]
            adj_mask = None if buffer.adj_mask is None else buffer.adj_mask[t]
        if self.actor_head.cfg.in0 != env.OBS:
            raise PolicyError("the actor head's in0 = %d, the env's obs are %d wide" % (self.actor_head.cfg.in0, env.OBS))
        return obs, node, adj, adj_mask, share

    def _cent_obs(self, env, src):
        """The critic head's first input block, chosen by its width: share_obs, obs, or nothing."""
        obs, share = src[0], src[4]
        n, N, OBS = env.num_envs, env.N, env.OBS
        ch = self.critic_head.cfg
        cent = None
        if ch.in0:
            if share is not None and share.shape[-1] == ch.in0:
                cent = share
            elif ch.in0 == OBS:
                cent = obs
            elif ch.in0 == N * OBS:
                # without a buffer there is no share_obs row: every agent's row is the env's obs, concatenated
                cent = obs.reshape(n, 1, N * OBS).expand(n, N, N * OBS).contiguous()
            else:
                raise PolicyError("the critic head's in0 = %d is neither the obs width %d nor the shared %d"
                                  % (ch.in0, OBS, N * OBS))
        return cent

    def _act(self, env, src, rnn_states, masks, deterministic, generator, available_actions):
        torch = _torch()
        obs, node, adj, adj_mask, _ = src
        M = env.num_envs * env.N
        u = None if deterministic else torch.rand(M, generator=generator, device=env.device, dtype=torch.float32)
        a_feat = self.actor_encoder.forward_step(node, adj, adj_mask, env.N, env.agent_id)
        a = self.actor_head.forward(obs, a_feat, rnn_states, masks, u=u, available_actions=available_actions)
        self.last_actor = a
        return a

    def _values(self, env, src, cent, rnn_states_critic, masks):
        _, node, adj, adj_mask, _ = src
        c_feat = self.critic_encoder.forward_step(node, adj, adj_mask, env.N, env.agent_id)
        c = self.critic_head.forward(cent, c_feat, rnn_states_critic, masks)
        self.last_critic = c
        return c

    def evaluate_actions(self, mb, data_chunk_length=None, check: bool = False, logits: bool = False):
        """GR_MAPPOPolicy.evaluate_actions on one minibatch: a dict yielded by
        DeviceGraphBuffer.recurrent_generator (data_chunk_length: the generator's) or by
        feed_forward_generator (data_chunk_length None; the learner adds its own 'actions' rows, and
        'available_actions' if it has them, gathered with the yielded indices). Both encoders run
        GraphEncoder.forward(mb['node_obs'], mb['adj'], mb['agent_id']), both heads their sequence form
        (PolicyHead.evaluate): six launches, no host synchronisation, no torch op besides views. The
        critic's first input block is mb['share_obs'] or mb['obs'], whichever has its width.

        Returns device tensors, valid until the next call: values [L*C, 1], action_log_probs [L*C, 1],
        dist_entropy (0-dim; weighted by mb['active_masks'] when the batch has them) and entropy [L*C];
        with logits=True also logits [L*C, num_actions] (one more store in the actor's launch)."""
        ah, ch = self.actor_head.cfg, self.critic_head.cfg
        if mb.get("adj") is None:
            raise PolicyError("the minibatch has no dense adj (edges=True): the encoder reads the [B, E, E] matrix")
        obs = mb["obs"]
        if obs.shape[-1] != ah.in0:
            raise PolicyError("the actor head's in0 = %d, the minibatch's obs are %d wide" % (ah.in0, obs.shape[-1]))
        cent = None
        if ch.in0:
            share = mb.get("share_obs")
            if share is not None and share.shape[-1] == ch.in0:
                cent = share
            elif obs.shape[-1] == ch.in0:
                cent = obs
            else:
                raise PolicyError("the critic head's in0 = %d is the width of neither share_obs nor obs" % ch.in0)
        if mb.get("actions") is None:
            raise PolicyError("the minibatch has no 'actions' rows to evaluate")
        T = None if data_chunk_length is None else int(data_chunk_length)
        a_feat = self.actor_encoder.forward(mb["node_obs"], mb["adj"], mb["agent_id"])
        a = self.actor_head.evaluate(obs, a_feat, mb.get("rnn_states"), mb.get("masks"), T, actions=mb["actions"],
                                     available_actions=mb.get("available_actions"),
                                     active_masks=mb.get("active_masks"), check=check, logits=logits)
        c_feat = self.critic_encoder.forward(mb["node_obs"], mb["adj"], mb["agent_id"])
        c = self.critic_head.evaluate(cent, c_feat, mb.get("rnn_states_critic"), mb.get("masks"), T)
        self.last_actor, self.last_critic = a, c
        self.last_head_inputs = {"actor": (obs, a_feat), "critic": (cent, c_feat)}   # what heads_backward needs
        out = {"values": c["values"], "action_log_probs": a["action_log_probs"], "dist_entropy": a["dist_entropy"],
               "entropy": a["entropy"]}
        if logits:
            out["logits"] = a["logits"]
        return out

    def ppo_loss(self, mb, loss, value_norm=None, data_chunk_length=None, update_actor: bool = True,
                 check: bool = False):
        """The head of GR_MAPPO.ppo_update on one minibatch: evaluate_actions with the logits kept, then
        `loss` (an lsm.loss.PPOLoss) on the minibatch's old_action_log_probs (or action_log_probs, as the
        generators name the stored rows), adv_targ (or advantages), value_preds, returns and active_masks. value_norm: the
        DeviceValueNorm that use_valuenorm updates. update_actor=False: the critic half alone, as the
        reference's flag. Ten launches, no host synchronisation. Returns device tensors, valid until the
        next call: policy_loss, value_loss, dist_entropy, ratio (0-dim), imp_weights [L*C, 1], dlogits
        [L*C, num_actions], dvalues [L*C, 1] -- the seeds of torch.autograd.backward([logits, values],
        [dlogits, dvalues]) -- and the forward's logits, values and action_log_probs."""
        def first(*names):
            for k in names:
                if mb.get(k) is not None:
                    return mb[k]
            raise PolicyError("the minibatch has none of %s" % " / ".join(names))

        if loss.cfg.num_actions != self.actor_head.cfg.num_actions:
            raise PolicyError("the loss was built for %d actions, the actor head for %d"
                              % (loss.cfg.num_actions, self.actor_head.cfg.num_actions))
        ev = self.evaluate_actions(mb, data_chunk_length, check=check, logits=True)
        out = loss.forward(ev["logits"] if update_actor else None, ev["values"], actions=mb["actions"],
                           old_log_probs=first("old_action_log_probs", "action_log_probs"),
                           advantages=first("adv_targ", "advantages"), value_preds=first("value_preds"),
                           returns=first("returns"), active_masks=mb.get("active_masks"),
                           available_actions=mb.get("available_actions"), value_norm=value_norm, check=check)
        return dict(out, logits=ev["logits"], values=ev["values"], action_log_probs=ev["action_log_probs"])

    def heads_backward(self, mb, loss_out, data_chunk_length=None, update_actor: bool = True, dx: bool = False):
        """The heads' half of loss.backward() on the minibatch ppo_loss (or evaluate_actions) just ran on and
        the dict ppo_loss returned: PolicyHead.backward of both heads from loss_out's dlogits and dvalues, on
        the encoder outputs evaluate_actions kept (last_head_inputs; the encoders' next call overwrites them).
        update_actor=False: the critic alone, as ppo_loss's flag. Two head calls, eight launches, no host
        synchronisation. Returns {'actor': ..., 'critic': ...}, each PolicyHead.backward's dict ('actor' None
        without update_actor); with dx=True their dx1 is the gradient at each encoder's output, the seed of
        the encoder's backward. Every weight's gradient is then in actor_head.gradients() /
        critic_head.gradients()."""
        if self.last_head_inputs is None:
            raise PolicyError("heads_backward follows ppo_loss or evaluate_actions on the same minibatch")
        if self.actor_encoder is self.critic_encoder:
            raise PolicyError("heads_backward needs two encoder objects: a shared one's cached output holds the "
                              "critic's features by now, and the actor would be differentiated at them")
        T = None if data_chunk_length is None else int(data_chunk_length)
        out = {"actor": None}
        if update_actor:
            if loss_out.get("dlogits") is None:
                raise PolicyError("loss_out has no dlogits")
            x0, x1 = self.last_head_inputs["actor"]
            out["actor"] = self.actor_head.backward(x0, x1, mb.get("rnn_states"), mb.get("masks"), T,
                                                    dlogits=loss_out["dlogits"],
                                                    available_actions=mb.get("available_actions"), dx=dx)
        if loss_out.get("dvalues") is None:
            raise PolicyError("loss_out has no dvalues")
        x0, x1 = self.last_head_inputs["critic"]
        out["critic"] = self.critic_head.backward(x0, x1, mb.get("rnn_states_critic"), mb.get("masks"), T,
                                                  dvalues=loss_out["dvalues"], dx=dx)
        return out

    def encoders_backward(self, mb, heads_out, update_actor: bool = True, dh0: bool = False, embed: bool = False):
        """The encoders' half, after heads_backward(..., dx=True) on the same minibatch: GraphEncoder.backward of
        both encoders on mb['node_obs'], mb['adj'], mb['agent_id'] from each head's dx1, the gradient at the
        encoder's output. update_actor=False: the critic's encoder alone. Two encoder calls, four launches, no
        host synchronisation. Returns {'actor': ..., 'critic': ...}, each GraphEncoder.backward's dict ('actor'
        None without update_actor); every conv-layer weight's gradient is then in actor_encoder.gradients() /
        critic_encoder.gradients(), and with dh0=True each dict's dh0 is the gradient at EmbedConv's output.
        embed=True: GraphEncoder.embed_backward follows each call on the same stream, seeded by that dh0 (two more
        launches per encoder), and gradients() then names every encoder weight's gradient, EmbedConv's included;
        by default the EmbedConv entries are 0, as before. Every graph size the encoders' forward accepts is
        accepted (GraphEncoder.backward goes to the spilled tier beyond lsm_gnn_backward's LDS limit)."""
        if self.last_head_inputs is None:
            raise PolicyError("heads_backward follows ppo_loss or evaluate_actions on the same minibatch")
        if self.actor_encoder is self.critic_encoder:
            raise PolicyError("heads_backward needs two encoder objects: a shared one's cached output holds the "
                              "critic's features by now, and the actor would be differentiated at them")
        if mb.get("adj") is None:
            raise PolicyError("the minibatch has no dense adj (edges=True): the encoder reads the [B, E, E] matrix")
        out = {"actor": None}
        for who, enc in (("actor", self.actor_encoder), ("critic", self.critic_encoder)):
            if who == "actor" and not update_actor:
                continue
            h = heads_out.get(who)
            if h is None or h.get("dx1") is None:
                raise PolicyError("heads_out has no %s dx1: call heads_backward(..., dx=True)" % who)
            out[who] = enc.backward(mb["node_obs"], mb["adj"], h["dx1"], mb["agent_id"], dh0=dh0, embed=embed)
        return out

    def _check_optimisers(self, actor_opt, critic_opt, update_actor):
        for opt, mods, who in ((actor_opt, (self.actor_encoder, self.actor_head), "actor"),
                               (critic_opt, (self.critic_encoder, self.critic_head), "critic")):
            if who == "actor" and not update_actor:
                continue
            held = getattr(opt, "modules", None)
            if held is None or len(held) != 2 or held[0] is not mods[0] or held[1] is not mods[1]:
                raise PolicyError("%s_opt must be a DeviceAdam over [%s_encoder, %s_head] of this policy"
                                  % (who, who, who))

    def optimizer_step(self, actor_opt, critic_opt, update_actor: bool = True):
        """The last lines of each half of GR_MAPPO.ppo_update: the gradient norm, clip_grad_norm_ and
        optimizer.step() of both networks in one lsm_optim_step call (lsm.optim, include/lsm_optim.h) on the
        gradients encoders_backward(embed=True) and heads_backward just left: three launches, no host
        synchronisation. actor_opt / critic_opt: DeviceAdam over [actor_encoder, actor_head] /
        [critic_encoder, critic_head]. The blobs are updated in place: the next evaluate_actions / get_actions
        reads the new weights. update_actor=False: the critic's group alone; the actor's weights, moments and
        state are untouched, as with torch's None gradients. Returns {'actor': ..., 'critic': ...}, each
        DeviceAdam.step's dict of 0-dim device views ('actor' None without update_actor)."""
        from . import optim
        self._check_optimisers(actor_opt, critic_opt, update_actor)
        return optim.optimizer_step(actor_opt, critic_opt, update_actor)

    def ppo_update(self, mb, loss, value_norm, actor_opt, critic_opt, data_chunk_length=None,
                   update_actor: bool = True):
        """GR_MAPPO.ppo_update on one minibatch, end to end on the device: ppo_loss, heads_backward(dx=True),
        encoders_backward(embed=True) and optimizer_step, a fixed sequence of launches with no host read
        anywhere. Returns the reference's tuple as a dict of device tensors, valid until the next call:
        value_loss, critic_grad_norm, policy_loss, dist_entropy, actor_grad_norm (0-dim), imp_weights [L*C, 1],
        and skipped = {'actor', 'critic'} (0-dim, 1 where a non-finite gradient left that network untouched).
        Without update_actor the actor's entries (policy_loss, dist_entropy, imp_weights too) are None."""
        self._check_optimisers(actor_opt, critic_opt, update_actor)
        out = self.ppo_loss(mb, loss, value_norm, data_chunk_length, update_actor=update_actor)
        heads = self.heads_backward(mb, out, data_chunk_length, update_actor=update_actor, dx=True)
        self.encoders_backward(mb, heads, update_actor=update_actor, embed=True)
        from . import optim
        st = optim.optimizer_step(actor_opt, critic_opt, update_actor)   # (checked above, before any launch)
        a, c = st["actor"], st["critic"]
        return {"value_loss": out.get("value_loss"), "critic_grad_norm": c["grad_norm"],
                "policy_loss": out.get("policy_loss"), "dist_entropy": out.get("dist_entropy"),
                "actor_grad_norm": a["grad_norm"] if a else None, "imp_weights": out.get("imp_weights"),
                "skipped": {"actor": a["skipped"] if a else None, "critic": c["skipped"]}}
