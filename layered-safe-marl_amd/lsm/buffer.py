"""Device-resident ``GraphReplayBuffer`` rows filled by the rollout with no copies.

Mirrors the env-produced fields of ``onpolicy/utils/graph_buffer.py:84-163`` (share_obs, obs,
node_obs, adj, agent_id, share_agent_id, rewards, masks, bad_masks, active_masks; same shapes and
dtypes, as torch tensors on the env's GPU) and the env-side halves of ``GMPERunner.warmup``
(``graph_mpe_runner.py:253-283``), ``GMPERunner.insert`` (``:444-487``) and
``GraphReplayBuffer.after_update`` (``graph_buffer.py:253-283``).

The rollout kernel writes obs / node_obs / adj into row t+1 and rewards into row t directly: the
env's output slots are ring-bound to the buffer (``lsm_bind_output_ring``), one ring index per
buffer row, so selecting a row is a host-side pointer choice. With a centralized critic
(``use_centralized_V``, the reference default) the kernel also writes that row's share_obs, masks and
active_masks (optional output slots); otherwise ``lsm_buffer_insert`` (HIP) derives them from the
step's obs and dones. agent_id / share_agent_id rows are constant and filled once.

With ``policy_rows`` the buffer also keeps the policy-side fields (``graph_buffer.py:117-151``:
rnn_states, rnn_states_critic, actions, action_log_probs, available_actions): ``insert_step(policy=...)``
writes a step's rows with one ``lsm_buffer_copy_rows`` launch after the step, zeroing the recurrent
states of agents that are done (``graph_mpe_runner.py:449-456``), and ``after_update`` carries row T to
row 0. Without it (the default) those fields stay with the learner.

Between the last env step and the first ppo_update the buffer also does what the reference does with
it (``include/lsm_learner.h``): ``compute_returns`` (``graph_buffer.py:285-366``, ``csrc/lsm_returns.hip``),
``advantages`` (``graph_mappo.py:258-268``) and ``feed_forward_generator`` (``graph_buffer.py:368-453``,
one ``lsm_buffer_gather`` launch per minibatch, ``csrc/lsm_gather.hip``), on ``value_preds`` handed to
``insert_step``. For the reference's default, a recurrent policy, ``recurrent_generator``
(``graph_buffer.py:597-755``) delivers each minibatch of data chunks with one
``lsm_buffer_gather_chunks`` launch (``include/lsm_recurrent.h``, ``csrc/lsm_chunks.hip``). With
``edges=True`` both generators deliver the minibatch as the GNN consumes it: ``adj`` stays in the buffer and
the batch carries ``edge_index`` / ``edge_attr`` (``include/lsm_minibatch_edges.h``, ``csrc/lsm_mb_edges.hip``).
"""
from __future__ import annotations

import ctypes as C

from . import capi


class BufferError(RuntimeError):
    pass


def chunk_rows(chunks, L, T, M):
    """Flat buffer rows (t * M + column) of a recurrent minibatch, in its time-major order: entry
    l * C + b is step l of chunk chunks[b], i.e. sample f = chunks[b] * L + l of the reference's
    (env, agent, t)-ordered view, at row (f % T) * M + f // T. Torch ops on the chunks' device: a learner
    that keeps its own [T, M, ...] tensors indexes them with these rows (the recurrent states with the
    first C of them)."""
    import torch
    f = chunks.reshape(1, -1) * L + torch.arange(L, device=chunks.device, dtype=chunks.dtype).reshape(-1, 1)
    return ((f % T) * M + torch.div(f, T, rounding_mode="floor")).reshape(-1)


class DeviceGraphBuffer:
    def __init__(self, env, episode_length=None, use_centralized_V: bool = True, policy_rows=None):
        import torch
        if env.return_numpy:
            # ring-bound outputs are never written to the env's own tensors: host copies of them
            # would be stale and cost a sync per step
            raise BufferError("DeviceGraphBuffer needs an env built with return_numpy=False")
        self.env = env
        self.lib = capi.load_library()
        self.T = int(episode_length or env.args.episode_length)
        self.centralized = bool(use_centralized_V)
        n, N, E, F, OBS = env.num_envs, env.N, env.E, env.F, env.OBS
        dev = env.device
        f32, i32 = torch.float32, torch.int32
        T1 = self.T + 1
        self.share_obs = torch.zeros((T1, n, N, N * OBS if self.centralized else OBS), dtype=f32, device=dev)
        self.obs = torch.zeros((T1, n, N, OBS), dtype=f32, device=dev)
        self.node_obs = torch.zeros((T1, n, N, E, F), dtype=f32, device=dev)
        if env.t_adj_mask is None:
            self.adj = torch.zeros((T1, n, N, E, E), dtype=f32, device=dev)
            self.adj_mask = None
        else:   # compact layout: one table per env + per-ego masks (expand with vec_env.expand_compact_adj)
            self.adj = torch.zeros((T1, n, E, E), dtype=f32, device=dev)
            self.adj_mask = torch.zeros((T1,) + tuple(env.t_adj_mask.shape), dtype=torch.int64, device=dev)
        self.agent_id = torch.zeros((T1, n, N, 1), dtype=i32, device=dev)
        self.share_agent_id = torch.zeros((T1, n, N, N if self.centralized else 1), dtype=i32, device=dev)
        self.rewards = torch.zeros((self.T, n, N, 1), dtype=f32, device=dev)
        self.masks = torch.ones((T1, n, N, 1), dtype=f32, device=dev)
        self.bad_masks = torch.ones_like(self.masks)
        self.active_masks = torch.ones_like(self.masks)
        # learner-side rows (graph_buffer.py:125-129): the critic's values come in through insert_step,
        # compute_returns fills returns
        self.value_preds = torch.zeros((T1, n, N, 1), dtype=f32, device=dev)
        self.returns = torch.zeros_like(self.value_preds)
        self._adv_ws = None   # advantages(): the partial-sum workspace, allocated on first use
        # policy-side rows (graph_buffer.py:117-151), only when asked for
        self.policy_rows = None
        self.rnn_states = self.rnn_states_critic = self.actions = self.action_log_probs = None
        self.available_actions = None
        if policy_rows is not None:
            pr = dict(recurrent_N=1, act_dim=1, num_actions=None)
            pr.update(policy_rows)
            if set(pr) != {"hidden_size", "recurrent_N", "act_dim", "num_actions"}:
                raise BufferError("policy_rows takes hidden_size, recurrent_N, act_dim and num_actions")
            hid, rn, ad = int(pr["hidden_size"]), int(pr["recurrent_N"]), int(pr["act_dim"])
            if hid < 1 or rn < 1 or ad < 1 or (pr["num_actions"] is not None and int(pr["num_actions"]) < 1):
                raise BufferError("policy_rows sizes must be positive")
            self.policy_rows = pr
            self.rnn_states = torch.zeros((T1, n, N, rn, hid), dtype=f32, device=dev)
            self.rnn_states_critic = torch.zeros_like(self.rnn_states)
            self.actions = torch.zeros((self.T, n, N, ad), dtype=f32, device=dev)
            self.action_log_probs = torch.zeros_like(self.actions)
            if pr["num_actions"] is not None:
                self.available_actions = torch.ones((T1, n, N, int(pr["num_actions"])), dtype=f32, device=dev)
        self.step = 0
        # agent ids are the same every row (the env returns agent index j for agent j)
        ids = torch.arange(N, dtype=i32, device=dev)
        self.agent_id.copy_(ids.view(1, 1, N, 1).expand_as(self.agent_id))
        self.share_agent_id.copy_((ids.view(1, 1, 1, N) if self.centralized else ids.view(1, 1, N, 1))
                                  .expand_as(self.share_agent_id))
        # centralized critic: the rollout kernel also writes share_obs / masks / active_masks rows
        # (LSM_OUT_SHARE_OBS / _MASKS / _ACTIVE_MASKS); otherwise lsm_buffer_insert derives them
        self.fused = self.centralized
        self._bind()
        # per-row kernel arguments, built once (the per-step host path is two ctypes calls)
        self._rows = [tuple(C.c_void_p(t[r].data_ptr()) for t in (self.obs, self.share_obs, self.agent_id,
                                                                  self.share_agent_id, self.masks,
                                                                  self.active_masks))
                      for r in range(T1)]
        self._done_ptr = C.c_void_p(env.t_done.data_ptr())

    # ring index i = buffer row i: obs-like rows at i, rewards at i - 1 (rewards[t] for step t)
    def _bind(self):
        rings = [(capi.OUT_OBS, self.obs, 0), (capi.OUT_NODE_OBS, self.node_obs, 0),
                 (capi.OUT_ADJ, self.adj, 0), (capi.OUT_REWARD, self.rewards, -1)]
        if self.adj_mask is not None:
            rings.append((capi.OUT_ADJ_MASK, self.adj_mask, 0))
        if self.fused:
            rings += [(capi.OUT_SHARE_OBS, self.share_obs, 0), (capi.OUT_MASKS, self.masks, 0),
                      (capi.OUT_ACTIVE_MASKS, self.active_masks, 0)]
        for slot, t, off in rings:
            stride = t[0].numel() * t.element_size()
            capi.check(self.lib.lsm_bind_output_ring(self.env.h, slot, C.c_void_p(t.data_ptr()), stride,
                                                     t.shape[0], off), self.env.h)

    def detach(self):
        """Unbind the rings: the env writes its own output tensors again."""
        for slot in (capi.OUT_OBS, capi.OUT_NODE_OBS, capi.OUT_ADJ, capi.OUT_REWARD, capi.OUT_ADJ_MASK,
                     capi.OUT_SHARE_OBS, capi.OUT_MASKS, capi.OUT_ACTIVE_MASKS):
            capi.check(self.lib.lsm_bind_output_ring(self.env.h, slot, None, 0, 0, 0), self.env.h)
        capi.check(self.lib.lsm_select_ring(self.env.h, -1), self.env.h)

    def _select(self, i):
        capi.check(self.lib.lsm_select_ring(self.env.h, int(i)), self.env.h)

    def _insert(self, row, with_dones):
        env = self.env
        o, so, aid, said, m, am = self._rows[row]
        rc = self.lib.lsm_buffer_insert(o, self._done_ptr if with_dones else None, env.num_envs, env.N, env.OBS,
                                        int(self.centralized), so, aid, said, m, am, env._stream())
        if rc != 0:
            raise BufferError(self.lib.lsm_buffer_last_error().decode())

    def warmup(self, num_current_episode: int = 0):
        """GMPERunner.warmup (graph_mpe_runner.py:253-283): reset into row 0. Returns ep_info."""
        self._select(0)
        ep = self.env.reset(num_current_episode)[-1]
        if not self.fused:
            self._insert(0, False)
        self.step = 0
        return ep

    def insert_step(self, actions, num_current_episode=None, value_preds=None, policy=None):
        """env.step + GMPERunner.insert's env-side rows for buffer step t = self.step: obs,
        node_obs, adj, share_obs, agent_id, share_agent_id, masks, active_masks at t+1 and
        rewards at t. value_preds (the critic's values for step t, n * N floats), when given, is
        copied into value_preds[t] first.

        policy (needs policy_rows): a mapping of device tensors actions, action_log_probs, rnn_states,
        rnn_states_critic and, with num_actions, optionally available_actions, shaped as one buffer
        row. They are written by one lsm_buffer_copy_rows launch after the step (GMPERunner.insert +
        GraphReplayBuffer.insert, graph_mpe_runner.py:444-487, graph_buffer.py:229-249): actions,
        action_log_probs (and value_preds) into row t, the recurrent states, zeroed where the step's
        dones are set, and available_actions into row t+1.

        Returns (dones [n, N] u8, (info, reset_flag, ep_info)) device tensors."""
        t = self.step
        copies = self._policy_copies(t, policy, value_preds) if policy is not None else None
        if value_preds is not None and copies is None:
            self.value_preds[t].copy_(self._as_f32(value_preds).reshape(self.value_preds[t].shape))
        self._select(t + 1)
        self.env.step_async(actions, num_current_episode)
        self.env.step_wait()
        if not self.fused:
            self._insert(t + 1, True)
        if copies is not None:
            arr, keep = copies   # keep: the sources stay referenced until the launch is queued
            rc = self.lib.lsm_buffer_copy_rows(arr, len(arr), self._done_ptr, self.env.num_envs * self.env.N,
                                               self.env._stream())
            if rc != 0:
                raise BufferError(self.lib.lsm_recurrent_last_error().decode())
        self.step = (t + 1) % self.T
        return self.env.t_done, (self.env.t_info, self.env.t_reset, self.env.t_epinfo)

    def _policy_copies(self, t, policy, value_preds):
        """The lsm_row_copy descriptors of step t's policy-side rows (and value_preds when given)."""
        if self.policy_rows is None:
            raise BufferError("insert_step(policy=...) needs a buffer built with policy_rows")
        names = {"actions", "action_log_probs", "rnn_states", "rnn_states_critic", "available_actions"}
        if set(policy) - names:
            raise BufferError("unknown policy fields: %s" % sorted(set(policy) - names))
        if names - {"available_actions"} - set(policy):
            raise BufferError("missing policy fields: %s" % sorted(names - {"available_actions"} - set(policy)))
        # (source, buffer row, zero where done)
        plan = [(policy["actions"], self.actions[t], 0), (policy["action_log_probs"], self.action_log_probs[t], 0),
                (policy["rnn_states"], self.rnn_states[t + 1], 1),
                (policy["rnn_states_critic"], self.rnn_states_critic[t + 1], 1)]
        if policy.get("available_actions") is not None:
            if self.available_actions is None:
                raise BufferError("available_actions given to a buffer built without num_actions")
            plan.append((policy["available_actions"], self.available_actions[t + 1], 0))
        if value_preds is not None:
            plan.append((value_preds, self.value_preds[t], 0))
        M = self.env.num_envs * self.env.N
        arr = (capi.LsmRowCopy * len(plan))()
        keep = []
        for c, (src, dst, zero) in zip(arr, plan):
            s = self._as_f32(src).contiguous()
            if s.numel() != dst.numel():
                raise BufferError("a policy tensor has %d elements, its buffer row %d" % (s.numel(), dst.numel()))
            keep.append(s)
            c.src, c.dst, c.row_bytes, c.zero_on_done = s.data_ptr(), dst.data_ptr(), dst.numel() // M * 4, zero
        return arr, keep

    def after_update(self):
        """GraphReplayBuffer.after_update (graph_buffer.py:253-283)."""
        fields = [self.share_obs, self.obs, self.node_obs, self.adj, self.agent_id, self.share_agent_id,
                  self.masks, self.active_masks, self.bad_masks]
        if self.adj_mask is not None:
            fields.append(self.adj_mask)
        if self.policy_rows is not None:
            fields += [self.rnn_states, self.rnn_states_critic]
            if self.available_actions is not None:
                fields.append(self.available_actions)
        for f in fields:
            f[0].copy_(f[-1])

    # ---- learner hand-off (include/lsm_learner.h) ------------------------------------------------

    def _as_f32(self, x):
        import torch
        return torch.as_tensor(x, dtype=torch.float32, device=self.env.device)

    def _denorm(self, value_normalizer):
        """The kernels' device float32 [2] = {sqrt(var), mean}, or None. From a normaliser object it is
        built with torch ops and no .item(): on the env's stream with no synchronisation when its
        tensors are on the env's device. CPU tensors, and a (scale, mean) pair of Python numbers, go
        through a host-to-device copy, which blocks the host; a device [2] tensor is used as it is."""
        import torch
        vn = value_normalizer
        if vn is None:
            return None
        if hasattr(vn, "running_mean_var"):
            mean, var = vn.running_mean_var()
            if mean.numel() != 1 or var.numel() != 1:
                raise BufferError("value_normalizer.running_mean_var() must return 1-element tensors")
            d = torch.stack([torch.sqrt(var.detach()).reshape(()), mean.detach().reshape(())])
            return d.to(device=self.env.device, dtype=torch.float32).contiguous()
        if isinstance(vn, torch.Tensor):
            if vn.shape != (2,) or vn.dtype != torch.float32 or vn.device != self.env.device:
                raise BufferError("a denorm tensor must be float32 [2] = (scale, mean) on the env's device")
            return vn.contiguous()
        scale, mean = vn
        return torch.tensor([float(scale), float(mean)], dtype=torch.float32, device=self.env.device)

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    def compute_returns(self, next_value, value_normalizer=None, *, gamma, gae_lambda, use_gae=True,
                        use_proper_time_limits=False):
        """GraphReplayBuffer.compute_returns (graph_buffer.py:285-366) on the device, bit for bit: fills
        returns[0..T-1] (and value_preds[T] with use_gae, returns[T] without) from rewards, value_preds,
        masks and bad_masks. value_normalizer: None, an object with running_mean_var() (ValueNorm,
        PopArt), a (scale, mean) pair or a device float32 [2] tensor. Stream-ordered. The call itself never
        synchronises; a normaliser or next_value that lives on the host costs a blocking upload (_denorm)."""
        env = self.env
        nv = self._as_f32(next_value).reshape(env.num_envs * env.N).contiguous()
        den = self._denorm(value_normalizer)
        cfg = capi.LsmReturnsConfig(gamma=float(gamma), gae_lambda=float(gae_lambda), use_gae=int(bool(use_gae)),
                                    use_proper_time_limits=int(bool(use_proper_time_limits)))
        p = self._ptr
        rc = self.lib.lsm_buffer_compute_returns(p(self.rewards), p(self.value_preds), p(self.masks), p(self.bad_masks),
                                                 p(nv), p(den), p(self.returns), self.T, env.num_envs * env.N,
                                                 C.byref(cfg), env._stream())
        if rc != 0:
            raise BufferError(self.lib.lsm_returns_last_error().decode())

    def advantages(self, value_normalizer=None):
        """The head of GR_MAPPO.train (graph_mappo.py:258-268): returns[:-1] - denormalize(value_preds[:-1]),
        normalised by the mean and std over entries whose active_masks is non-zero. Returns (advantages
        [T, n, N, 1] float32, stats float64 [3] = mean, std, active count), device tensors; the
        statistics are float64 sums in a fixed order. Stream-ordered; no synchronisation with a device
        normaliser (see _denorm for host-side ones)."""
        import torch
        env = self.env
        count = self.T * env.num_envs * env.N
        if self._adv_ws is None:
            nbytes = int(self.lib.lsm_buffer_advantages_workspace_bytes(count))
            self._adv_ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=env.device)
        ws = self._adv_ws
        adv = torch.empty((self.T, env.num_envs, env.N, 1), dtype=torch.float32, device=env.device)
        stats = torch.empty(3, dtype=torch.float64, device=env.device)
        den = self._denorm(value_normalizer)
        p = self._ptr
        rc = self.lib.lsm_buffer_advantages(p(self.returns), p(self.value_preds), p(self.active_masks), p(den), count,
                                            p(adv), p(stats), p(ws), ws.numel() * 8, env._stream())
        if rc != 0:
            raise BufferError(self.lib.lsm_returns_last_error().decode())
        return adv, stats

    def _gather_sources(self, advantages):
        """(name, source tensor over rows [0, T) viewed per sample, per-sample shape), in yield order."""
        E = self.env.E
        adj_shape = (E, E)
        src = [("share_obs", self.share_obs), ("obs", self.obs), ("node_obs", self.node_obs), ("adj", self.adj),
               ("agent_id", self.agent_id), ("share_agent_id", self.share_agent_id),
               ("value_preds", self.value_preds), ("returns", self.returns), ("masks", self.masks),
               ("active_masks", self.active_masks), ("advantages", advantages)]
        return [(k, t, adj_shape if k == "adj" else tuple(t.shape[3:])) for k, t in src]

    def feed_forward_generator(self, advantages, num_mini_batch=None, mini_batch_size=None, indices=None,
                               generator=None, edges=False):
        """GraphReplayBuffer.feed_forward_generator (graph_buffer.py:368-453) for the buffer's fields:
        yields, per minibatch, a dict of device tensors share_obs, obs, node_obs, adj, agent_id,
        share_agent_id, value_preds, returns, masks, active_masks, advantages (each [B, ...], row b the
        sample indices[b] of the field's [:-1].reshape(T * n * N, ...) view) and indices, all gathered by
        one lsm_buffer_gather launch. adj is always the reference's [B, E, E] matrix; a compact buffer
        expands it from its table and masks in the same launch. indices: an int64 permutation of the
        T * n * N samples (validated once, which synchronises); by default torch.randperm on the device
        (generator: its torch.Generator). The learner gathers its own policy-side tensors (actions,
        log-probs, rnn states) with the yielded indices.

        edges=True: the minibatch comes as the GNN consumes it (GNNBase.forward, gnn.py:545-564, keeps
        only process_adj's result). adj is left out of the gather launch and yielded as None, and the
        batch ends with edge_index int64 [2, nnz] and edge_attr float32 [nnz, 1], process_adj of the
        minibatch's [B, E, E] adjacency, made from the buffer's own adjacency in either layout by
        lsm.edges.minibatch_edges (which synchronises once, like torch.nonzero); they are fresh tensors.

        The output tensors are allocated once per generator and reused: a yielded batch is valid until
        the next one is requested."""
        import torch
        env = self.env
        dev = env.device
        n, N = env.num_envs, env.N
        batch_size = n * self.T * N
        if mini_batch_size is None:
            # the reference's rule (an assert there too): at least one sample per minibatch
            assert num_mini_batch is not None and batch_size >= num_mini_batch, (
                "%d minibatches asked of %d samples (%d envs x %d steps x %d agents)"
                % (num_mini_batch or 0, batch_size, n, self.T, N))
            mini_batch_size = batch_size // num_mini_batch
        mb = int(mini_batch_size)
        if mb < 1:
            raise BufferError("mini_batch_size < 1")
        if num_mini_batch is None:
            num_mini_batch = batch_size // mb
        if mb * num_mini_batch > batch_size:
            raise BufferError("mini_batch_size * num_mini_batch exceeds the %d samples" % batch_size)
        if indices is None:
            perm = torch.randperm(batch_size, device=dev, generator=generator)
        else:
            perm = torch.as_tensor(indices, device=dev)
            if perm.dtype != torch.int64 or perm.shape != (batch_size,):
                raise BufferError("indices must be an int64 permutation of the %d samples" % batch_size)
            perm = perm.contiguous()
            if not torch.equal(torch.sort(perm).values, torch.arange(batch_size, device=dev)):
                raise BufferError("indices is not a permutation of range(%d)" % batch_size)
        plan = self._gather_plan(advantages, mb, edges)
        for i in range(num_mini_batch):
            yield self._gather(plan, perm[i * mb:(i + 1) * mb])

    def _gather_plan(self, advantages, mb, edges=False):
        """The field descriptors and the output tensors of minibatches of mb samples, built once."""
        import torch
        env = self.env
        dev = env.device
        batch_size = env.num_envs * self.T * env.N
        adv = torch.as_tensor(advantages, device=dev)
        if adv.dtype != torch.float32 or adv.numel() != batch_size:
            raise BufferError("advantages must be float32 with T * n * N entries")
        adv = adv.reshape(self.T, env.num_envs, env.N, 1).contiguous()
        sources = self._gather_sources(adv)
        names = [k for k, _, _ in sources]
        if edges:   # adj stays in the buffer: _minibatch_edges reads it there
            sources = [s for s in sources if s[0] != "adj"]
        out = {k: torch.empty((mb,) + shape, dtype=t.dtype, device=dev) for k, t, shape in sources}
        fields = (capi.LsmGatherField * len(sources))()
        for f, (k, t, shape) in zip(fields, sources):
            f.src, f.dst = t.data_ptr(), out[k].data_ptr()
            if k == "adj" and self.adj_mask is not None:
                f.kind, f.masks, f.E, f.N = capi.LSM_GATHER_COMPACT_ADJ, self.adj_mask.data_ptr(), env.E, env.N
            else:
                f.kind, f.row_bytes = capi.LSM_GATHER_ROWS, out[k][0].numel() * t.element_size()
        return fields, out, adv, batch_size, names, bool(edges)

    def _gather(self, plan, idx):
        """One minibatch: every field's rows idx (a contiguous int64 device tensor) in one launch."""
        fields, out, _, batch_size, names, edges = plan   # the plan keeps the advantages tensor alive
        rc = self.lib.lsm_buffer_gather(fields, len(fields), C.c_void_p(idx.data_ptr()), idx.numel(), batch_size, None,
                                        self.env._stream())
        if rc != 0:
            raise BufferError(self.lib.lsm_gather_last_error().decode())
        batch = {k: out.get(k) for k in names}
        batch["indices"] = idx
        if edges:
            batch["edge_index"], batch["edge_attr"] = self._minibatch_edges(idx, None)
        return batch

    def _minibatch_edges(self, ids, chunks):
        """process_adj of the minibatch named by ids, from rows [0, T) of the buffer's adjacency."""
        from . import edges as lsm_edges
        masks = self.adj_mask[:self.T] if self.adj_mask is not None else None
        return lsm_edges.minibatch_edges(self.adj[:self.T], masks, self.env.N, ids, chunks=chunks)

    # ---- recurrent policy (include/lsm_recurrent.h) ----------------------------------------------

    def _chunk_sources(self, advantages):
        """(name, source tensor, per-sample shape), in the reference's yield order
        (graph_buffer.py:751-755); the policy-side fields only with policy_rows."""
        E = self.env.E
        src = [("share_obs", self.share_obs), ("obs", self.obs), ("node_obs", self.node_obs), ("adj", self.adj),
               ("agent_id", self.agent_id), ("share_agent_id", self.share_agent_id),
               ("rnn_states", self.rnn_states), ("rnn_states_critic", self.rnn_states_critic),
               ("actions", self.actions), ("value_preds", self.value_preds), ("returns", self.returns),
               ("masks", self.masks), ("active_masks", self.active_masks),
               ("action_log_probs", self.action_log_probs), ("advantages", advantages),
               ("available_actions", self.available_actions)]
        return [(k, t, (E, E) if k == "adj" else tuple(t.shape[3:])) for k, t in src if t is not None]

    def recurrent_generator(self, advantages, num_mini_batch, data_chunk_length, chunks=None, generator=None,
                            edges=False):
        """GraphReplayBuffer.recurrent_generator (graph_buffer.py:597-755): the T * n * N samples, ordered
        (env, agent, t), are cut into data_chunks = T * n * N // data_chunk_length chunks of L consecutive
        samples (the tail is dropped; when L does not divide T a chunk runs into the next agent's series,
        as in the reference), and each minibatch takes C = data_chunks // num_mini_batch of them. Yields,
        per minibatch, a dict of device tensors under the reference's names and in its order: share_obs,
        obs, node_obs, adj, agent_id, share_agent_id, rnn_states, rnn_states_critic, actions, value_preds,
        returns, masks, active_masks, action_log_probs, advantages, available_actions (None without
        num_actions), and chunks. Each is [L * C, ...], row l * C + b step l of chunk chunks[b]; the two
        recurrent states are [C, recurrent_N, hidden], taken at each chunk's first step. All of it is
        gathered by one lsm_buffer_gather_chunks launch; adj is always the reference's [L * C, E, E]
        matrix, which a compact buffer expands in the same launch. A buffer without policy_rows leaves
        the five policy-side fields out: the learner indexes its own tensors with chunk_rows().

        chunks: an int64 permutation of range(data_chunks) (validated once, which synchronises); by
        default torch.randperm on the device (generator: its torch.Generator).

        edges=True: as in feed_forward_generator -- adj is left out of the gather launch and yielded as
        None, and the batch ends with edge_index / edge_attr, process_adj of the minibatch's
        [L * C, E, E] adjacency (graph l * C + b is step l of chunk chunks[b]), fresh tensors made from
        the buffer's own adjacency by lsm.edges.minibatch_edges.

        The output tensors are allocated once per generator and reused: a yielded batch is valid until
        the next one is requested."""
        import torch
        env = self.env
        dev = env.device
        L = int(data_chunk_length)
        batch_size = env.num_envs * self.T * env.N
        if L < 1 or L > batch_size:
            raise BufferError("data_chunk_length outside 1..%d" % batch_size)
        data_chunks = batch_size // L
        mb = data_chunks // int(num_mini_batch)
        if mb < 1:
            raise BufferError("%d minibatches asked of %d chunks" % (num_mini_batch, data_chunks))
        if chunks is None:
            perm = torch.randperm(data_chunks, device=dev, generator=generator)
        else:
            perm = torch.as_tensor(chunks, device=dev)
            if perm.dtype != torch.int64 or perm.shape != (data_chunks,):
                raise BufferError("chunks must be an int64 permutation of the %d chunks" % data_chunks)
            perm = perm.contiguous()
            if not torch.equal(torch.sort(perm).values, torch.arange(data_chunks, device=dev)):
                raise BufferError("chunks is not a permutation of range(%d)" % data_chunks)
        plan = self._chunk_plan(advantages, mb, L, edges)
        for i in range(int(num_mini_batch)):
            yield self._gather_chunks(plan, perm[i * mb:(i + 1) * mb])

    def _chunk_plan(self, advantages, mb, L, edges=False):
        """The field descriptors and the output tensors of minibatches of mb chunks of L steps, built once."""
        import torch
        env = self.env
        dev = env.device
        batch_size = env.num_envs * self.T * env.N
        adv = torch.as_tensor(advantages, device=dev)
        if adv.dtype != torch.float32 or adv.numel() != batch_size:
            raise BufferError("advantages must be float32 with T * n * N entries")
        adv = adv.reshape(self.T, env.num_envs, env.N, 1).contiguous()
        sources = self._chunk_sources(adv)
        names = [k for k, _, _ in sources]
        if edges:   # adj stays in the buffer: _minibatch_edges reads it there
            sources = [s for s in sources if s[0] != "adj"]
        first = ("rnn_states", "rnn_states_critic")
        out = {k: torch.empty(((mb if k in first else L * mb),) + shape, dtype=t.dtype, device=dev)
               for k, t, shape in sources}
        fields = (capi.LsmChunkField * len(sources))()
        for f, (k, t, shape) in zip(fields, sources):
            f.src, f.dst = t.data_ptr(), out[k].data_ptr()
            if k == "adj" and self.adj_mask is not None:
                f.kind, f.masks, f.E, f.N = capi.LSM_CHUNK_COMPACT_ADJ, self.adj_mask.data_ptr(), env.E, env.N
            else:
                f.kind = capi.LSM_CHUNK_FIRST_ROW if k in first else capi.LSM_CHUNK_ROWS
                f.row_bytes = out[k][0].numel() * t.element_size()
        if self.policy_rows is not None and self.available_actions is None:
            names.append("available_actions")   # the reference yields None for a non-discrete action space
        return fields, out, adv, names, L, bool(edges)

    def _gather_chunks(self, plan, idx):
        """One minibatch: every field's chunks idx (a contiguous int64 device tensor) in one launch."""
        fields, out, _, names, L, edges = plan   # the plan keeps the advantages tensor alive
        env = self.env
        rc = self.lib.lsm_buffer_gather_chunks(fields, len(fields), C.c_void_p(idx.data_ptr()), idx.numel(), L, self.T,
                                               env.num_envs * env.N, None, env._stream())
        if rc != 0:
            raise BufferError(self.lib.lsm_recurrent_last_error().decode())
        batch = {k: out.get(k) for k in names}
        batch["chunks"] = idx
        if edges:
            batch["edge_index"], batch["edge_attr"] = self._minibatch_edges(idx, (L, self.T, env.num_envs * env.N))
        return batch
