"""The reference's graph encoder, ``GNNBase.forward`` (``onpolicy/algorithms/utils/gnn.py:545-564``), as
one kernel launch on the step's own outputs (``csrc/lsm_gnn.hip`` through ``include/lsm_gnn.h``).

``GraphEncoder.forward(node_obs, adj, agent_id)`` takes what ``GNNBase.forward`` takes (CUDA float32
``[B, E, F]`` / ``[B, E, E]``, ``agent_id`` ``[B, 1]`` or ``[B]``) and returns its ``[B, out_dim]`` row per
graph; ``forward_compact`` reads the compact adjacency layout (one ``[n, E, E]`` table + per-ego
disconnect words) without expanding it. No edge list, no per-edge tensor and no host synchronisation:
``process_adj`` is not called. There is no CPU fallback, as elsewhere in the project.

``GraphEncoder.backward(node_obs, adj, dout, agent_id)`` (``csrc/lsm_gnn_backward.hip`` through
``include/lsm_gnn_backward.h`` and, beyond its LDS limit, ``include/lsm_gnn_backward_large.h``) is the backward pass through the readout and the TransformerConv layers: from
the gradient at ``forward``'s output to the gradient of every conv-layer weight and to ``dh0``, the gradient at
EmbedConv's output. ``GraphEncoder.embed_backward(node_obs, adj, dh0)`` (``csrc/lsm_gnn_embed_backward.hip`` through
``include/lsm_gnn_embed_backward.h``) is EmbedConv's own backward, from ``dh0`` to the gradient of the blob's
EmbedConv entries; ``backward(..., embed=True)`` runs both and leaves a complete gradient in ``dweights``.

Weights travel as one packed float32 blob (layout: ``include/lsm_gnn.h``). ``pack_weights`` builds it from
a ``GNNBase`` state dict, checking every shape against the config; ``GraphEncoder.load`` refreshes the
device copy after an optimiser step.

``embed_add_self_loop`` has no effect in the reference (``EmbedConv.forward`` adds self loops only when
``edge_attr is None``, which ``GNNBase`` never passes: gnn.py:112), so ``GnnConfig`` has no such field.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import capi
from ._device import DeviceOp, OutputCache, _torch, pack_entries, ptr, unpack_entries

AGGR = {"node": capi.LSM_GNN_NODE, "global_mean": capi.LSM_GNN_GLOBAL_MEAN, "global_max": capi.LSM_GNN_GLOBAL_MAX,
        "global_add": capi.LSM_GNN_GLOBAL_ADD}


class GnnError(RuntimeError):
    pass


@dataclass(frozen=True)
class GnnConfig:
    """The network's shape: the fields of ``lsm_gnn_config``. ``aggr``: 'node', 'global_mean',
    'global_max' or 'global_add'. The defaults are the reference's (onpolicy/config.py:400-446)."""
    F: int
    num_embeddings: int = 4
    embedding_size: int = 2
    embed_hidden: int = 16
    embed_layer_N: int = 1
    embed_relu: bool = True
    layer_norm: bool = True
    C: int = 16
    H: int = 3
    concat: bool = False
    layer_N: int = 2
    relu: bool = True
    aggr: str = "node"
    ego_only: bool = False   # timing knob of the last layer (include/lsm_gnn.h); same output

    @classmethod
    def from_args(cls, all_args, node_obs_dim: int, graph_aggr: str) -> "GnnConfig":
        """From the reference's argument names; graph_aggr is GNNBase's 'node' or 'global' (the latter
        with all_args.global_aggr_type)."""
        if graph_aggr == "node":
            aggr = "node"
        elif graph_aggr == "global":
            aggr = "global_%s" % all_args.global_aggr_type
        else:
            raise ValueError("graph_aggr must be 'node' or 'global', got %r" % (graph_aggr,))
        return cls(F=int(node_obs_dim), num_embeddings=int(all_args.num_embeddings),
                   embedding_size=int(all_args.embedding_size), embed_hidden=int(all_args.embed_hidden_size),
                   embed_layer_N=int(all_args.embed_layer_N), embed_relu=bool(all_args.embed_use_ReLU),
                   layer_norm=bool(all_args.use_feature_normalization), C=int(all_args.gnn_hidden_size),
                   H=int(all_args.gnn_num_heads), concat=bool(all_args.gnn_concat_heads),
                   layer_N=int(all_args.gnn_layer_N), relu=bool(all_args.gnn_use_ReLU), aggr=aggr)

    @property
    def out_dim(self) -> int:
        return self.C * (self.H if self.concat else 1)

    def struct(self) -> capi.LsmGnnConfig:
        if self.aggr not in AGGR:
            raise ValueError("aggr must be one of %s, got %r" % (sorted(AGGR), self.aggr))
        return capi.LsmGnnConfig(F=self.F, num_embeddings=self.num_embeddings, embedding_size=self.embedding_size,
                                 embed_hidden=self.embed_hidden, embed_layer_N=self.embed_layer_N,
                                 embed_relu=int(self.embed_relu), layer_norm=int(self.layer_norm), C=self.C, H=self.H,
                                 concat=int(self.concat), layer_N=self.layer_N, relu=int(self.relu),
                                 aggr=AGGR[self.aggr], ego_only=int(self.ego_only))


def weight_entries(cfg: GnnConfig):
    """[(state-dict name without prefix, shape)] in the blob's order (include/lsm_gnn.h)."""
    Hd, HC, D = cfg.embed_hidden, cfg.H * cfg.C, cfg.out_dim
    K = cfg.F - 1 + cfg.embedding_size + 1
    out = [("embed_layer.entity_embed.weight", (cfg.num_embeddings, cfg.embedding_size)),
           ("embed_layer.lin1.weight", (Hd, K)), ("embed_layer.lin1.bias", (Hd,)),
           ("embed_layer.layer_norm.weight", (Hd,)), ("embed_layer.layer_norm.bias", (Hd,))]
    for k in range(cfg.embed_layer_N):
        out += [("embed_layer.layers.%d.weight" % (3 * k), (Hd, Hd)), ("embed_layer.layers.%d.bias" % (3 * k), (Hd,))]
    for l in range(cfg.layer_N + 1):
        conv = "gnn1" if l == 0 else "gnn2.%d" % (l - 1)
        din = Hd if l == 0 else D
        for lin in ("query", "key", "value"):
            out += [("%s.lin_%s.weight" % (conv, lin), (HC, din)), ("%s.lin_%s.bias" % (conv, lin), (HC,))]
        out += [("%s.lin_edge.weight" % conv, (HC, 1)),
                ("%s.lin_skip.weight" % conv, (D, din)), ("%s.lin_skip.bias" % conv, (D,))]
    return out


def weights_floats(cfg: GnnConfig) -> int:
    """lsm_gnn_weights_floats(cfg); raises for a config the library refuses."""
    lib = capi.load_library()
    n = int(lib.lsm_gnn_weights_floats(cfg.struct()))
    if n == 0:
        raise GnnError(lib.lsm_gnn_last_error().decode())
    return n


def pack_weights(state_dict, cfg: GnnConfig, prefix: str = "gnn.") -> np.ndarray:
    """The packed float32 blob of a GNNBase state dict (tensors or arrays). Every entry's shape is
    checked against cfg; a missing or mis-shaped one is refused by name. Without layer norm the state
    dict has no layer_norm entries (nn.Identity) and the blob's unread gamma / beta are 1 / 0."""
    return pack_entries(state_dict, weight_entries(cfg), prefix, None if cfg.layer_norm else ".layer_norm.",
                        lambda: weights_floats(cfg), GnnError, "pack_weights")


def unpack_weights(blob, cfg: GnnConfig, prefix: str = "gnn."):
    """The inverse of pack_weights: {name: float32 array} (layer_norm entries only with layer norm)."""
    return unpack_entries(blob, weight_entries(cfg), prefix, None if cfg.layer_norm else ".layer_norm.",
                          lambda: weights_floats(cfg), GnnError, "unpack_weights")


class GraphEncoder(DeviceOp):
    """GNNBase.forward on the GPU for one config and one weight blob.

    The output tensor is preallocated per (B, stream) and is valid until the next call with that B on
    that stream. check=True reads the call's bad-input word (one synchronisation) and raises when an
    entity type or an agent_id was out of range; by default the word is not read."""

    def __init__(self, cfg: GnnConfig, weights, device):
        self.cfg = cfg
        super().__init__(device, GnnError, "GraphEncoder", "encoder")
        self._struct = cfg.struct()
        self._out = OutputCache()
        self._bwd_out = OutputCache()
        self._emb_out = OutputCache()
        self._last_dweights = None
        self._last_embed = False   # whether the last backward() ran with embed=True (lsm.optim.DeviceAdam asks)
        self._alloc_weights(weights_floats(cfg), weights)

    def load(self, state_dict, prefix: str = "gnn."):
        """Refresh the blob from a GNNBase state dict (after each optimiser step)."""
        self._set(pack_weights(state_dict, self.cfg, prefix))

    def state_dict(self, prefix: str = "gnn."):
        """The current device blob as {name: float32 tensor}, the inverse of load (unpack_weights; one
        download): a checkpoint after lsm.optim.DeviceAdam's steps needs no torch module."""
        torch = _torch()
        return {k: torch.from_numpy(v) for k, v in unpack_weights(self.weights.cpu().numpy(), self.cfg, prefix).items()}

    def _agent_id(self, agent_id, B):
        """agent_id as the library reads it ([B] int64, contiguous); None for the global readouts."""
        torch = _torch()
        if self.cfg.aggr != "node":
            return None
        if agent_id is None:
            raise GnnError("the 'node' readout needs agent_id")
        if not isinstance(agent_id, torch.Tensor) or not agent_id.is_cuda:
            raise GnnError("agent_id must be a CUDA (HIP) tensor; there is no CPU fallback")
        if agent_id.numel() != B:
            raise GnnError("agent_id must be [B] or [B, 1], got %s" % (tuple(agent_id.shape),))
        aid = agent_id.reshape(B)
        if aid.dtype != torch.int64:
            aid = aid.long()   # GNNBase.forward: agent_id.long()
        return aid.contiguous()

    def _run(self, node_obs, adj, masks, B, E, N, agent_id, check):
        torch = _torch()
        cfg = self.cfg
        node_obs = self._tensor(node_obs, "node_obs", shape=(B, E, cfg.F))
        aid = self._agent_id(agent_id, B)
        sh = self._stream()
        out = self._out.get((B, sh), lambda: torch.empty((B, cfg.out_dim), dtype=torch.float32, device=self.device))
        rc = self.lib.lsm_gnn_forward(self._struct, C.c_void_p(self.weights.data_ptr()),
                                      C.c_void_p(node_obs.data_ptr()), C.c_void_p(adj.data_ptr()),
                                      C.c_void_p(masks.data_ptr()) if masks is not None else None, B, E, N,
                                      C.c_void_p(aid.data_ptr()) if aid is not None else None,
                                      C.c_void_p(out.data_ptr()), C.c_void_p(self.bad.data_ptr()), C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_gnn_last_error, check,
                     "an entity type outside [0, num_embeddings) or an agent_id outside [0, E) reached the encoder")
        return out

    def forward(self, node_obs, adj, agent_id=None, check: bool = False):
        """node_obs [B, E, F], adj [B, E, E] (the reference layout), agent_id [B, 1] or [B]."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        adj = self._tensor(adj, "adj", shape=(B, E, E))
        return self._run(node_obs, adj, None, B, E, 1, agent_id, check)

    def forward_compact(self, node_obs, table, masks, num_agents: int, agent_id=None, check: bool = False):
        """The compact layout: table [n, E, E], masks [n, N, W] (or [n * N, W]) int64 disconnect words,
        node_obs [n * N, E, F]; graph b = env * N + ego."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        N = int(num_agents)
        if N < 1 or B % N:
            raise GnnError("node_obs holds %d graphs, not a multiple of num_agents = %d" % (B, N))
        table = self._tensor(table, "table", shape=(B // N, E, E))
        if not isinstance(masks, torch.Tensor) or masks.numel() != B * ((E + 63) // 64):
            raise GnnError("masks must hold [n * N, ceil(E / 64)] words")
        masks = self._tensor(masks.reshape(B, (E + 63) // 64), "masks", dtype=torch.int64, shape=(B, (E + 63) // 64))
        return self._run(node_obs, table, masks, B, E, N, agent_id, check)

    def forward_step(self, node_obs, adj, adj_mask, num_agents: int, agent_id=None, check: bool = False):
        """One step's graphs as a GpuGraphVecEnv or a DeviceGraphBuffer row holds them, in either adjacency
        layout: node_obs [n, N, E, F]; adj [n, N, E, E] with adj_mask None (the reference layout), or the
        table [n, E, E] with adj_mask [n, N, W] (the compact layout). Returns [n * N, out_dim]."""
        E, F = int(node_obs.shape[-2]), int(node_obs.shape[-1])
        node = node_obs.reshape(-1, E, F)
        aid = None if agent_id is None else agent_id.reshape(-1)
        if adj_mask is None:
            return self.forward(node, adj.reshape(-1, E, E), aid, check=check)
        return self.forward_compact(node, adj, adj_mask, num_agents, aid, check=check)

    __call__ = forward

    # ---- the backward pass: readout and conv layers (include/lsm_gnn_backward.h) ---------------------------------

    def _bwd_outputs(self, B, E):
        torch = _torch()
        n = int(self.lib.lsm_gnn_backward_workspace_bytes(self._struct, B, E))
        # a size lsm_gnn_backward refuses (a graph beyond its LDS limit, or one nothing accepts) goes to the spilled
        # tier, whose workspace also holds the scratch
        large = n == 0 and B > 0
        if large:
            n = int(self.lib.lsm_gnn_backward_large_workspace_bytes(self._struct, B, E, 0))
            if n == 0:
                raise GnnError(self.lib.lsm_gnn_backward_large_last_error().decode())
        f32 = dict(dtype=torch.float32, device=self.device)
        return {"dweights": torch.zeros(self._n, **f32), "dh0": torch.empty((B, E, self.cfg.embed_hidden), **f32),
                "workspace": torch.empty((n + 7) // 8 or 1, dtype=torch.float64, device=self.device), "large": large}

    def _run_backward(self, node_obs, adj, masks, B, E, N, dout, agent_id, dh0, check, embed=False):
        cfg = self.cfg
        node_obs = self._tensor(node_obs, "node_obs", shape=(B, E, cfg.F))
        dout = self._tensor(dout, "dout", shape=(B, cfg.out_dim), detach=True)
        aid = self._agent_id(agent_id, B)
        sh = self._stream()
        out = self._bwd_out.get((B, E, sh), lambda: self._bwd_outputs(B, E))
        io = capi.LsmGnnBwdIo(node_obs=ptr(node_obs), adj=ptr(adj), masks=ptr(masks), agent_id=ptr(aid), dout=ptr(dout),
                              dweights=ptr(out["dweights"]), dh0=ptr(out["dh0"]) if dh0 or embed else None,
                              workspace=ptr(out["workspace"]), bad=ptr(self.bad))
        if out["large"]:
            rc = self.lib.lsm_gnn_backward_large(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), B, E, N,
                                                 0, C.c_void_p(sh))
            last_error = self.lib.lsm_gnn_backward_large_last_error
        else:
            rc = self.lib.lsm_gnn_backward(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), B, E, N,
                                           C.c_void_p(sh))
            last_error = self.lib.lsm_gnn_backward_last_error
        self._finish(rc, last_error, check,
                     "an entity type outside [0, num_embeddings) or an agent_id outside [0, E) reached the encoder")
        self._last_dweights, self._last_embed = out["dweights"], False
        if embed:   # the same stream: seeded by this call's dh0, into the EmbedConv range of the same dweights
            self._run_embed_backward(node_obs, adj, masks, B, E, N, out["dh0"], out["dweights"], check)
            self._last_embed = True   # only once the embed call went through: the range holds a gradient
        return {"dweights": out["dweights"], "dh0": out["dh0"] if dh0 else None}

    def backward(self, node_obs, adj, dout, agent_id=None, dh0: bool = False, check: bool = False,
                 embed: bool = False):
        """The backward pass through the readout and the conv layers on forward's inputs: dout [B, out_dim] is
        the gradient at forward's output (PolicyHead.backward's dx1). Two launches, no host synchronisation; the
        call recomputes the forward itself. Returns preallocated device tensors, cached per (B, E, stream) and
        valid until the next call with them: dweights [floats of the blob] -- the gradient of every conv-layer
        weight in the blob's own layout, overwritten, not accumulated, 0 over EmbedConv's entries (gradients()
        names them) -- and, with dh0=True, dh0 [B, E, embed_hidden], the gradient at EmbedConv's output (None
        otherwise). The workspace (one float64 row of the conv entries per 256 graphs) is cached with them.
        Every size forward accepts is accepted: where a graph's backward does not fit one workgroup's LDS
        (lsm_gnn_backward's limit, E = 113 at the defaults) the call goes to lsm_gnn_backward_large
        (``include/lsm_gnn_backward_large.h``), which keeps part of a graph's buffers in a scratch behind the
        workspace; the result and the number of launches are the same.
        embed=True: EmbedConv's backward (embed_backward) follows on the same stream, two more launches, seeded
        by this call's dh0 (produced internally whatever dh0= says) and writing the EmbedConv range of the same
        dweights, which is then the complete gradient. embed=False: the EmbedConv range is 0."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        adj = self._tensor(adj, "adj", shape=(B, E, E))
        return self._run_backward(node_obs, adj, None, B, E, 1, dout, agent_id, dh0, check, embed)

    def backward_compact(self, node_obs, table, masks, num_agents: int, dout, agent_id=None, dh0: bool = False,
                         check: bool = False, embed: bool = False):
        """backward on forward_compact's inputs."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        N = int(num_agents)
        if N < 1 or B % N:
            raise GnnError("node_obs holds %d graphs, not a multiple of num_agents = %d" % (B, N))
        table = self._tensor(table, "table", shape=(B // N, E, E))
        if not isinstance(masks, torch.Tensor) or masks.numel() != B * ((E + 63) // 64):
            raise GnnError("masks must hold [n * N, ceil(E / 64)] words")
        masks = self._tensor(masks.reshape(B, (E + 63) // 64), "masks", dtype=torch.int64, shape=(B, (E + 63) // 64))
        return self._run_backward(node_obs, table, masks, B, E, N, dout, agent_id, dh0, check, embed)

    def backward_step(self, node_obs, adj, adj_mask, num_agents: int, dout, agent_id=None, dh0: bool = False,
                      check: bool = False, embed: bool = False):
        """backward on forward_step's inputs (either adjacency layout); dout [n * N, out_dim]."""
        E, F = int(node_obs.shape[-2]), int(node_obs.shape[-1])
        node = node_obs.reshape(-1, E, F)
        aid = None if agent_id is None else agent_id.reshape(-1)
        if adj_mask is None:
            return self.backward(node, adj.reshape(-1, E, E), dout, aid, dh0=dh0, check=check, embed=embed)
        return self.backward_compact(node, adj, adj_mask, num_agents, dout, aid, dh0=dh0, check=check, embed=embed)

    # ---- EmbedConv's backward, from dh0 (include/lsm_gnn_embed_backward.h) ---------------------------------------

    def embed_floats(self) -> int:
        """lsm_gnn_embed_floats(cfg): the blob's EmbedConv entries, [0, offset of conv layer 0)."""
        return int(self.lib.lsm_gnn_embed_floats(self._struct))

    def _emb_outputs(self, B, E):
        torch = _torch()
        n = int(self.lib.lsm_gnn_embed_backward_workspace_bytes(self._struct, B, E))
        if n == 0 and B > 0:
            raise GnnError(self.lib.lsm_gnn_embed_backward_last_error().decode())
        return {"dembed": torch.zeros(self.embed_floats(), dtype=torch.float32, device=self.device),
                "workspace": torch.empty(max(n // 8, 1), dtype=torch.float64, device=self.device)}

    def _run_embed_backward(self, node_obs, adj, masks, B, E, N, dh0, out, check):
        torch = _torch()
        cfg = self.cfg
        node_obs = self._tensor(node_obs, "node_obs", shape=(B, E, cfg.F))
        dh0 = self._tensor(dh0, "dh0", shape=(B, E, cfg.embed_hidden), detach=True)
        sh = self._stream()
        cached = self._emb_out.get((B, E, sh), lambda: self._emb_outputs(B, E))
        n = self.embed_floats()
        if out is None:
            out = cached["dembed"]
        elif (not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32
              or not out.is_contiguous() or out.numel() < n):
            raise GnnError("out must be a contiguous float32 CUDA (HIP) tensor of at least %d values" % n)
        io = capi.LsmGnnEmbedBwdIo(node_obs=ptr(node_obs), adj=ptr(adj), masks=ptr(masks), dh0=ptr(dh0),
                                   dembed=ptr(out), workspace=ptr(cached["workspace"]), bad=ptr(self.bad))
        rc = self.lib.lsm_gnn_embed_backward(self._struct, C.c_void_p(self.weights.data_ptr()), C.byref(io), B, E, N,
                                             C.c_void_p(sh))
        self._finish(rc, self.lib.lsm_gnn_embed_backward_last_error, check,
                     "an entity type outside [0, num_embeddings) reached the encoder")
        return {"dembed": out.reshape(-1)[:n]}

    def embed_backward(self, node_obs, adj, dh0, out=None, check: bool = False):
        """EmbedConv's backward on forward's inputs: dh0 [B, E, embed_hidden] is the gradient at EmbedConv's
        output (backward's dh0). Two launches, no host synchronisation; the per-edge MLP is recomputed. Returns
        {'dembed': tensor}: the gradient of the blob's EmbedConv entries (entity embedding, lin1, the shared
        LayerNorm, the embed layers) in the blob's own layout, [embed_floats()] values, overwritten, not
        accumulated; preallocated and cached per (B, E, stream) with the workspace, valid until the next call
        with them. out=: a contiguous float32 device tensor to write into instead (its first embed_floats()
        values; a backward()'s dweights, for one)."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        adj = self._tensor(adj, "adj", shape=(B, E, E))
        return self._run_embed_backward(node_obs, adj, None, B, E, 1, dh0, out, check)

    def embed_backward_compact(self, node_obs, table, masks, num_agents: int, dh0, out=None, check: bool = False):
        """embed_backward on forward_compact's inputs."""
        torch = _torch()
        if not isinstance(node_obs, torch.Tensor) or node_obs.dim() != 3:
            raise GnnError("node_obs must be a CUDA (HIP) tensor [B, E, F]; there is no CPU fallback")
        B, E = int(node_obs.shape[0]), int(node_obs.shape[1])
        N = int(num_agents)
        if N < 1 or B % N:
            raise GnnError("node_obs holds %d graphs, not a multiple of num_agents = %d" % (B, N))
        table = self._tensor(table, "table", shape=(B // N, E, E))
        if not isinstance(masks, torch.Tensor) or masks.numel() != B * ((E + 63) // 64):
            raise GnnError("masks must hold [n * N, ceil(E / 64)] words")
        masks = self._tensor(masks.reshape(B, (E + 63) // 64), "masks", dtype=torch.int64, shape=(B, (E + 63) // 64))
        return self._run_embed_backward(node_obs, table, masks, B, E, N, dh0, out, check)

    def embed_backward_step(self, node_obs, adj, adj_mask, num_agents: int, dh0, out=None, check: bool = False):
        """embed_backward on forward_step's inputs (either adjacency layout); dh0 [n * N, E, embed_hidden]."""
        E, F = int(node_obs.shape[-2]), int(node_obs.shape[-1])
        node = node_obs.reshape(-1, E, F)
        dh0 = dh0.reshape(-1, E, self.cfg.embed_hidden)
        if adj_mask is None:
            return self.embed_backward(node, adj.reshape(-1, E, E), dh0, out=out, check=check)
        return self.embed_backward_compact(node, adj, adj_mask, num_agents, dh0, out=out, check=check)

    def gradients(self, prefix: str = "gnn."):
        """{state-dict name: gradient}: views, without a copy, of the last backward()'s dweights in the
        parameters' shapes, under the names of weight_entries (layer_norm entries only with layer norm). After
        backward(embed=True) this is the complete gradient; after a plain backward() the EmbedConv entries are 0.
        They are that call's cached tensor: valid until the next backward() with its (B, E, stream)."""
        if self._last_dweights is None:
            raise GnnError("gradients() follows a backward()")
        out, o = {}, 0
        for name, shape in weight_entries(self.cfg):
            n = int(np.prod(shape))
            if self.cfg.layer_norm or ".layer_norm." not in name:
                out[prefix + name] = self._last_dweights[o:o + n].view(shape)
            o += n
        return out
