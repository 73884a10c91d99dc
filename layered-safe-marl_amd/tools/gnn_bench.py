"""Device time of the graph encoder's forward pass (GNNBase.forward) on a step's outputs:

  (A) lsm.gnn.GraphEncoder: one launch of csrc/lsm_gnn.hip on node_obs + the adjacency as the step left
      them (GpuGraphVecEnv.gnn_features), no edge list;
  (B) the same formulas in plain torch on the device: lsm.edges.process_adj (which synchronises), then
      index_select / index_add_ / scatter_reduce_ over [nnz, hidden] and [nnz, H, C] tensors, the shape
      of the reference's torch_geometric path.

Configurations: 4096 envs x 8 agents (B = 32768 graphs, E = 24) in both adjacency layouts, and 128 envs
x 64 agents (B = 8192, E = 192); the reference's default network; the actor's readout ('node') and the
critic's ('global' mean). The inputs are a real env's step outputs after a few random steps. For the
actor, (A) is also timed with the last layer's attention restricted to the ego row (cfg.ego_only).

Method: both sides are run once and checked first, by the tests' criterion on the first 8 envs' graphs:
the same torch ops in float64 are the truth, e32 is the float32 torch path's error against it, and a
fused error above 4 * e32 + 4 * 2^-23 * max|truth| ends the run (the two float32 results' own distance
is recorded, not judged: at E = 192 sums over ~190 incoming edges make it a few 1e-3 of the output). Then a
warm-up, HIP events on the stream around `reps` back-to-back calls, the sides in alternating rounds, and
the median / min / max of the rounds' means (tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/gnn_bench.py [--out FILE] [--quick]
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


def torch_forward(cfg, p, node_obs, adj, agent_id, edge_list=None):
    """GNNBase.forward as torch ops on the device, in node_obs' dtype. p: {name: tensor} (the reference's
    parameter names without prefix). edge_list: process_adj's result when the caller already has it."""
    import torch
    import torch.nn.functional as Fn
    from lsm import edges
    B, E, F = node_obs.shape
    H, C, Hd = cfg.H, cfg.C, cfg.embed_hidden
    act_e = torch.relu if cfg.embed_relu else torch.tanh
    act_g = torch.relu if cfg.relu else torch.tanh
    ei, e = edges.process_adj(adj) if edge_list is None else edge_list
    src, dst = ei[0], ei[1]
    dt = node_obs.dtype
    x = node_obs.reshape(B * E, F)
    emb = p["embed_layer.entity_embed.weight"][x[:, F - 1].long()]

    def ln(v):
        if not cfg.layer_norm:
            return v
        return Fn.layer_norm(v, (Hd,), p["embed_layer.layer_norm.weight"], p["embed_layer.layer_norm.bias"], 1e-5)

    m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
    m = ln(act_e(Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])))
    for k in range(cfg.embed_layer_N):
        m = ln(act_e(Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)], p["embed_layer.layers.%d.bias" % (3 * k)])))
    h = torch.zeros(B * E, Hd, device=x.device, dtype=dt).index_add_(0, dst, m)
    dsth = dst.unsqueeze(1).expand(-1, H)
    for conv in ["gnn1"] + ["gnn2.%d" % i for i in range(cfg.layer_N)]:
        lin = lambda nm, v: Fn.linear(v, p["%s.lin_%s.weight" % (conv, nm)], p["%s.lin_%s.bias" % (conv, nm)])
        q, k, v = (lin(nm, h).view(-1, H, C) for nm in ("query", "key", "value"))
        ee = Fn.linear(e, p["%s.lin_edge.weight" % conv]).view(-1, H, C)
        logit = (q.index_select(0, dst) * (k.index_select(0, src) + ee)).sum(dim=-1) / float(C) ** 0.5
        amax = torch.full((B * E, H), -float("inf"), device=x.device, dtype=dt).scatter_reduce_(0, dsth, logit, "amax")
        pexp = torch.exp(logit - amax.index_select(0, dst))
        den = torch.zeros(B * E, H, device=x.device, dtype=dt).index_add_(0, dst, pexp)
        alpha = pexp / (den.index_select(0, dst) + 1e-16)
        o = torch.zeros(B * E, H, C, device=x.device, dtype=dt).index_add_(0, dst, alpha.unsqueeze(-1) * (v.index_select(0, src) + ee))
        o = o.reshape(B * E, H * C) if cfg.concat else o.mean(dim=1)
        h = act_g(o + lin("skip", h))
    h = h.view(B, E, -1)
    if cfg.aggr == "node":
        return h.gather(1, agent_id.view(B, 1, 1).expand(-1, -1, h.size(-1))).squeeze(1)
    return {"global_mean": h.mean(dim=1), "global_max": h.max(dim=1)[0], "global_add": h.sum(dim=1)}[cfg.aggr]


def seeded_state_dict(cfg, seed=0):
    """Weights at O(1) output scale (rows ~ U(-1, 1) * 1.5 / sqrt(fan_in)), as the tests use."""
    import numpy as np
    from lsm import gnn
    rng = np.random.default_rng(seed)
    sd = {}
    for name, shape in gnn.weight_entries(cfg):
        if name.endswith("layer_norm.weight"):
            a = 1.0 + 0.3 * rng.normal(size=shape)
        elif name.endswith("bias"):
            a = 0.3 * rng.normal(size=shape)
        elif len(shape) == 2 and shape[1] > 1 and "entity_embed" not in name:
            a = rng.uniform(-1, 1, size=shape) * 1.5 / np.sqrt(shape[1])
        else:
            a = 0.5 * rng.normal(size=shape)
        sd[name] = a.astype(np.float32)
    return sd


def bench_env(envs, agents, layout, quick):
    import torch
    from lsm import edges, gnn, hj_tables
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    # bench.py's configs 3 and 5 (double integrator, HJ filter on, world_size 4)
    args = EnvArgs(dynamics_type="double_integrator", num_agents=agents, num_landmarks=2, world_size=4,
                   episode_length=250, num_env_steps=1000, use_safety_filter=True, seed=0)
    vt = hj_tables.default_tables("double_integrator", small=True)[0]
    env = GpuGraphVecEnv(args, num_envs=envs, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                         adj_layout=layout)
    env.reset(0)
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(5):
        env.step(torch.randint(0, 25, (envs, agents), generator=g, device=DEV, dtype=torch.int32), 0)
    B, E, F = envs * agents, env.E, env.F
    node = env.t_node.view(B, E, F)
    dense = env.reference_adj().reshape(B, E, E).contiguous()
    aid = env.agent_id.view(B)
    nnz = int((dense != 0).sum().item())
    res = {"envs": envs, "agents": agents, "layout": layout, "B": B, "E": E, "F": F, "edges": nnz,
           "edges_per_graph": nnz / B, "kernel": env.kernel_name}
    for role, aggr in (("actor", "node"), ("critic", "global_mean")):
        cfg = gnn.GnnConfig(F=F, aggr=aggr)
        sd = seeded_state_dict(cfg)
        enc = gnn.GraphEncoder(cfg, gnn.pack_weights(sd, cfg, prefix=""), DEV)
        p = {k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}
        fused = lambda: env.gnn_features(enc)
        plain = lambda: torch_forward(cfg, p, node, dense, aid)
        a, b = fused().clone(), plain()
        diff, scale = float((a - b).abs().max().item()), float(b.abs().max().item())
        # the tests' criterion on the first graphs: both float32 results against the same torch ops in float64
        nb = min(B, 8 * agents)
        el = edges.process_adj(dense[:nb])
        p64 = {k: v.double() for k, v in p.items()}
        r64 = torch_forward(cfg, p64, node[:nb].double(), None, aid[:nb], (el[0], el[1].double()))
        # a float64 result far outside the float32 results' range is no truth to judge by: recorded, not used
        usable = float(r64.abs().max().item()) <= 10.0 * max(1.0, scale)
        chk = criterion({role: a[:nb]}, {role: b[:nb]}, {role: r64}, [role], layout, bound="4 * e32 + 4 ulp =",
                        enforce=usable)[role]
        err, e32 = chk["fused_err_vs_float64"], chk["torch_err_vs_float64"]
        sides = {"fused": (fused, 5 if quick else 20), "torch": (plain, 1 if quick else 3)}
        if aggr == "node":
            enc_ego = gnn.GraphEncoder(gnn.GnnConfig(F=F, aggr=aggr, ego_only=True), enc.weights, DEV)
            if not torch.equal(env.gnn_features(enc_ego), a):
                raise SystemExit("%s: ego_only changed the output" % layout)
            sides["fused_ego_only"] = (lambda: env.gnn_features(enc_ego), sides["fused"][1])
        for fn, _ in sides.values():   # warm-up
            fn()
        t = alternated(sides)
        res[role] = dict(t, max_abs_diff=diff, max_abs_output=scale, checked_graphs=nb, float64_check_usable=usable, fused_err_vs_float64=err,
                         torch_err_vs_float64=e32, ratio_torch_over_fused=t["torch"]["median"] / t["fused"]["median"])
        print("%d x %d %s %s: fused %.3f ms, torch %.3f ms (x%.1f)%s" % (
            envs, agents, layout, role, t["fused"]["median"], t["torch"]["median"], res[role]["ratio_torch_over_fused"],
            ", ego-only %.3f ms" % t["fused_ego_only"]["median"] if "fused_ego_only" in t else ""),
            file=sys.stderr, flush=True)
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    ap.add_argument("--only", default=None, help="'small' (E = 24) or 'large' (E = 192)")
    a = ap.parse_args()
    runs = []
    if a.only in (None, "small"):
        runs += [bench_env(4096, 8, "reference", a.quick), bench_env(4096, 8, "compact", a.quick)]
    if a.only in (None, "large"):
        runs += [bench_env(128, 64, "compact", a.quick)]   # the layout bench.py's config 5 steps in
    emit({"gnn_bench": runs}, a.out)


if __name__ == "__main__":
    main()
