"""Device time of EmbedConv's backward pass, from dh0 (the gradient at EmbedConv's output) to the gradient of the
entity embedding, lin1, the shared LayerNorm and the embed layers:

  (A) lsm.gnn.GraphEncoder.embed_backward_step: two launches of csrc/lsm_gnn_embed_backward.hip on node_obs + the
      adjacency as the step left them (either layout), recomputing the per-edge MLP, no edge list;
  (B) EmbedConv alone as edge-list torch ops on the device, every EmbedConv parameter a leaf: the forward and
      torch.autograd.backward([h0], [dh0]), seeded by the same dh0 (what a PPO update pays, and the figure to
      compare (A) with, since (A) recomputes the forward). The edge list (lsm.edges.process_adj, which
      synchronises) is built once outside the timing, in torch's favour.
  (C) GraphEncoder.backward_step with embed=True against the plain call: the cost the embed call adds to the
      encoder's backward (tools/gnn_backward_bench.py times the plain call against torch).

Shapes: tools/gnn_backward_bench.py's small one, 4096 envs x 8 agents (B = 32768 graphs, E = 24) after five random
steps, in both adjacency layouts; the reference's default network; dh0 is the conv backward's own, under the
actor's readout ('node': most rows are zero) and the critic's ('global' mean).

Method: both sides are run once and checked first, by the tests' criterion on the first 64 graphs: the same torch
ops in float64 are the truth, e32 is the float32 torch path's error against it per gradient tensor, and a fused
error above 4 * e32 + 4 * 2^-23 * max|truth| ends the run. Then a warm-up, HIP events on the stream around `reps`
back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds' means
(tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/gnn_embed_backward_bench.py [--out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, criterion, emit  # noqa: E402
from gnn_bench import seeded_state_dict  # noqa: E402

DEV = "cuda:0"
PROFILE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "gnn_embed_backward_bench.json")
CHECKED = 64


def embed_names(cfg):
    from lsm import gnn
    return [n for n, _ in gnn.weight_entries(cfg)
            if n.startswith("embed_layer.") and (cfg.layer_norm or ".layer_norm." not in n)]


def embed_forward(cfg, p, node_obs, edge_list):
    """EmbedConv's output h0 [B * E, embed_hidden] with the graph kept."""
    import torch
    import torch.nn.functional as Fn
    B, E, F = node_obs.shape
    Hd = cfg.embed_hidden
    act_e = torch.relu if cfg.embed_relu else torch.tanh
    (src, dst), e = edge_list
    x = node_obs.reshape(B * E, F)

    def ln(v):
        if not cfg.layer_norm:
            return v
        return Fn.layer_norm(v, (Hd,), p["embed_layer.layer_norm.weight"], p["embed_layer.layer_norm.bias"], 1e-5)

    emb = p["embed_layer.entity_embed.weight"][x[:, F - 1].long()]
    m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
    m = ln(act_e(Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])))
    for k in range(cfg.embed_layer_N):
        m = ln(act_e(Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)], p["embed_layer.layers.%d.bias" % (3 * k)])))
    return torch.zeros(B * E, Hd, device=x.device, dtype=x.dtype).index_add(0, dst, m)


def torch_gradients(cfg, p, node_obs, edge_list, dh0):
    """{EmbedConv parameter name: gradient} by torch.autograd on fresh leaves."""
    import torch
    names = embed_names(cfg)
    leaves = dict(p)
    for nm in names:
        leaves[nm] = p[nm].detach().clone().requires_grad_(True)
    h0 = embed_forward(cfg, leaves, node_obs, edge_list)
    torch.autograd.backward([h0], [dh0.reshape(h0.shape)])
    return {nm: leaves[nm].grad for nm in names}


def bench_env(envs, agents, layout, quick, enforce=True):
    import torch
    from lsm import edges, gnn, hj_tables
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    # tools/gnn_bench.py's small environment (bench.py's config 3)
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
    el = edges.process_adj(dense)
    el = ((el[0][0], el[0][1]), el[1])
    nnz = int(el[1].shape[0])
    res = {"envs": envs, "agents": agents, "layout": layout, "B": B, "E": E, "F": F, "edges": nnz,
           "edges_per_graph": nnz / B}
    for role, aggr in (("actor", "node"), ("critic", "global_mean")):
        cfg = gnn.GnnConfig(F=F, aggr=aggr)
        sd = seeded_state_dict(cfg)
        enc = gnn.GraphEncoder(cfg, gnn.pack_weights(sd, cfg, prefix=""), DEV)
        p = {k: torch.from_numpy(v).to(DEV) for k, v in sd.items()}
        dout = torch.randn((B, cfg.out_dim), generator=g, device=DEV)
        step = lambda **kw: enc.backward_step(env.t_node, env.t_adj, env.t_adj_mask, env.N, dout, env.agent_id, **kw)
        dh0 = step(dh0=True)["dh0"].clone()
        fused = lambda: enc.embed_backward_step(env.t_node, env.t_adj, env.t_adj_mask, env.N, dh0)
        fused()
        names = embed_names(cfg)
        # the tests' criterion on the first graphs: both float32 results against the same torch ops in float64
        nb = min(B, CHECKED)
        eln = edges.process_adj(dense[:nb])
        eln = ((eln[0][0], eln[0][1]), eln[1])
        sub = enc.embed_backward(node[:nb].contiguous(), dense[:nb].contiguous(), dh0[:nb].contiguous())["dembed"]
        f_sub, o = {}, 0
        for n, shape in gnn.weight_entries(cfg):
            k = 1
            for s in shape:
                k *= s
            if n in names:
                f_sub[n] = sub[o:o + k].view(shape).clone()
            o += k
            if o >= sub.numel():
                break
        t32 = torch_gradients(cfg, p, node[:nb], eln, dh0[:nb])
        p64 = {k: v.double() for k, v in p.items()}
        t64 = torch_gradients(cfg, p64, node[:nb].double(), (eln[0], eln[1].double()), dh0[:nb].double())
        chk = criterion(f_sub, t32, t64, names, "%s %s" % (layout, role), bound="4 * e32 + 4 ulp =", enforce=enforce)
        worst = max(names, key=lambda n: chk[n]["fused_err_vs_float64"] / max(chk[n]["tolerance"], 1e-300))
        # the timed sides
        leaves = dict(p)
        for nm in names:
            leaves[nm] = p[nm].detach().clone().requires_grad_(True)
        seed = dh0.reshape(B * E, cfg.embed_hidden)

        def fwd_bwd():
            torch.autograd.backward([embed_forward(cfg, leaves, node, el)], [seed])

        sides = {"fused": (fused, 3 if quick else 10), "torch_forward_backward": (fwd_bwd, 1 if quick else 3),
                 "backward_plain": (lambda: step(), 2 if quick else 5),
                 "backward_with_embed": (lambda: step(embed=True), 2 if quick else 5)}
        for fn, _ in sides.values():   # warm-up
            fn()
        t = alternated(sides)
        res[role] = dict(t, checked_graphs=nb, worst_tensor=worst, worst_check=chk[worst],
                         dh0_zero_rows=float((dh0.abs().amax(dim=2) == 0).float().mean().item()),
                         ratio_torch_forward_backward_over_fused=t["torch_forward_backward"]["median"] / t["fused"]["median"],
                         added_by_embed_ms=t["backward_with_embed"]["median"] - t["backward_plain"]["median"])
        print("%d x %d %s %s: fused %.3f ms [%.3f, %.3f], torch forward + backward %.3f ms [%.3f, %.3f] (x%.2f); "
              "backward %.3f ms, with embed %.3f ms" % (
                  envs, agents, layout, role, t["fused"]["median"], t["fused"]["min"], t["fused"]["max"],
                  t["torch_forward_backward"]["median"], t["torch_forward_backward"]["min"],
                  t["torch_forward_backward"]["max"], res[role]["ratio_torch_forward_backward_over_fused"],
                  t["backward_plain"]["median"], t["backward_with_embed"]["median"]), file=sys.stderr, flush=True)
        del leaves
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PROFILE)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--record-only", action="store_true", help="record the criterion's figures without ending the run on a miss")
    a = ap.parse_args()
    runs = [bench_env(a.envs, 8, "reference", a.quick, not a.record_only),
            bench_env(a.envs, 8, "compact", a.quick, not a.record_only)]
    emit({"gnn_embed_backward_bench": runs}, a.out)


if __name__ == "__main__":
    main()
