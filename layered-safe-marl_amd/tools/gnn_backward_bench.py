"""Device time of the graph encoder's backward pass through the readout and the TransformerConv layers, from
the gradient at the encoder's output to every conv-layer weight's gradient and dh0:

  (A) lsm.gnn.GraphEncoder.backward_step: two launches of csrc/lsm_gnn_backward.hip on node_obs + the adjacency
      as the step left them (either layout), recomputing the forward itself, no edge list;
  (B) the same formulas as edge-list torch ops on the device (the shape of the reference's torch_geometric path):
      EmbedConv without a graph, its output h0 and the conv parameters as leaves, the conv layers and the readout
      with the graph kept, then torch.autograd.backward to the conv parameters and h0. Two variants: the forward
      with the backward (what a PPO update pays, and the figure to compare (A) with, since (A) recomputes the
      forward), and the backward alone on a kept graph. The edge list (lsm.edges.process_adj, which
      synchronises) is built once outside the timing, in torch's favour.

Shapes: tools/gnn_bench.py's, 4096 envs x 8 agents (B = 32768 graphs, E = 24) in both adjacency layouts and 128
envs x 64 agents (B = 8192, E = 192); the reference's default network; the actor's readout ('node') and the
critic's ('global' mean). E = 192 is beyond lsm_gnn_backward's LDS limit and runs through the spilled tier
(include/lsm_gnn_backward_large.h); each row records the plan (the spill level, G, the LDS and the scratch) and the
time per graph. A size even that refuses is recorded with the refusal's text and not timed.

  (C) the price of spilling where both exist: at 4096 x 8, E = 24, lsm_gnn_backward_large with min_spill = 0
      (lsm_gnn_backward's own kernel) against min_spill = 4 (only the forward's region left in LDS) on the same
      inputs, checked bit-equal first, in alternating rounds.

Method: both sides are run once and checked first, by the tests' criterion on the first 8 envs' graphs: the same
torch ops in float64 are the truth, e32 is the float32 torch path's error against it per gradient tensor, and a
fused error above 4 * e32 + 4 * 2^-23 * max|truth| ends the run. Then a warm-up, HIP events on the stream around
`reps` back-to-back calls, the sides in alternating rounds, and the median / min / max of the rounds' means
(tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/gnn_backward_bench.py [--out FILE] [--quick] [--only small|large|spill]
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
PROFILE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "gnn_backward_bench.json")


def conv_names(cfg):
    out = []
    for conv in ["gnn1"] + ["gnn2.%d" % i for i in range(cfg.layer_N)]:
        for lin in ("query", "key", "value"):
            out += ["%s.lin_%s.weight" % (conv, lin), "%s.lin_%s.bias" % (conv, lin)]
        out += ["%s.lin_edge.weight" % conv, "%s.lin_skip.weight" % conv, "%s.lin_skip.bias" % conv]
    return out


def embed(cfg, p, node_obs, edge_list):
    """EmbedConv's output h0 [B * E, embed_hidden], without a graph."""
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

    with torch.no_grad():
        emb = p["embed_layer.entity_embed.weight"][x[:, F - 1].long()]
        m = torch.cat([x.index_select(0, src)[:, :F - 1], emb.index_select(0, src), e], dim=1)
        m = ln(act_e(Fn.linear(m, p["embed_layer.lin1.weight"], p["embed_layer.lin1.bias"])))
        for k in range(cfg.embed_layer_N):
            m = ln(act_e(Fn.linear(m, p["embed_layer.layers.%d.weight" % (3 * k)],
                                   p["embed_layer.layers.%d.bias" % (3 * k)])))
        return torch.zeros(B * E, Hd, device=x.device, dtype=x.dtype).index_add_(0, dst, m)


def conv_forward(cfg, p, h0, B, E, edge_list, agent_id):
    """The conv layers and the readout on h0, with the graph kept: [B, out_dim]."""
    import torch
    import torch.nn.functional as Fn
    H, C = cfg.H, cfg.C
    act_g = torch.relu if cfg.relu else torch.tanh
    (src, dst), e = edge_list
    dt, dev = h0.dtype, h0.device
    dsth = dst.unsqueeze(1).expand(-1, H)
    h = h0
    for conv in ["gnn1"] + ["gnn2.%d" % i for i in range(cfg.layer_N)]:
        lin = lambda nm, v: Fn.linear(v, p["%s.lin_%s.weight" % (conv, nm)], p["%s.lin_%s.bias" % (conv, nm)])
        q, k, v = (lin(nm, h).view(-1, H, C) for nm in ("query", "key", "value"))
        ee = Fn.linear(e, p["%s.lin_edge.weight" % conv]).view(-1, H, C)
        logit = (q.index_select(0, dst) * (k.index_select(0, src) + ee)).sum(dim=-1) / float(C) ** 0.5
        amax = torch.full((B * E, H), -float("inf"), device=dev, dtype=dt).scatter_reduce_(0, dsth, logit.detach(), "amax")
        pexp = torch.exp(logit - amax.index_select(0, dst))
        den = torch.zeros(B * E, H, device=dev, dtype=dt).index_add(0, dst, pexp)
        alpha = pexp / (den.index_select(0, dst) + 1e-16)
        o = torch.zeros(B * E, H, C, device=dev, dtype=dt).index_add(0, dst, alpha.unsqueeze(-1) * (v.index_select(0, src) + ee))
        o = o.reshape(B * E, H * C) if cfg.concat else o.mean(dim=1)
        h = act_g(o + lin("skip", h))
    h = h.view(B, E, -1)
    if cfg.aggr == "node":
        return h.gather(1, agent_id.view(B, 1, 1).expand(-1, -1, h.size(-1))).squeeze(1)
    return {"global_mean": h.mean(dim=1), "global_max": h.max(dim=1)[0], "global_add": h.sum(dim=1)}[cfg.aggr]


def torch_gradients(cfg, p, h0, B, E, edge_list, agent_id, dout):
    """{conv parameter name: gradient, 'dh0': [B, E, embed_hidden]} by torch.autograd on fresh leaves."""
    import torch
    names = conv_names(cfg)
    leaves = dict(p)
    for nm in names:
        leaves[nm] = p[nm].detach().clone().requires_grad_(True)
    h = h0.detach().clone().requires_grad_(True)
    out = conv_forward(cfg, leaves, h, B, E, edge_list, agent_id)
    torch.autograd.backward([out], [dout])
    res = {nm: leaves[nm].grad for nm in names}
    res["dh0"] = h.grad.view(B, E, -1)
    return res


def large_plan(lib, cfg, B, E, min_spill=0):
    import ctypes as C
    from lsm import capi
    p = capi.LsmGnnBwdLargeLaunchPlan()
    if lib.lsm_gnn_backward_large_plan(cfg.struct(), B, E, 1, 0, min_spill, C.byref(p)):
        return {"refused": lib.lsm_gnn_backward_large_last_error().decode()}
    return {n: int(getattr(p, n)) for n, _ in p._fields_}


def bench_spill(envs, agents, quick):
    """(C): level 0 against level 4 through the C ABI, on a step's graphs in the reference layout."""
    import ctypes as C
    import torch
    from lsm import capi, gnn, hj_tables
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    args = EnvArgs(dynamics_type="double_integrator", num_agents=agents, num_landmarks=2, world_size=4,
                   episode_length=250, num_env_steps=1000, use_safety_filter=True, seed=0)
    vt = hj_tables.default_tables("double_integrator", small=True)[0]
    env = GpuGraphVecEnv(args, num_envs=envs, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                         adj_layout="reference")
    env.reset(0)
    g = torch.Generator(device=DEV).manual_seed(3)
    for _ in range(5):
        env.step(torch.randint(0, 25, (envs, agents), generator=g, device=DEV, dtype=torch.int32), 0)
    B, E, F = envs * agents, env.E, env.F
    node = env.t_node.view(B, E, F).contiguous()
    dense = env.reference_adj().reshape(B, E, E).contiguous()
    aid = env.agent_id.view(B).long().contiguous()
    lib = capi.load_library()
    res = {"envs": envs, "agents": agents, "layout": "reference", "B": B, "E": E}
    for role, aggr in (("actor", "node"), ("critic", "global_mean")):
        cfg = gnn.GnnConfig(F=F, aggr=aggr)
        enc = gnn.GraphEncoder(cfg, gnn.pack_weights(seeded_state_dict(cfg), cfg, prefix=""), DEV)
        dout = torch.randn((B, cfg.out_dim), generator=g, device=DEV)
        bad = torch.zeros(1, dtype=torch.int64, device=DEV)
        sides, outs, plans = {}, {}, {}
        for k in (0, 4):
            n = int(lib.lsm_gnn_backward_large_workspace_bytes(cfg.struct(), B, E, k))
            o = {"dweights": torch.zeros(enc.weights.numel(), device=DEV), "dh0": torch.empty((B, E, cfg.embed_hidden), device=DEV),
                 "workspace": torch.empty((n + 7) // 8, dtype=torch.float64, device=DEV)}
            io = capi.LsmGnnBwdIo(node_obs=node.data_ptr(), adj=dense.data_ptr(), masks=None,
                                  agent_id=aid.data_ptr() if aggr == "node" else None, dout=dout.data_ptr(),
                                  dweights=o["dweights"].data_ptr(), dh0=o["dh0"].data_ptr(),
                                  workspace=o["workspace"].data_ptr(), bad=bad.data_ptr())

            def run(k=k, io=io):
                rc = lib.lsm_gnn_backward_large(cfg.struct(), C.c_void_p(enc.weights.data_ptr()), C.byref(io), B, E, 1, k,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream))
                if rc:
                    raise RuntimeError(lib.lsm_gnn_backward_large_last_error().decode())
            run()
            outs[k], plans[k] = o, large_plan(lib, cfg, B, E, k)
            sides["level%d" % k] = (run, 3 if quick else 10)
        torch.cuda.synchronize()
        for nm in ("dweights", "dh0"):
            if not torch.equal(outs[0][nm].view(torch.int32), outs[4][nm].view(torch.int32)):
                raise SystemExit("level 4 differs from level 0 in %s (%s)" % (nm, role))
        t = alternated(sides)
        res[role] = dict(t, plan_level0=plans[0], plan_level4=plans[4], bit_equal=True,
                         ratio_level4_over_level0=t["level4"]["median"] / t["level0"]["median"])
        print("%d x %d spill %s: level 0 %.3f ms [%.3f, %.3f], level 4 %.3f ms [%.3f, %.3f] (x%.2f)" % (
            envs, agents, role, t["level0"]["median"], t["level0"]["min"], t["level0"]["max"], t["level4"]["median"],
            t["level4"]["min"], t["level4"]["max"], res[role]["ratio_level4_over_level0"]), file=sys.stderr, flush=True)
    env.close()
    return res


def bench_env(envs, agents, layout, quick, enforce=True):
    import torch
    from lsm import edges, gnn, hj_tables
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    # tools/gnn_bench.py's environments (bench.py's configs 3 and 5)
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
        fused = lambda: enc.backward_step(env.t_node, env.t_adj, env.t_adj_mask, env.N, dout, env.agent_id, dh0=True)
        try:
            fused()
        except gnn.GnnError as err:
            res[role] = {"refused": str(err)}
            print("%d x %d %s %s: %s" % (envs, agents, layout, role, err), file=sys.stderr, flush=True)
            continue
        names = conv_names(cfg) + ["dh0"]
        # the tests' criterion on the first graphs: both float32 results against the same torch ops in float64
        nb = min(B, 8 * agents)
        eln = edges.process_adj(dense[:nb])
        eln = ((eln[0][0], eln[0][1]), eln[1])
        sub = enc.backward(node[:nb].contiguous(), dense[:nb].contiguous(), dout[:nb].contiguous(), aid[:nb].contiguous(),
                           dh0=True)
        f_sub = {n: (sub["dh0"] if n == "dh0" else enc.gradients()["gnn." + n]).clone() for n in names}
        h0n = embed(cfg, p, node[:nb], eln)
        t32 = torch_gradients(cfg, p, h0n, nb, E, eln, aid[:nb], dout[:nb])
        p64 = {k: v.double() for k, v in p.items()}
        h064 = embed(cfg, p64, node[:nb].double(), (eln[0], eln[1].double()))
        t64 = torch_gradients(cfg, p64, h064, nb, E, (eln[0], eln[1].double()), aid[:nb], dout[:nb].double())
        chk = criterion(f_sub, t32, t64, names, "%s %s" % (layout, role), bound="4 * e32 + 4 ulp =", enforce=enforce)
        worst = max(names, key=lambda n: chk[n]["fused_err_vs_float64"] / max(chk[n]["tolerance"], 1e-300))
        # the timed sides
        h0 = embed(cfg, p, node, el)
        leaves = dict(p)
        for nm in conv_names(cfg):
            leaves[nm] = p[nm].detach().clone().requires_grad_(True)
        hleaf = h0.detach().clone().requires_grad_(True)

        def fwd_bwd():
            o = conv_forward(cfg, leaves, hleaf, B, E, el, aid)
            torch.autograd.backward([o], [dout])

        kept = conv_forward(cfg, leaves, hleaf, B, E, el, aid)
        bwd = lambda: torch.autograd.backward([kept], [dout], retain_graph=True)
        sides = {"fused": (fused, 3 if quick else 10), "torch_forward_backward": (fwd_bwd, 1 if quick else 3),
                 "torch_backward": (bwd, 1 if quick else 3)}
        for fn, _ in sides.values():   # warm-up
            fn()
        t = alternated(sides)
        plan = large_plan(enc.lib, cfg, B, E)
        res[role] = dict(t, checked_graphs=nb, worst_tensor=worst, worst_check=chk[worst], plan=plan,
                         fused_us_per_graph=1e3 * t["fused"]["median"] / B,
                         ratio_torch_forward_backward_over_fused=t["torch_forward_backward"]["median"] / t["fused"]["median"])
        print("%d x %d %s %s: fused %.3f ms [%.3f, %.3f], torch forward + backward %.3f ms [%.3f, %.3f] (x%.2f), "
              "torch backward alone %.3f ms" % (
                  envs, agents, layout, role, t["fused"]["median"], t["fused"]["min"], t["fused"]["max"],
                  t["torch_forward_backward"]["median"], t["torch_forward_backward"]["min"],
                  t["torch_forward_backward"]["max"], res[role]["ratio_torch_forward_backward_over_fused"],
                  t["torch_backward"]["median"]), file=sys.stderr, flush=True)
        del kept, leaves, hleaf
    env.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=PROFILE)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    ap.add_argument("--only", default=None, help="'small' (E = 24), 'large' (E = 192) or 'spill' (level 0 against 4)")
    ap.add_argument("--record-only", action="store_true", help="record the criterion's figures without ending the run on a miss")
    a = ap.parse_args()
    runs = []
    if a.only in (None, "small"):
        runs += [bench_env(4096, 8, "reference", a.quick, not a.record_only),
                 bench_env(4096, 8, "compact", a.quick, not a.record_only)]
    if a.only in (None, "large"):
        runs += [bench_env(128, 64, "compact", a.quick, not a.record_only)]
    out = {"gnn_backward_bench": runs}
    if a.only in (None, "small", "spill"):
        out["gnn_backward_spill_bench"] = [bench_spill(4096, 8, a.quick)]
    emit(out, a.out)


if __name__ == "__main__":
    main()
