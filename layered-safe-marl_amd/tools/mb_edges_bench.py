"""Device time of a PPO minibatch delivered as the GNN consumes it -- every field plus edge_index /
edge_attr -- at the headline shape (4096 envs x 8 agents, T = EnvArgs().episode_length, E = 24,
data_chunk_length 10, 16 minibatches), for both generators and both adjacency layouts:

  (A) the generator with edges=True: adj left out of the gather launch, the edge list made from the
      buffer's own adjacency by lsm.edges.minibatch_edges (csrc/lsm_mb_edges.hip);
  (B) what the library did before: the default generator, which gathers the dense [G, E, E] adj, then
      lsm.edges.process_adj(batch["adj"]).

Both sides get the same permutation (so both pay the generator's one validation of it) and synchronise
once per minibatch, for the edge count. The outputs are compared first, every minibatch of both
generators (torch.equal on edge_index and edge_attr), and a difference ends the run. Then HIP events
around whole passes over the buffer (16 minibatches) on an otherwise idle stream, after a warm-up; the
sides are timed in alternating rounds and the median, minimum and maximum of the rounds' means are
recorded (tools/bench_common.py's alternated()).

    python layered-safe-marl_amd/tools/mb_edges_bench.py [--envs 4096] [--steps T] [--mini-batches 16] [--out FILE]

The bytes are the algorithm's, per minibatch of G graphs with nnz edges. Both sides: every field but adj
read and written once, the ids, 20 B per edge written. (B) adds the dense adjacency: read (E*E*4 per graph
in the reference layout, E*E*4 / N + the mask words in the compact one) and written by the gather, read by
the count pass and read by the emit pass. (A) reads the buffer's adjacency twice, count and emit, in its
own layout.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, emit  # noqa: E402

L_CHUNK, HIDDEN, ACTIONS = 10, 64, 25
REPS = 3   # passes over the buffer per round


def bench_layout(layout, a, T):
    import torch
    from lsm import edges as lsm_edges
    from lsm import hj_tables
    from lsm.buffer import DeviceGraphBuffer
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    dev = "cuda:0"
    n, N, L, k_mb = a.envs, 8, L_CHUNK, a.mini_batches
    M = n * N
    args = EnvArgs(num_agents=N, episode_length=T, num_env_steps=T * 4, use_safety_filter=True, seed=0)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    env = GpuGraphVecEnv(args, num_envs=n, device=dev, value_table=vt, return_numpy=False, build_infos=False,
                         adj_layout=layout)
    buf = DeviceGraphBuffer(env, episode_length=T,
                            policy_rows=dict(hidden_size=HIDDEN, recurrent_N=1, num_actions=ACTIONS))
    g = torch.Generator(device=dev).manual_seed(1)
    buf.warmup(4)
    for _ in range(T):
        acts = torch.randint(0, ACTIONS, (n, N), generator=g, device=dev, dtype=torch.int32)
        pol = dict(actions=acts.to(torch.float32).reshape(n, N, 1),
                   action_log_probs=torch.randn((n, N, 1), generator=g, device=dev),
                   rnn_states=torch.randn((n, N, 1, HIDDEN), generator=g, device=dev),
                   rnn_states_critic=torch.randn((n, N, 1, HIDDEN), generator=g, device=dev),
                   available_actions=(torch.rand((n, N, ACTIONS), generator=g, device=dev) > 0.2).float())
        buf.insert_step(acts, 4, value_preds=torch.randn((n, N), generator=g, device=dev), policy=pol)
    buf.compute_returns(torch.randn((n, N, 1), generator=g, device=dev), None, gamma=0.99, gae_lambda=0.95)
    adv, _ = buf.advantages(None)
    batch = T * M
    E = env.E
    W = (E + 63) // 64
    res = {"layout": layout, "envs": n, "agents": N, "T": T, "E": E, "L": L, "samples": batch, "mini_batches": k_mb}
    perm = torch.randperm(batch, generator=g, device=dev)
    cperm = torch.randperm(batch // L, generator=g, device=dev)

    def feed_forward(edges):
        return buf.feed_forward_generator(adv, num_mini_batch=k_mb, indices=perm, edges=edges)

    def recurrent(edges):
        return buf.recurrent_generator(adv, k_mb, L, chunks=cperm, edges=edges)

    for tag, make in (("feed_forward", feed_forward), ("recurrent", recurrent)):
        # outputs first: every minibatch, both tensors; the other bytes of a minibatch on the way
        nnz = graphs = other = 0
        for i, (x, y) in enumerate(zip(make(True), make(False))):
            ei, ea = lsm_edges.process_adj(y["adj"])
            if x["adj"] is not None or not torch.equal(x["edge_index"], ei) or not torch.equal(x["edge_attr"], ea):
                raise SystemExit("%s, %s layout: the edges of minibatch %d differ between edges=True and "
                                 "process_adj(batch['adj'])" % (tag, layout, i))
            if i == 0:
                graphs = y["adj"].shape[0]
                other = sum(2 * v.numel() * v.element_size() for k, v in y.items()
                            if v is not None and k not in ("adj", "indices", "chunks"))
                other += 8 * y["indices" if tag == "feed_forward" else "chunks"].numel()
            nnz += ea.shape[0]
            del ei, ea
        res["%s_outputs_equal" % tag] = True
        res["%s_graphs_per_minibatch" % tag] = graphs
        res["%s_edges_per_minibatch" % tag] = nnz / k_mb
        torch.cuda.empty_cache()

        def side_a():
            for x in make(True):
                pass

        def side_b():
            for y in make(False):
                lsm_edges.process_adj(y["adj"])

        side_a()
        side_b()
        t = alternated({"a": (side_a, REPS), "b": (side_b, REPS)})
        per_mb = lambda d: {k: (v / k_mb if k in ("median", "min", "max") else v) for k, v in d.items()}
        res["%s_edges_from_buffer_ms_per_minibatch" % tag] = per_mb(t["a"])
        res["%s_dense_then_process_adj_ms_per_minibatch" % tag] = per_mb(t["b"])
        dense = graphs * E * E * 4
        stored = dense if layout == "reference" else dense // N + graphs * 8 * W
        out = 20 * nnz // k_mb + 32 * graphs   # the edges; counts, scan and offsets
        bytes_a = other + 2 * stored + out
        bytes_b = other + stored + dense + 2 * dense + out
        res["%s_bytes_a" % tag], res["%s_bytes_b" % tag] = bytes_a, bytes_b
        res["%s_bytes_ratio_a_over_b" % tag] = bytes_a / bytes_b
        res["%s_time_ratio_a_over_b" % tag] = t["a"]["median"] / t["b"]["median"]
        spread = max(t["a"]["max"] - t["a"]["min"], t["b"]["max"] - t["b"]["min"])
        res["%s_target_met" % tag] = bool(t["a"]["median"] <= t["b"]["median"] + spread)
        print("%s %s: %.3f against %.3f ms per minibatch" % (layout, tag, t["a"]["median"] / k_mb,
                                                              t["b"]["median"] / k_mb), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    env.close()
    del buf, env, adv
    torch.cuda.empty_cache()
    return res


def main():
    from lsm.config import EnvArgs
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=EnvArgs().episode_length)
    ap.add_argument("--mini-batches", type=int, default=16)
    ap.add_argument("--layouts", default="reference,compact")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mb_edges_bench needs a GPU")
    out = {layout: bench_layout(layout, a, a.steps) for layout in a.layouts.split(",")}
    emit(out, a.out)


if __name__ == "__main__":
    main()
