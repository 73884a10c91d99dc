#!/usr/bin/env python
"""Record recurrent_generator's minibatches FROM THE REFERENCE ITSELF (build container only).

Imports the reference's own ``GraphReplayBuffer`` (onpolicy/utils/graph_buffer.py) with
``oracle/ref_stubs`` first on the path and bytecode writing off, fills every field of a buffer with
seeded random rows, records ``torch.randperm(data_chunks)`` under ``torch.manual_seed(s)``, reseeds and
runs ``recurrent_generator`` (graph_buffer.py:597-755), which then draws that same permutation. One file
per case under ``tests/golden/recurrent/``:

  inputs   T, n, N, E, L (data_chunk_length), num_mini_batch, recurrent_N, use_centralized_V, perm
           [data_chunks] int64, and in_<field> for share_obs, obs, node_obs, adj, agent_id,
           share_agent_id, rnn_states, rnn_states_critic, actions, action_log_probs, value_preds,
           returns, masks, active_masks, available_actions (the buffer's arrays, all rows) and
           advantages [T,n,N,1]; adj_table [T+1,n,E,E] and adj_bits [T+1,n,N,E]: the compact statement
           in_adj was built from (in_adj[t,e,a][r][c] = 0 where bit r or bit c of adj_bits[t,e,a] is set,
           else adj_table[t,e][r][c]; in some (t, e) every agent has the last bit set)
  outputs  b<i>_<name> for minibatch i and every array the generator yields, under the names of
           NAMES below (its yield order)

masks hold about 30 % zeros, active_masks about 20 %. Cases, all n = 3, N = 5, E = 4, T = 6: L = 4 with
recurrent_N = 2 (chunks straddle two series and the tail is dropped), L = 3, L = 1, L = T, and L = 4
without the centralized critic.

Usage:  python tests/golden/make_recurrent_golden.py
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)

from oracle import ref_harness  # noqa: E402

OUT = os.path.join(HERE, "recurrent")
# GraphReplayBuffer.recurrent_generator's yield order (graph_buffer.py:751-755)
NAMES = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "rnn_states", "rnn_states_critic",
         "actions", "value_preds", "returns", "masks", "active_masks", "action_log_probs", "advantages",
         "available_actions")
E, F, OBS, HIDDEN, ACTIONS = 4, 3, 6, 4, 25


def fill(buf, rng, n, N):
    """Seeded random rows in every field the generator reads. Returns (advantages, adj_table, adj_bits)."""
    f32 = np.float32
    for k in ("share_obs", "obs", "node_obs", "rnn_states", "rnn_states_critic", "action_log_probs", "value_preds",
              "returns"):
        a = getattr(buf, k)
        a[:] = rng.normal(0.0, 1.0, a.shape).astype(f32)
    for k in ("agent_id", "share_agent_id"):
        a = getattr(buf, k)
        a[:] = rng.integers(0, N, a.shape).astype(np.int32)
    buf.actions[:] = rng.integers(0, ACTIONS, buf.actions.shape).astype(f32)
    buf.available_actions[:] = (rng.random(buf.available_actions.shape) >= 0.25).astype(f32)
    buf.masks[:] = (rng.random(buf.masks.shape) >= 0.3).astype(f32)
    buf.active_masks[:] = (rng.random(buf.active_masks.shape) >= 0.2).astype(f32)
    T1 = buf.adj.shape[0]
    table = rng.normal(0.0, 1.0, (T1, n, E, E)).astype(f32)
    table[table == 0] = 1.0
    bits = rng.random((T1, n, N, E)) < 0.25
    for t in range(T1):
        for e in range(n):
            if (t + e) % 2 == 0:
                bits[t, e, :, E - 1] = True   # an entity no agent of this env is connected to
    drop = bits[..., :, None] | bits[..., None, :]
    buf.adj[:] = np.where(drop, f32(0), table[:, :, None])
    adv = rng.normal(0.0, 1.0, buf.rewards.shape).astype(f32)
    return adv, table, bits


def record(name, T, n, N, L, k, seed, recurrent_N=1, centralized=True):
    import torch
    from gym import spaces
    from onpolicy.utils.graph_buffer import GraphReplayBuffer
    args = argparse.Namespace(episode_length=T, n_rollout_threads=n, hidden_size=HIDDEN, recurrent_N=recurrent_N,
                              gamma=0.99, gae_lambda=0.95, use_gae=True, use_popart=False, use_valuenorm=False,
                              use_proper_time_limits=False, use_centralized_V=centralized)
    box = lambda *s: spaces.Box(-np.inf, np.inf, shape=s)
    buf = GraphReplayBuffer(args, N, box(OBS), box(OBS * N if centralized else OBS), box(E, F), box(1), box(N),
                            box(E, E), spaces.Discrete(ACTIONS))
    adv, table, bits = fill(buf, np.random.default_rng(seed), n, N)
    assert bits.all(axis=2).any()
    data_chunks = T * n * N // L
    torch.manual_seed(seed)
    perm = torch.randperm(data_chunks).numpy().astype(np.int64)
    torch.manual_seed(seed)
    d = {}
    count = 0
    for i, batch in enumerate(buf.recurrent_generator(adv, k, L)):
        assert len(batch) == len(NAMES)
        for nm, a in zip(NAMES, batch):
            d["b%d_%s" % (i, nm)] = np.ascontiguousarray(a)
        count += 1
    assert count == k
    mb = data_chunks // k
    assert d["b0_obs"].shape == (L * mb, OBS) and d["b0_rnn_states"].shape == (mb, recurrent_N, HIDDEN)
    for nm in NAMES:
        src = adv if nm == "advantages" else getattr(buf, nm)
        d["in_" + nm] = src.copy()
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, T=np.int32(T), n=np.int32(n), N=np.int32(N), E=np.int32(E), L=np.int32(L),
                        num_mini_batch=np.int32(k), recurrent_N=np.int32(recurrent_N),
                        use_centralized_V=np.int32(centralized), perm=perm, adj_table=table, adj_bits=bits, **d)
    return path, perm


def main():
    if not os.path.isdir(os.path.join(ref_harness.REF_ROOT, "onpolicy")):
        raise SystemExit("reference not available here")
    ref_harness._install_paths()
    T, n, N = 6, 3, 5
    cases = [("t6_l4_mb2_rn2", 4, 2, 30, dict(recurrent_N=2)), ("t6_l3_mb3", 3, 3, 31, {}),
             ("t6_l1_mb2", 1, 2, 32, {}), ("t6_l6_mb3", 6, 3, 33, {}),
             ("t6_l4_mb2_decv", 4, 2, 34, dict(centralized=False))]
    total = 0
    for name, L, k, seed, kw in cases:
        path, perm = record(name, T, n, N, L, k, seed, **kw)
        used = perm[:(len(perm) // k) * k]
        straddles = ((used * L) % T + L > T).any()
        if name == "t6_l4_mb2_rn2":
            # some drawn chunk runs past the end of its (env, agent) series, and 90 samples leave a tail
            assert straddles and (T * n * N) % L != 0
        if L in (1, 3, 6):
            assert not straddles
        total += os.path.getsize(path)
    print("wrote %d files under" % len(cases), OUT, total // 1024, "KB")


if __name__ == "__main__":
    main()
