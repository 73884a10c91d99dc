#!/usr/bin/env python
"""Record compute_returns / the advantage normalisation FROM THE REFERENCE ITSELF (build container only).

Imports the reference's own ``GraphReplayBuffer`` (onpolicy/utils/graph_buffer.py) and ``ValueNorm``
(onpolicy/utils/valuenorm.py) with ``oracle/ref_stubs`` first on the path and bytecode writing off, fills
a buffer with seeded random float32 rows, calls ``compute_returns`` in each of its eight branches
(use_gae x use_proper_time_limits x value normaliser) and then executes the advantage head of
``GR_MAPPO.train`` (onpolicy/algorithms/graph_mappo.py:258-268), read from the reference's file at
record time. One file per case under
``tests/golden/returns/``:

  inputs   rewards [T,n,N,1], value_preds_in / masks / bad_masks / active_masks [T+1,n,N,1], next_value
           [n,N,1], gamma, gae_lambda, use_gae, use_proper_time_limits, use_valuenorm,
           vn_mean / vn_var (ValueNorm.running_mean_var()), denorm = [sqrt(var), mean]
  outputs  returns, value_preds_out (after the call), adv_raw, adv_mean / adv_std (the reference's
           float32 nanmean / nanstd), adv_norm

masks / bad_masks hold about 30 % zeros (at least one in row T and one in row 1), active_masks about
20 %. Cases: T = 6, n = 3, N = 5 in all eight branches, and one T = 1 case.

Usage:  python tests/golden/make_returns_golden.py
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

OUT = os.path.join(HERE, "returns")
GAMMA, LAMBDA = 0.99, 0.95
# onpolicy/algorithms/graph_mappo.py, GR_MAPPO.train: the raw advantages, then their normalisation
RAW_LINES, NORM_LINES = (258, 263), (264, 268)


def reference_lines(first, last):
    """Lines first..last of the reference's graph_mappo.py, dedented and compiled."""
    import linecache
    import textwrap
    path = os.path.join(ref_harness.REF_ROOT, "onpolicy", "algorithms", "graph_mappo.py")
    src = textwrap.dedent("".join(linecache.getline(path, i) for i in range(first, last + 1)))
    assert "advantages" in src, "graph_mappo.py:%d-%d is not the advantage head" % (first, last)
    return compile(src, "%s:%d-%d" % (path, first, last), "exec")


def case_inputs(T, n, N, seed):
    rng = np.random.default_rng(seed)
    f32 = np.float32
    d = dict(rewards=rng.normal(0.0, 2.0, (T, n, N, 1)).astype(f32),
             value_preds_in=rng.normal(0.5, 1.5, (T + 1, n, N, 1)).astype(f32),
             next_value=rng.normal(0.5, 1.5, (n, N, 1)).astype(f32),
             masks=(rng.random((T + 1, n, N, 1)) >= 0.3).astype(f32),
             bad_masks=(rng.random((T + 1, n, N, 1)) >= 0.3).astype(f32),
             active_masks=(rng.random((T + 1, n, N, 1)) >= 0.2).astype(f32))
    for k in ("masks", "bad_masks"):
        d[k][T, 0, 1] = 0.0
        d[k][1, n - 1, 0] = 0.0
    d["active_masks"][0, 0, 0] = 0.0
    return d


def record(name, T, n, N, seed, use_gae, proper, use_vn):
    import torch
    from gym import spaces
    from onpolicy.utils.graph_buffer import GraphReplayBuffer
    from onpolicy.utils.valuenorm import ValueNorm
    args = argparse.Namespace(episode_length=T, n_rollout_threads=n, hidden_size=4, recurrent_N=1, gamma=GAMMA,
                              gae_lambda=LAMBDA, use_gae=use_gae, use_popart=False, use_valuenorm=use_vn,
                              use_proper_time_limits=proper, use_centralized_V=True)
    box = lambda *s: spaces.Box(-np.inf, np.inf, shape=s)
    buf = GraphReplayBuffer(args, N, box(6), box(6 * N), box(4, 3), box(1), box(N), box(4, 4), spaces.Discrete(25))
    d = case_inputs(T, n, N, seed)
    buf.rewards[:] = d["rewards"]
    buf.value_preds[:] = d["value_preds_in"]
    buf.masks[:] = d["masks"]
    buf.bad_masks[:] = d["bad_masks"]
    buf.active_masks[:] = d["active_masks"]
    vn = ValueNorm(1)
    vn.update(np.random.default_rng(seed + 1).normal(2.0, 3.0, (64, 1)).astype(np.float32))
    mean, var = vn.running_mean_var()
    buf.compute_returns(d["next_value"].copy(), vn if use_vn else None)

    # the advantage head of GR_MAPPO.train: the reference's own lines, read from its file at record
    # time and executed with its names bound (self, buffer, np)
    env = dict(np=np, buffer=buf,
               self=argparse.Namespace(_use_popart=False, _use_valuenorm=use_vn, value_normalizer=vn))
    exec(reference_lines(*RAW_LINES), env)      # advantages = returns[:-1] - denormalize(value_preds[:-1])
    adv_raw = env["advantages"].copy()
    exec(reference_lines(*NORM_LINES), env)     # the masked nanmean / nanstd normalisation
    advantages, mean_advantages, std_advantages = env["advantages"], env["mean_advantages"], env["std_advantages"]

    assert buf.returns.dtype == np.float32 and advantages.dtype == np.float32 and adv_raw.dtype == np.float32
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(
        path, gamma=np.float64(GAMMA), gae_lambda=np.float64(LAMBDA), use_gae=np.int32(use_gae),
        use_proper_time_limits=np.int32(proper), use_valuenorm=np.int32(use_vn),
        vn_mean=mean.numpy(), vn_var=var.numpy(),
        denorm=np.array([torch.sqrt(var).numpy()[0], mean.numpy()[0]], dtype=np.float32),
        returns=buf.returns, value_preds_out=buf.value_preds, adv_raw=adv_raw,
        adv_mean=np.float32(mean_advantages), adv_std=np.float32(std_advantages), adv_norm=advantages, **d)
    return path


def main():
    if not os.path.isdir(os.path.join(ref_harness.REF_ROOT, "onpolicy")):
        raise SystemExit("reference not available here")
    ref_harness._install_paths()
    total = 0
    for use_gae in (0, 1):
        for proper in (0, 1):
            for use_vn in (0, 1):
                p = record("t6_gae%d_ptl%d_vn%d" % (use_gae, proper, use_vn), 6, 3, 5, 20, bool(use_gae), bool(proper),
                           bool(use_vn))
                total += os.path.getsize(p)
    total += os.path.getsize(record("t1_gae1_ptl1_vn1", 1, 3, 5, 21, True, True, True))
    print("wrote 9 files under", OUT, total // 1024, "KB")


if __name__ == "__main__":
    main()
