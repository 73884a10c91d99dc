"""Device time of the learner hand-off (csrc/lsm_returns.hip, csrc/lsm_gather.hip) at the headline shape
(4096 envs x 8 agents, T = EnvArgs().episode_length), against a torch-ops statement of the same work
on the device: the T-step loop of elementwise ops plus the masked mean / std for compute_returns +
advantages, and one index_select per field for a minibatch. HIP events around repeated calls on an
otherwise idle stream, after a warm-up of every shape; the outputs of the two sides are compared first
and a difference ends the run. The two sides are timed in alternating rounds and the median, minimum and
maximum of the rounds are recorded.

    python layered-safe-marl_amd/tools/returns_bench.py [--envs 4096] [--steps T] [--mini-batches 16] [--out FILE]

The gather's bytes are the algorithm's: per sample and field one row read and one row written, plus the
8-byte index; for the compact adjacency E*E*4 written, E*E*4 / N read (a table serves N samples) and
the mask words. The compact layout has no torch baseline: its samples exist only through the expansion.
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, emit  # noqa: E402

GAMMA, LAMBDA = 0.99, 0.95
DEN = (2.85, 2.04)


def torch_returns_advantages(buf, next_value, den):
    """compute_returns (GAE, value normaliser) and the advantage head as torch ops on the device."""
    import torch
    s, mu = den
    v, r, m = buf.value_preds, buf.rewards, buf.masks
    ret = torch.empty_like(buf.returns)
    v[-1] = next_value
    gae = torch.zeros_like(next_value)
    for t in reversed(range(buf.T)):
        dv = v[t] * s + mu
        delta = r[t] + GAMMA * (v[t + 1] * s + mu) * m[t + 1] - dv
        gae = delta + GAMMA * LAMBDA * m[t + 1] * gae
        ret[t] = gae + dv
    adv = ret[:-1] - (v[:-1] * s + mu)
    act = buf.active_masks[:-1] != 0
    x = adv.double()
    cnt = act.sum()
    mean = torch.where(act, x, 0.0).sum() / cnt
    std = torch.sqrt(torch.where(act, (x - mean) ** 2, 0.0).sum() / cnt)
    return ret, (adv - mean.float()) / (std.float() + 1e-5)


def gather_bytes(buf, B):
    env = buf.env
    total = 8 * B
    for k, t, shape in buf._gather_sources(buf.returns[:-1]):
        row = t.element_size()
        for d in shape:
            row *= d
        if k == "adj" and buf.adj_mask is not None:
            total += B * (row + row // env.N + 8 * buf.adj_mask.shape[-1])
        else:
            total += 2 * B * row
    return total


def bench_layout(layout, a, T):
    import torch
    from lsm import hj_tables
    from lsm.buffer import DeviceGraphBuffer
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    dev = "cuda:0"
    n, N = a.envs, 8
    args = EnvArgs(num_agents=N, episode_length=T, num_env_steps=T * 4, use_safety_filter=True, seed=0)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    env = GpuGraphVecEnv(args, num_envs=n, device=dev, value_table=vt, return_numpy=False, build_infos=False,
                         adj_layout=layout)
    buf = DeviceGraphBuffer(env, episode_length=T)
    g = torch.Generator(device=dev).manual_seed(1)
    buf.warmup(4)
    for _ in range(T):
        acts = torch.randint(0, 25, (n, N), generator=g, device=dev, dtype=torch.int32)
        buf.insert_step(acts, 4, value_preds=torch.randn((n, N), generator=g, device=dev))
    next_value = torch.randn((n, N, 1), generator=g, device=dev)
    batch = T * n * N
    res = {"layout": layout, "envs": n, "agents": N, "T": T, "E": env.E, "samples": batch}

    # the normaliser as a device tensor: a (scale, mean) pair of Python numbers would add a blocking upload
    den_t = torch.tensor(DEN, dtype=torch.float32, device=dev)

    def hip_returns():
        buf.compute_returns(next_value, den_t, gamma=GAMMA, gae_lambda=LAMBDA)

    def hip_ra():
        hip_returns()
        return buf.advantages(den_t)

    adv, _ = hip_ra()
    if layout == "reference":
        t_ret, t_adv = torch_returns_advantages(buf, next_value, DEN)
        res["returns_max_abs_diff_vs_torch"] = float((t_ret[:-1] - buf.returns[:-1]).abs().max())
        res["advantages_max_abs_diff_vs_torch"] = float((t_adv - adv).abs().max())
        if res["returns_max_abs_diff_vs_torch"] > 1e-5 or res["advantages_max_abs_diff_vs_torch"] > 1e-5:
            raise SystemExit("the torch statement and the HIP path disagree: %r" % res)
        del t_ret, t_adv
        for _ in range(3):
            hip_ra()
        torch_returns_advantages(buf, next_value, DEN)
        # the working set (about 16 B x T x M, 130 MB at the headline shape) is re-read every call, so it
        # stays warm in the 256 MB last-level cache on both sides: these are not cold-HBM times
        t = alternated({"hip": (hip_ra, 500), "hip_returns_only": (hip_returns, 500),
                        "torch": (lambda: torch_returns_advantages(buf, next_value, DEN), 8)})
        res["hip_returns_advantages_ms"] = t["hip"]
        res["hip_returns_only_ms"] = t["hip_returns_only"]
        res["torch_returns_advantages_ms"] = t["torch"]

    perm = torch.randperm(batch, generator=g, device=dev)
    flat = {}
    if layout == "reference":
        flat = {k: t[:-1].reshape((batch,) + tuple(t.shape[3:])) if t.shape[0] == T + 1 else t.reshape((batch, 1))
                for k, t, _ in buf._gather_sources(adv)}
    for k_mb in (1, a.mini_batches):
        mb = batch // k_mb
        tag = "mb%d" % k_mb
        # the generator's per-minibatch work alone (its once-per-generator permutation check and output
        # allocation are not part of a minibatch): the plan is built once, the k_mb launches are timed
        plan = buf._gather_plan(adv, mb)

        def hip_gather():
            for i in range(k_mb):
                buf._gather(plan, perm[i * mb:(i + 1) * mb])

        def torch_gather():
            for i in range(k_mb):
                idx = perm[i * mb:(i + 1) * mb]
                for t in flat.values():
                    torch.index_select(t, 0, idx)

        if layout == "reference":   # same rows from both
            first = buf._gather(plan, perm[:mb])
            for k, t in flat.items():
                if not torch.equal(first[k], torch.index_select(t, 0, perm[:mb])):
                    raise SystemExit("gather of %s differs from index_select" % k)
            res["gather_%s_equals_index_select" % tag] = True
            del first
            torch_gather()
        hip_gather()
        reps = 10   # a call covers the whole buffer in k_mb launches: about 0.13 s per round and side
        sides = {"hip": (hip_gather, reps)}
        if layout == "reference":
            sides["torch"] = (torch_gather, reps)
        t = alternated(sides)
        nbytes = gather_bytes(buf, mb)
        per_mb = lambda d: {k: (v / k_mb if k in ("median", "min", "max") else v) for k, v in d.items()}
        res["hip_gather_%s_ms_per_minibatch" % tag] = per_mb(t["hip"])
        res["hip_gather_%s_bytes" % tag] = nbytes
        res["hip_gather_%s_TBps" % tag] = nbytes / (t["hip"]["median"] / k_mb * 1e-3) / 1e12
        if layout == "reference":
            res["torch_index_select_%s_ms_per_minibatch" % tag] = per_mb(t["torch"])
            res["torch_index_select_%s_TBps" % tag] = nbytes / (t["torch"]["median"] / k_mb * 1e-3) / 1e12
        del plan
        torch.cuda.empty_cache()
    env.close()
    del buf, env, flat, adv
    torch.cuda.empty_cache()
    return res


def main():
    from lsm.config import EnvArgs
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=EnvArgs().episode_length)
    ap.add_argument("--mini-batches", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("returns_bench needs a GPU")
    out = {"reference": bench_layout("reference", a, a.steps), "compact": bench_layout("compact", a, a.steps)}
    emit(out, a.out)


if __name__ == "__main__":
    main()
