"""Every env of a full-size GPU run against the oracle (test infrastructure).

The full-size parity tests (BASELINE configs 3 and 4) compare ALL envs of a launch with the oracle
over the first steps after a reset, on the full-shape synthetic HJ / TTR tables the bench times
(``lsm.hj_tables.default_tables``, ``bench.py``). One oracle env-step costs ~4 ms (DI, N = 8) to
~36 ms (airtaxi, N = 16) on one core, so the envs are split over worker processes. Workers are
started with the "spawn" method: fresh interpreters that never touch the GPU (the test process has
initialised it; forked children would inherit its device handles). Each worker rebuilds the tables
(deterministic, ~2 s) and runs its envs one at a time (an oracle env copies its 20-25 MB value table,
as HjDataHandle shifts it in place, so thousands cannot be alive at once).

run_all_resets is the truth of tests/test_gpu_all_env_resets.py: every env doing nothing but reset, with
the draw counts of each reset, in numpy's MT19937 stream or fed from the Philox stream function.
"""
from __future__ import annotations

import multiprocessing as mp
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(dyn):
    sys.path.insert(0, os.path.join(ROOT, "layered-safe-marl_amd"))
    from lsm import hj_tables
    from golden_replay import table_dict
    vt, tt = hj_tables.default_tables(dyn)
    return table_dict(vt), table_dict(tt)


def _chunk(job):
    meta, seed, k0, k1, ep, actions = job
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle.lsm_oracle import OracleVecEnv
    vt, tt = _tables(meta["dynamics_type"])
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    S = actions.shape[1]
    out = dict(reset_obs=[], reset_adj=[], state=[], obs=[], adj=[], dones=[], rew=[])
    for k in range(k0, k1):
        ora = OracleVecEnv(meta, 1, seed=seed, value_table=vt, ttr_table=tt, integrator="restated",
                           seed_offset=k)
        r = ora.reset(ep)
        out["reset_obs"].append(f32(r[0][0]))
        out["reset_adj"].append(np.packbits(np.asarray(r[3][0]) != 0))
        st, ob, ad, dn, rw = [], [], [], [], []
        for s in range(S):
            o = ora.step(actions[k - k0, s][None], ep)
            ob.append(f32(o[0][0]))
            ad.append(np.packbits(np.asarray(o[3][0]) != 0))
            dn.append(np.asarray(o[5][0], dtype=bool))
            rw.append(f32(o[4][0]))
            st.append(ora.envs[0].s.copy())
        out["obs"].append(np.stack(ob))
        out["adj"].append(np.stack(ad))
        out["dones"].append(np.stack(dn))
        out["rew"].append(np.stack(rw))
        out["state"].append(np.stack(st))
        del ora
    return k0, {k: np.stack(v) for k, v in out.items()}


def philox_source(seed):
    """DrawSource of one env under LSM_RNG_PHILOX: at its r-th reset, uniform answers from
    lsm_host_philox_uniforms(seed, r, ...) in draw order (the stream function tests/test_capi.py pins
    to Random123's known answers). The stream is counter-based, so a longer request repeats the
    shorter one's prefix."""
    from oracle.lsm_oracle import DrawSource
    from lsm import capi
    lib = capi.load_library()

    class PhiloxSource(DrawSource):
        def __init__(self, seed):
            super().__init__(seed)
            self._r, self._pos, self._buf = -1, 0, np.zeros(0)

        def _fill(self, count):
            self._buf = np.zeros(count)
            rc = lib.lsm_host_philox_uniforms(self.seed, self._r, count, 0.0, 1.0, self._buf.ctypes.data)
            assert rc == 0

        def begin_reset(self):
            super().begin_reset()
            self._r += 1
            self._pos = 0
            self._fill(1024)

        def _doubles(self, n):
            if self._pos + n > len(self._buf):
                self._fill(2 * (self._pos + n))
            d = self._buf[self._pos:self._pos + n]
            self._pos += n
            return d

    return PhiloxSource(seed)


def _source(rng, seed):
    from oracle.lsm_oracle import DrawSource
    if rng == "mt19937":
        return DrawSource(seed)
    if rng == "philox":
        return philox_source(seed)
    raise ValueError("rng must be 'mt19937' or 'philox'")


def resets_of_env(meta, seed_k, ep, resets, rng, vt, tt, outputs=True):
    """Env with seed seed_k doing nothing but reset(ep) `resets` times. What env k shows after its
    r-th reset depends only on (seed + 1000 k, r, ep): the oracle draws only while it resets
    (tests/test_reset_truth.py pins that). outputs=False: only the draw counts (the scenario draw
    alone, no observations)."""
    from oracle.lsm_oracle import DrawSource, OracleEnv
    f32 = lambda x: np.asarray(x, dtype=np.float32)
    src = _source(rng, seed_k)
    e = OracleEnv(meta, seed_k, vt, tt, integrator="restated", rng=src)
    out = dict(obs=[], node=[], adj=[], state=[], lm=[])
    for r in range(resets):
        if not outputs:
            e.update_curriculum(ep)
            src.begin_reset()
            e.random_scenario()
            continue
        o = e.reset(ep)
        adj = f32(o[3])
        # the reset's mask (done, departed, reached goals) is the same for every ego, so the N ego
        # adjacencies are one matrix: kept once, as float32 values (N = 64 is 147 KB per env and reset
        # so, against 9.4 MB for the N copies: small enough to hold every env at once, and the nonzero
        # pattern is read off the values)
        assert all(np.array_equal(adj[0], a) for a in adj[1:]), "ego adjacencies differ at a reset"
        out["obs"].append(f32(o[0]))
        out["node"].append(f32(o[2]))
        out["adj"].append(adj[0])
        out["state"].append(e.s.copy())
        out["lm"].append(np.column_stack([e.lm_pos, e.lm_heading, e.lm_speed]))
    res = {k: np.stack(v) for k, v in out.items()} if outputs else {}
    res["words"] = np.array([x["words"] for x in src.log], dtype=np.int64)
    res["start"] = np.array([x["start"] for x in src.log], dtype=np.int64)
    res["redraws"] = np.array([x["redraws"] for x in src.log], dtype=np.int64)
    res["longest"] = np.array([x["longest"] for x in src.log], dtype=np.int64)
    res["crosses"] = np.array([DrawSource.crosses_block(x) for x in src.log], dtype=bool)
    return res


def _reset_chunk(job):
    meta, seed, k0, k1, ep, resets, rng, outputs = job
    for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "layered-safe-marl_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from golden_replay import table_dict, tables_for
    vt, tt = tables_for(meta)   # a reset reads no table; the oracle env wants them for its steps
    vt, tt = table_dict(vt), table_dict(tt)
    parts = [resets_of_env(meta, seed + 1000 * k, ep, resets, rng, vt, tt, outputs) for k in range(k0, k1)]
    return k0, {key: np.stack([p[key] for p in parts]) for key in parts[0]}


def run_all_resets(meta, seed, n_envs, ep, resets, rng="mt19937", workers=None, outputs=True):
    """Reset truth of envs [0, n_envs) (seed + 1000 k), reset indices r = 0 .. resets - 1, from the
    oracle in spawned workers (they never touch the GPU). rng: "mt19937" (numpy's legacy stream, the
    reference's) or "philox" (philox_source). Returns arrays with leading axes [env, r]: obs f32
    [., ., N, OBS], node f32 [., ., N, E, F], adj f32 [., ., E, E] (one matrix for all egos of a reset),
    state f64 [., ., N, 4], lm f64 [., ., N L, 4] (landmark x, y, heading, speed), and the draw counts
    words, start (stream position in words at the reset's first draw), redraws, longest (the highest
    attempt index of one rejection loop), crosses (a 624-word block boundary inside the reset's
    draws). outputs=False: the counts alone. The largest set the tests ask for (61 envs x 4 resets at
    N = 64) is 150 MB, so everything is returned at once."""
    # the Philox workers load the project's library for its host stream function: they make no
    # device call, and are still kept few enough to stay under any limit on processes with the library
    workers = workers or workers_for_box(cap=12 if rng == "philox" else 16)
    chunk = max(1, -(-n_envs // (workers * 4)))
    jobs = [(dict(meta), seed, a, min(n_envs, a + chunk), ep, resets, rng, outputs)
            for a in range(0, n_envs, chunk)]
    ctx = mp.get_context("spawn")
    with ctx.Pool(min(workers, len(jobs))) as pool:
        parts = pool.map(_reset_chunk, jobs)
    return {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}


def workers_for_box(cap=16):
    """Worker processes: the job's CPU share (the affinity set, capped by a cgroup quota; a GPU box
    lends each GPU a share of a larger host), at most `cap`."""
    n = len(os.sched_getaffinity(0))
    try:
        q, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            n = max(1, min(n, int(int(q) // int(period))))
    except Exception:
        pass
    return max(1, min(cap, n))


def run_all_envs(meta, seed, n_envs, ep, actions, workers=None):
    """Oracle of envs [0, n_envs) (seed + 1000 k): reset(ep), then actions[k, s] for s < S.
    actions: int [n_envs, S, N]. Returns dict of arrays with a leading env axis: reset_obs f32
    [n, N, OBS], reset_adj packed bits, then per step: obs, adj (packed bits of adj != 0), dones,
    rew (f32), state (f64 [n, S, N, 4])."""
    workers = workers or workers_for_box()
    edges = np.linspace(0, n_envs, workers * 4 + 1).astype(int)   # several chunks per worker
    jobs = [(dict(meta), seed, int(a), int(b), ep, np.ascontiguousarray(actions[a:b]))
            for a, b in zip(edges[:-1], edges[1:]) if b > a]
    ctx = mp.get_context("spawn")
    with ctx.Pool(workers) as pool:
        parts = sorted(pool.map(_chunk, jobs), key=lambda x: x[0])
    return {k: np.concatenate([p[1][k] for p in parts]) for k in parts[0][1]}
