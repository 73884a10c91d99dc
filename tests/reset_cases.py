"""The env sets of the all-env reset tests (test infrastructure), shared by the CPU side
(tests/test_reset_truth.py: the truth's own properties and the coverage condition) and the GPU side
(tests/test_gpu_all_env_resets.py).

One CONFIG is an env set: its meta, a prime env count (every team size and every envs-per-wave
packing leaves a partly filled last workgroup / wave), the step count, the envs driven all-done
early (`early`: step -> envs injected after that step, so that they reset at the next one, off the
common episode boundary), and the kernel variants ("families") that run it with the same seeds and
actions. How often each env resets follows from the steps and the injections (reset_schedule); the
truth holds that many reset indices per env (n_resets). A "philox" entry overrides fields for that
stream.
"""
from __future__ import annotations

import numpy as np

SEED = 21
EP = 4
EPISODE_LENGTH = 6


def _meta(dyn, n, **kw):
    ws = 4 if dyn == "double_integrator" else 6
    return dict(dynamics_type=dyn, num_agents=n, num_landmarks=2, world_size=ws, episode_length=EPISODE_LENGTH,
                num_env_steps=EPISODE_LENGTH * 4, n_rollout_threads=1, use_safety_filter=True, use_masking=True,
                num_internal_step=1, seed=SEED, env_seed=SEED, **kw)


# a family: the kernel the dispatch must choose, its kernel_select, the adjacency layout, and the
# MT19937 words a team-kernel lane may take from the staged blocks (lsm_test_set_mt_stage) or None
def _fam(kernel, ksel=None, layout="reference", stage=None):
    return dict(kernel=kernel, ksel=ksel or {}, layout=layout, stage=stage)


CONFIGS = {
    # double integrator, N = 8: steps 0 .. 19, episode ends at steps 5, 11, 17; some envs all-done early
    "di8": dict(meta=_meta("double_integrator", 8), n_envs=1021, steps=20,
                early={2: (0, 5, 9, 100, 517, 1020), 8: (3, 5, 64, 1016, 1019), 13: (7, 8, 14, 511, 1020)},
                families={"t8": _fam("rollout_team_kernel<0, 8, 8, false>", {"team": 8}), "t4": _fam("rollout_team_kernel<0, 8, 4, false>", {"team": 4}),
                          "t2": _fam("rollout_team_kernel<0, 8, 2, false>", {"team": 2}),
                          "t4s": _fam("rollout_team_kernel<0, 8, 4, false>", {"team": 4}, stage=40),
                          "wave": _fam("rollout_kernel<0, 64, 8>", {"team": 0}),
                          "generic": _fam("rollout_kernel<0, 64, 0>", {"generic": 1, "lanes_per_env": 64}),
                          "block": _fam("rollout_block_kernel<0, 0, true, false>", {"workgroup_per_env": 1}),
                          "blockc": _fam("rollout_block_kernel<0, 0, true, false>", {"workgroup_per_env": 1},
                                         layout="compact")}),
    # (all-done injection is the double integrator's: an airtaxi agent cannot be put at rest on a goal)
    "at16": dict(meta=_meta("airtaxi", 16), n_envs=509, steps=20, early={},
                 families={"t4": _fam("rollout_team_kernel<1, 16, 4, false>", {"team": 4}),
                           "t2": _fam("rollout_team_kernel<1, 16, 2, false>", {"team": 2}),
                           "wave": _fam("rollout_kernel<1, 64, 16>", {"team": 0}),
                           "block": _fam("rollout_block_kernel<1, 0, true, false>", {"workgroup_per_env": 1})}),
    # 4 and 2 envs per wave. A reset of 3 agents draws 68 .. 120 words, so four of them stay inside
    # the first 624-word block: 54 steps (ten resets) take every env across a block boundary
    # Envs driven all-done early at several phases: env 0 alone in wave 0, envs 5 and 6 of wave 1
    # (envs 4 .. 7) together, 1017 in the last full wave, 1020 alone in the partly filled last wave;
    # some twice, so that a wave's envs end up in three different phases
    "di3": dict(meta=_meta("double_integrator", 3), n_envs=1021, steps=54,
                early={2: (0, 5, 6, 1020), 8: (3, 9, 514), 13: (0, 1017), 21: (5, 258, 1020), 32: (2, 6, 771),
                       44: (10, 1017)},
                families={"lpe16": _fam("rollout_kernel<0, 16, 0>", {"lanes_per_env": 16})}),
    # two envs per wave: 0 of (0, 1), both of (4, 5), 1019 of (1018, 1019), 1020 alone in the last wave
    "di5": dict(meta=_meta("double_integrator", 5), n_envs=1021, steps=54,
                early={2: (0, 4, 5, 1020), 8: (3, 9, 514), 13: (0, 1019), 21: (4, 258, 1020), 32: (2, 7, 771),
                       44: (10, 1019)},
                families={"lpe32": _fam("rollout_kernel<0, 32, 0>", {"lanes_per_env": 32})}),
    # the workgroup-per-env kernels chosen automatically (E = 192; E = 99: the generic one), compact
    # layout read through reference_adj(). A workgroup holds one env there, so no workgroup can hold
    # resetting and non-resetting envs and none is driven all-done early. MT19937: two resets (the
    # first, and the episode end at step 5); Philox: 20 steps, reset indices 0 .. 3
    "di64": dict(meta=_meta("double_integrator", 64), n_envs=61, steps=8, early={}, philox=dict(steps=20),
                 families={"blockc": _fam("rollout_block_kernel<0, 64, true, false>", layout="compact")}),
    "di33": dict(meta=_meta("double_integrator", 33), n_envs=61, steps=8, early={}, philox=dict(steps=20),
                 families={"blockc": _fam("rollout_block_kernel<0, 0, true, false>", layout="compact")}),
}

# (config, family, rng): every family in numpy's MT19937 stream, and each once more in Philox
GPU_CASES = [(c, f, r) for r in ("mt19937", "philox") for c, cfg in CONFIGS.items() for f in cfg["families"]
             if not (r == "philox" and cfg["families"][f]["stage"] is not None)]   # the stage is MT19937's


def case(name, rng="mt19937"):
    """CONFIGS[name] as it runs in stream rng."""
    cfg = dict(CONFIGS[name])
    if rng == "philox":
        cfg.update(cfg.get("philox", {}))
    return cfg


# resets every env of a config is compared at whatever the actions do: the first one and the
# episode ends inside `steps` (the coverage condition counts only these)
def sure_resets(cfg):
    return 1 + cfg["steps"] // EPISODE_LENGTH


def reset_schedule(cfg):
    """{env: [steps at which it resets]} for the envs driven all-done early (an injection after step
    t makes step t + 1 reach every final goal; an episode otherwise ends EPISODE_LENGTH steps after
    its reset), and the common schedule of all other envs under the key None."""
    def steps_of(inj):
        out, left = [], EPISODE_LENGTH
        for t in range(cfg["steps"]):
            left -= 1
            if left == 0 or (t - 1) in inj:
                out.append(t)
                left = EPISODE_LENGTH
        return out
    sched = {None: steps_of(())}
    for k in sorted({k for ks in cfg["early"].values() for k in ks}):
        sched[k] = steps_of({t for t, ks in cfg["early"].items() if k in ks})
    return sched


def n_resets(cfg):
    """Reset indices the truth holds per env: the first reset and the most resets any env makes."""
    return 1 + max(len(v) for v in reset_schedule(cfg).values())


def actions(name, rng="mt19937"):
    """int32 [steps, n_envs, N]: the config's random actions, the same for every family. An env
    driven all-done early gets zero acceleration (index 12) at the step after the injection."""
    cfg = case(name, rng)
    import zlib
    a = np.random.default_rng(zlib.crc32(name.encode())).integers(
        0, 25, (cfg["steps"], cfg["n_envs"], cfg["meta"]["num_agents"])).astype(np.int32)
    for t, ks in cfg["early"].items():
        a[t + 1, list(ks)] = 12
    return a


def arrive_all_state(lm, N, L):
    """Every agent on its last goal at the goal's speed and heading, reached_goal = L - 1
    (make_golden.py's inject_goal_arrival for all agents; test_gpu_parity._arrive_all): with zero
    acceleration the next step reaches every final goal, so the env is all-done early.
    lm: [N L, 4] landmark x, y, heading, speed."""
    st = np.zeros((N, 4))
    for i in range(N):
        x, y, h, sp = lm[(L - 1) * N + i]
        st[i] = [x, y, sp * np.cos(h), sp * np.sin(h)]
    return st, np.full(N, L - 1, dtype=np.int32)


F32_ATOL, STATE_ATOL = 1e-5, 1e-9   # the project's parity bounds (tests/test_gpu_parity.py)
REW_RTOL, REW_ATOL = 1e-6, 1e-5


def replay(name, rng, k, r, t0, t, acts):
    """The arbiter of a disagreement between two families: the oracle's outputs of env k at step t,
    its reset index r reached by resets alone, then the actions of steps t0 + 1 .. t (t0: the step of
    that reset, -1 for the first), with the all-done injections of the config."""
    from golden_replay import table_dict, tables_for
    from oracle.lsm_oracle import OracleVecEnv
    from oracle_pool import _source
    cfg = case(name, rng)
    meta = cfg["meta"]
    N, L = meta["num_agents"], meta["num_landmarks"]
    vt, tt = tables_for(meta)
    ora = OracleVecEnv(meta, 1, seed=SEED, value_table=table_dict(vt), ttr_table=table_dict(tt),
                       integrator="restated", seed_offset=k, rng=lambda s: _source(rng, s))
    e = ora.envs[0]

    def inject():
        st, reached = arrive_all_state(np.column_stack([e.lm_pos, e.lm_heading, e.lm_speed]), N, L)
        e.s[:] = st
        e.reached_goal[:] = reached
        e.calculate_distances()

    for _ in range(r + 1):
        o = ora.reset(EP)
    if k in cfg["early"].get(t0, ()):
        inject()
    for s in range(t0 + 1, t + 1):
        o = ora.step(acts[s][k][None], EP)
        if k in cfg["early"].get(s, ()) and s < t:
            inject()
    return step_outputs(o, e, N)


def step_outputs(o, e, N):
    """One env's outputs of an OracleVecEnv step as the arbiter compares them."""
    return dict(obs=np.asarray(o[0][0], np.float32), node=np.asarray(o[2][0], np.float32),
                adj=np.asarray(o[3][0], np.float32), rew=np.asarray(o[4][0], np.float64).reshape(-1),
                dones=np.asarray(o[5][0], bool), reset=len(o[6][0]) > N, state=e.s.copy())


def within_project_tolerance(g, want):
    """(ok, why): one env's outputs g of one step against the oracle's `want` at the project's bounds."""
    try:
        np.testing.assert_array_equal(g["dones"], want["dones"])
        assert bool(g["reset"]) == bool(want["reset"]), "reset flag"
        np.testing.assert_array_equal(g["adj"] != 0, want["adj"] != 0)
        np.testing.assert_allclose(g["obs"], want["obs"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g["node"], want["node"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g["adj"], want["adj"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g["rew"], want["rew"], rtol=REW_RTOL, atol=REW_ATOL)
        np.testing.assert_allclose(g["state"], want["state"], rtol=0, atol=STATE_ATOL)
    except AssertionError as err:
        return False, str(err)
    return True, ""
