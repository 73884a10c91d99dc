"""The reset truth of tests/test_gpu_all_env_resets.py, checked on the CPU.

* The oracle draws random numbers only while it resets, so what env k shows after its r-th reset
  depends only on (seed + 1000 k, r, ep). Pinned here: a stepped oracle's post-reset outputs equal,
  bit for bit, those of an oracle that only resets (oracle_pool.resets_of_env). If the oracle ever
  draws during a step, this fails first.
* The Philox-fed oracle (oracle_pool.philox_source) at reset index 0 equals the project's host
  restatement lsm_host_scenario(LSM_RNG_PHILOX) exactly, for every env of the GPU cases' env sets.
* The envs the GPU cases drive all-done early reset exactly when reset_cases.reset_schedule says, and the
  arbiter of a disagreement between two kernel families (reset_cases.replay) reproduces a plainly
  stepped oracle at every step, injections included, in both streams.
* The coverage condition: over each GPU case's env set and reset count, the rare branches of the
  device's staged MT19937 draw occur at least 8 times each, counted from the oracle alone.
"""
import ctypes as C
import math

import numpy as np
import pytest

from golden_replay import table_dict, tables_for
from reset_cases import CONFIGS, EP, SEED, actions, arrive_all_state, case, replay, reset_schedule, step_outputs, \
    sure_resets, within_project_tolerance

MIN_EVENTS = 8


def _meta(dyn, n, epl):
    ws = 4 if dyn == "double_integrator" else 6
    return dict(dynamics_type=dyn, num_agents=n, num_landmarks=2, world_size=ws, episode_length=epl,
                num_env_steps=epl * 4, n_rollout_threads=1, use_safety_filter=True, use_masking=True,
                num_internal_step=1, seed=SEED, env_seed=SEED)


# (dynamics, N, auto-resets, env index, step after which the env is driven all-done or None)
INDEPENDENCE = [("double_integrator", 8, 3, 0, None), ("airtaxi", 16, 2, 1, None),
                ("double_integrator", 64, 1, 2, None), ("double_integrator", 8, 3, 3, 3)]


@pytest.mark.parametrize("dyn,N,n_auto,k,early", INDEPENDENCE)
def test_post_reset_outputs_do_not_depend_on_actions(dyn, N, n_auto, k, early):
    """Episode length 3, random actions (one env also driven all-done early, off the episode
    boundary): after every auto-reset the stepped oracle's obs, node_obs, adjacency (every ego),
    state and landmarks, and its draw counts, equal the resets-only oracle's at the same reset index."""
    from oracle.lsm_oracle import DrawSource, OracleVecEnv
    from oracle_pool import resets_of_env
    meta = _meta(dyn, N, 3)
    vt, tt = tables_for(meta)
    vt, tt = table_dict(vt), table_dict(tt)
    seed_k = SEED + 1000 * k
    ora = OracleVecEnv(meta, 1, seed=SEED, value_table=vt, ttr_table=tt, integrator="restated", seed_offset=k,
                       rng=DrawSource)
    e = ora.envs[0]
    got = [ora.reset(EP)]
    states, lms = [e.s.copy()], [np.column_stack([e.lm_pos, e.lm_heading, e.lm_speed])]
    rng = np.random.default_rng(N)
    t = 0
    reset_steps = []
    while len(got) < 1 + n_auto + (early is not None):
        a = rng.integers(0, 25, (1, N))
        if early is not None and t == early + 1:
            a[:] = 12
        o = ora.step(a, EP)
        if len(o[6][0]) > N:   # the episode summary was appended: the env reset
            got.append(o)
            states.append(e.s.copy())
            lms.append(np.column_stack([e.lm_pos, e.lm_heading, e.lm_speed]))
            reset_steps.append(t)
        if early is not None and t == early:
            st, reached = arrive_all_state(lms[-1], N, 2)
            e.s[:] = st
            e.reached_goal[:] = reached
            e.calculate_distances()
        t += 1
        assert t < 40
    if early is not None:
        assert early + 1 in reset_steps, "the env driven all-done did not reset early: %s" % reset_steps
    want = resets_of_env(meta, seed_k, EP, len(got), "mt19937", vt, tt)
    for r, o in enumerate(got):
        ctx = "reset index %d" % r
        np.testing.assert_array_equal(np.asarray(o[0][0], dtype=np.float32), want["obs"][r], err_msg=ctx)
        np.testing.assert_array_equal(np.asarray(o[2][0], dtype=np.float32), want["node"][r], err_msg=ctx)
        adj = np.asarray(o[3][0], dtype=np.float32)
        for i in range(N):
            np.testing.assert_array_equal(adj[i], want["adj"][r], err_msg=ctx)
        np.testing.assert_array_equal(states[r], want["state"][r], err_msg=ctx)
        np.testing.assert_array_equal(lms[r], want["lm"][r], err_msg=ctx)
    log = e._src.log
    assert len(log) == len(got), "the oracle began a reset outside reset()"
    np.testing.assert_array_equal([x["words"] for x in log], want["words"])
    np.testing.assert_array_equal([x["start"] for x in log], want["start"])   # no draw between resets
    np.testing.assert_array_equal([x["redraws"] for x in log], want["redraws"])


def test_draw_source_is_numpys_stream():
    """DrawSource(seed) answers RandomState(seed).uniform bit for bit (scalars and arrays), and the
    oracle's reset through it equals the default source's."""
    from oracle.lsm_oracle import DrawSource, OracleEnv
    a, b = DrawSource(7), np.random.RandomState(7)
    for lo, hi, size in ((0, 1, None), (-3.2, 3.2, 2), (0.1, 0.5, 2), (0.0, 2 * np.pi, None)):
        np.testing.assert_array_equal(a.uniform(lo, hi, size), b.uniform(lo, hi, size))
    assert a.words == 12
    meta = _meta("airtaxi", 6, 5)
    vt, tt = tables_for(meta)
    envs = [OracleEnv(meta, 99, table_dict(vt), table_dict(tt), integrator="restated", rng=r)
            for r in (None, DrawSource(99))]
    for _ in range(3):
        o = [e.reset(EP) for e in envs]
        for i in (0, 2, 3):
            np.testing.assert_array_equal(np.array(o[0][i]), np.array(o[1][i]))
        np.testing.assert_array_equal(envs[0].s, envs[1].s)
    rec = envs[1]._src.log
    assert [x["start"] for x in rec] == list(np.cumsum([0] + [x["words"] for x in rec[:-1]]))


class _GlibcAtan2:
    """numpy with arctan2 answered by the C library's atan2 (math.atan2), which the host text calls:
    numpy's own arctan2 differs from it in the last ulp for some arguments (tests/test_capi.py
    test_host_scenario_matches_oracle), and the landmark headings go through it."""

    def __getattr__(self, name):
        return getattr(np, name)

    @staticmethod
    def arctan2(y, x):
        return math.atan2(y, x)


@pytest.mark.parametrize("libm", ["glibc_atan2", "numpy_arctan2"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_philox_fed_oracle_matches_host_scenario(name, libm, monkeypatch):
    """Reset index 0 of every env of the config's env set: the oracle's scenario drawn from
    lsm_host_philox_uniforms(seed + 1000 k, 0, ...) against lsm_host_scenario(cfg with LSM_RNG_PHILOX,
    cur, seed + 1000 k), agent states and landmarks. (Both dynamics: "at16" is airtaxi.)
    "glibc_atan2": with the C library's atan2 in the oracle's scenario code, everything is equal
    exactly. "numpy_arctan2" (the oracle as it is, the truth of the GPU tests): everything drawn is equal
    exactly -- agent states, landmark positions and speeds -- and the headings, atan2 of exactly
    equal arguments plus an exactly equal draw, within the two libraries' last ulp (4e-16, the bound
    of tests/test_capi.py). So the device's draw sequence under Philox is the oracle's call
    sequence, and the Philox truth is the oracle itself at every reset index."""
    from lsm import capi, curriculum
    from lsm.config import EnvArgs
    import oracle.lsm_oracle as lsm_oracle
    from oracle_pool import philox_source
    if libm == "glibc_atan2":
        monkeypatch.setattr(lsm_oracle, "np", _GlibcAtan2())
    cfg_ = CONFIGS[name]
    meta = cfg_["meta"]
    N, L = meta["num_agents"], meta["num_landmarks"]
    di = meta["dynamics_type"] == "double_integrator"
    lib = capi.load_library()
    cfg = capi.LsmConfig(dynamics=0 if di else 1, num_envs=1, num_agents=N, num_landmarks=L,
                         episode_length=meta["episode_length"], world_size=meta["world_size"],
                         rng=capi.LSM_RNG_PHILOX)
    args = EnvArgs.from_namespace(type("A", (), meta)())
    cur = curriculum.to_struct(curriculum.curriculum_block(args, EP))
    vt, tt = tables_for(meta)
    vt, tt = table_dict(vt), table_dict(tt)
    for k in range(cfg_["n_envs"]):
        seed_k = SEED + 1000 * k
        src = philox_source(seed_k)
        e = lsm_oracle.OracleEnv(meta, seed_k, vt, tt, integrator="restated", rng=src)
        e.update_curriculum(EP)
        src.begin_reset()
        e.random_scenario()
        st, lm = np.zeros((N, 4)), np.zeros((L * N, 4))
        assert lib.lsm_host_scenario(C.byref(cfg), C.byref(cur), seed_k, st.ctypes.data, lm.ctypes.data) == 0
        ctx = "env %d" % k
        np.testing.assert_array_equal(e.s, st, err_msg=ctx)
        np.testing.assert_array_equal(e.lm_pos, lm[:, :2], err_msg=ctx)
        np.testing.assert_array_equal(e.lm_speed, lm[:, 3], err_msg=ctx)
        if libm == "glibc_atan2":
            np.testing.assert_array_equal(e.lm_heading, lm[:, 2], err_msg=ctx)
        else:
            np.testing.assert_allclose(e.lm_heading, lm[:, 2], rtol=4e-16, atol=4e-16, err_msg=ctx)


def test_philox_source_reset_index_selects_the_stream():
    """philox_source's r-th reset reads lsm_host_philox_uniforms(seed, r, ...): the scenarios of reset
    indices 0 .. 3 are those of four sources read at index 0 of keys whose streams are fetched
    directly, and all differ."""
    from lsm import capi
    from oracle_pool import philox_source
    lib = capi.load_library()
    src = philox_source(4021)
    seen = []
    for r in range(4):
        src.begin_reset()
        got = np.array([src.uniform(-2.0, 3.0) for _ in range(9)] + list(src.uniform(-2.0, 3.0, 2)))
        want = np.zeros(11)
        lib.lsm_host_philox_uniforms(4021, r, 11, -2.0, 3.0, want.ctypes.data)
        np.testing.assert_array_equal(got, want)
        assert src.log[r] == dict(start=22 * r, words=22, redraws=0, longest=0)
        seen.append(got)
    assert len({tuple(x) for x in seen}) == 4


_COUNTS = {}


def _counts(name):
    from oracle_pool import run_all_resets
    if name not in _COUNTS:
        cfg = CONFIGS[name]
        _COUNTS[name] = run_all_resets(cfg["meta"], SEED, cfg["n_envs"], EP, sure_resets(cfg), outputs=False)
    return _COUNTS[name]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_coverage_condition(name):
    """From the oracle alone, over the resets every env of the config is compared at (the first and
    the episode ends; envs driven all-done early add more): at least 8 resets with a rejection
    redraw, at least 8 whose draws cross a 624-word MT19937 block boundary, for a family with a
    small stage at least 8 that need more than the staged words, and for the team kernels at least 8
    with a rejection loop past the eight attempts one ballot resolves."""
    cfg = CONFIGS[name]
    c = _counts(name)
    assert c["words"].shape == (cfg["n_envs"], sure_resets(cfg))
    redraw = int((c["redraws"] > 0).sum())
    cross = int(c["crosses"].sum())
    print("coverage %s: envs=%d resets=%d resets_with_redraw=%d (max redraws %d) resets_crossing_block=%d "
          "words per reset min/max=%d/%d" % (name, cfg["n_envs"], c["words"].size, redraw, int(c["redraws"].max()),
                                             cross, int(c["words"].min()), int(c["words"].max())))
    assert redraw >= MIN_EVENTS
    assert cross >= MIN_EVENTS
    if any(f["kernel"].startswith("rollout_team_kernel<") for f in cfg["families"].values()):
        # the team kernel's wave draw resolves attempts 0 .. 7 of two agents in one ballot: an agent
        # accepted at attempt 7 leaves its neighbour to the next ballot, a longer loop goes on 64 at a time
        seven = int((c["longest"] >= 7).sum())
        longer = int((c["longest"] >= 8).sum())
        print("coverage %s: resets_with_a_loop_reaching_attempt_7=%d beyond_7=%d (longest %d)" % (
            name, seven, longer, int(c["longest"].max())))
        assert longer >= MIN_EVENTS
    for fam, f in cfg["families"].items():
        if f["stage"] is None:
            continue
        # the staged stream serves min(2 * 624 - p0, stage) words of a reset starting at word p0
        p0 = np.where(c["start"] % 624 == 0, 624, c["start"] % 624)
        over = int((c["words"] > np.minimum(2 * 624 - p0, f["stage"])).sum())
        print("coverage %s/%s: resets_needing_more_than_stage=%d" % (name, fam, over))
        assert over >= MIN_EVENTS


@pytest.mark.parametrize("name", list(CONFIGS))
def test_draw_counts_of_the_scenario_alone_equal_those_of_reset(name):
    """The coverage condition counts draws with outputs=False (the scenario draw alone); the GPU truth
    comes from reset() itself. Same counts, first three envs, two resets."""
    from oracle_pool import resets_of_env
    meta = CONFIGS[name]["meta"]
    vt, tt = tables_for(meta)
    vt, tt = table_dict(vt), table_dict(tt)
    for k in range(3):
        a = resets_of_env(meta, SEED + 1000 * k, EP, 2, "mt19937", vt, tt, outputs=True)
        b = resets_of_env(meta, SEED + 1000 * k, EP, 2, "mt19937", vt, tt, outputs=False)
        for key in ("words", "start", "redraws", "longest", "crosses"):
            np.testing.assert_array_equal(a[key], b[key], err_msg="env %d %s" % (k, key))


def _plain_run(name, rng, k):
    """Env k of the config stepped plainly through all its steps (the GPU test's actions and
    injections): [(outputs, reset index, step of the latest reset before this step)] per step."""
    from oracle.lsm_oracle import OracleVecEnv
    from oracle_pool import _source
    cfg = case(name, rng)
    meta = cfg["meta"]
    N, L = meta["num_agents"], meta["num_landmarks"]
    vt, tt = tables_for(meta)
    ora = OracleVecEnv(meta, 1, seed=SEED, value_table=table_dict(vt), ttr_table=table_dict(tt),
                       integrator="restated", seed_offset=k, rng=lambda s: _source(rng, s))
    e = ora.envs[0]
    ora.reset(EP)
    acts = actions(name, rng)
    out, r, t0 = [], 0, -1
    for t in range(cfg["steps"]):
        o = ora.step(acts[t][k][None], EP)
        out.append((step_outputs(o, e, N), r, t0))
        if out[-1][0]["reset"]:
            r, t0 = r + 1, t
        if k in cfg["early"].get(t, ()):
            st, reached = arrive_all_state(np.column_stack([e.lm_pos, e.lm_heading, e.lm_speed]), N, L)
            e.s[:] = st
            e.reached_goal[:] = reached
            e.calculate_distances()
    return out


@pytest.mark.parametrize("name", [n for n, c in CONFIGS.items() if c["early"]])
def test_injected_envs_reset_on_schedule(name):
    """Every env a GPU case drives all-done early, and one it does not, stepped through the oracle:
    it resets at exactly the steps of reset_schedule (the injection makes the next step all-done;
    nothing else ends an episode early), which the GPU test then asserts of the device's flags."""
    sched = reset_schedule(CONFIGS[name])
    for k, want in sched.items():
        run = _plain_run(name, "mt19937", 1 if k is None else k)
        got = [t for t, (o, _, _) in enumerate(run) if o["reset"]]
        assert got == want, "env %s resets at %s, schedule %s" % (k, got, want)
    off = sorted({t for k, v in sched.items() if k is not None for t in v} - set(sched[None]))
    assert len(off) >= 3, off   # several phases off the common boundary


@pytest.mark.parametrize("name,rng,k", [("di8", "mt19937", 5), ("di8", "philox", 1020), ("di3", "mt19937", 5)])
def test_replay_arbiter_reproduces_a_plain_run(name, rng, k):
    """reset_cases.replay (resets alone up to the reset index, then the episode's actions and
    injections) gives, at every step, exactly what the plainly stepped oracle shows; and
    within_project_tolerance accepts those outputs and refuses a shifted observation, a state off
    by 1e-8 and a wrong reset flag."""
    acts = actions(name, rng)
    run = _plain_run(name, rng, k)
    assert {r for _, r, _ in run} >= {0, 1, 2, 3}
    for t, (plain, r, t0) in enumerate(run[:24]):
        want = replay(name, rng, k, r, t0, t, acts)
        for key in plain:
            np.testing.assert_array_equal(plain[key], want[key], err_msg="step %d %s" % (t, key))
        assert within_project_tolerance(plain, want)[0]
    for key, delta in (("obs", 5e-5), ("state", 1e-8)):
        bad = dict(plain)
        bad[key] = plain[key] + delta
        ok, why = within_project_tolerance(bad, want)
        assert not ok and why
    assert not within_project_tolerance(dict(plain, reset=not plain["reset"]), want)[0]
