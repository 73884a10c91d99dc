"""Injected layouts for the safety filter's choice of a deconflicting agent, and the oracle run that
tests/test_gpu_filter_choice.py replays through every one-wave, team and small-N workgroup kernel.

The smooth synthetic table almost never separates the value argmin from the nearest agent, never ties,
and never leaves an ego with one partner or none. The layouts here do, on the hard tables of
tests/hj_bounds_model.py ("rough": noise per node; "spike": lowered nodes, the "last" one by GATE_DEPTH
so that the coordination-range gate alone decides an outcome). Every layout comes with a proof of power
computed from the oracle alone (pair_table / OracleEnv._filter_one): what a kernel with the wrong tie
rule, the distance argmin in the value path or no range gate would answer differs from the oracle.

    spike pairs   partner 1 is ego 0's exact argmin and not its nearest agent (M.spike_injections)
    twins         two agents in one bit-identical state, both ego 0's argmin: the lower index wins
    loner         ego 0 has no in-grid pair: the first active other, filter not applied;
                  second form with agent 1 retired first (the first active other is 2)
    third         every third agent on its final goal: done agents, egos and candidates in one wave
    sole          every agent but SOLE_KEEP arrives: an active ego with no active other, no reset
    offgrid       ego 0 within range of the others and every pair outside the table (by velocity)
    gate          ego 0's argmin has a value below the optimal-control threshold, and its nearest agent
                  is 0.1 beyond the coordination range: unfiltered, and filtered without the gate
"""
from __future__ import annotations

import numpy as np

import hj_bounds_model as M
from golden_replay import table_dict

DI, AT = "double_integrator", "airtaxi"
SHAPES = {DI: M.DI_SMALL, AT: M.AT_SMALL}
BSHIFT = 1
GATE_DEPTH = 6.0
KINDS = ("rough", "spike")
# (dynamics, agents) of the parity cases: the team kernels' N, the NT = 0 rows, compile-time N = 3
SPECS = ((DI, 8), (AT, 16), (DI, 5), (AT, 6), (DI, 3), (AT, 3))
ALL_TERMS = ("safety_violation", "potential_conflict", "diff_from_filtered_action", "hj_value")

STATUSES = ("inactive", "alone", "beyond_range", "out_of_grid", "optimal", "qp")
FILTER_THRESHOLD = 1e-4    # _filter_one: filtered = |u - u_ref| > 1e-4
OPTIMAL_BELOW = 0.4        # _filter_one: the optimal (bang-bang) control below this value, else the QP

# run shape: 15 envs (a partly filled last workgroup at 2, 4 and 8 envs per workgroup), two auto-resets
N_ENVS, EPISODE_LENGTH, STEPS, EP, SEED = 15, 6, 14, 4, 11
INJECT_AT = (0, EPISODE_LENGTH)      # the steps that run on injected states
# envs 4..7 share a workgroup at 4 and at 8 envs per workgroup; 9, 10 and 14 sit in another
ENV_TWINS, ENV_SOLE, ENV_LONER, ENV_GATE, ENV_OFFGRID, ENV_THIRD, ENV_LONER2 = 4, 5, 6, 7, 8, 9, 10
ENV_SPIKES = (0, 1, 2, 3, 11, 14)    # the spike pairs in order, again from the first where they run out
SOLE_KEEP = 2
ARRIVE_ACTION = 12                   # zero acceleration / zero turn rate

_TABLES, _TTR, _RUNS = {}, {}, {}


def table(dyn, kind):
    """The small hard table of ``kind``; "spike" has its "last" node lowered by GATE_DEPTH."""
    if (dyn, kind) not in _TABLES:
        depth = {"last": GATE_DEPTH} if kind == "spike" else None
        _TABLES[dyn, kind] = M.make_table(dyn, kind, SHAPES[dyn], bshift=BSHIFT, depth=depth)
    return _TABLES[dyn, kind]


def ttr(dyn):
    from lsm import hj_tables
    if dyn == DI:
        return None
    if dyn not in _TTR:
        _TTR[dyn] = hj_tables.ttr_table_from_stored(hj_tables.synthetic_ttr((25, 25, 24, 7)))
    return _TTR[dyn]


def spec_meta(dyn, N, rext=False):
    meta = dict(dynamics_type=dyn, num_agents=N, num_landmarks=2, world_size=4 if dyn == DI else 6,
                episode_length=EPISODE_LENGTH, num_env_steps=EPISODE_LENGTH * 4, n_rollout_threads=1,
                use_safety_filter=True, use_masking=True, num_internal_step=1, seed=SEED, env_seed=SEED)
    if rext:
        meta.update(collaborative=True, reward_terms=ALL_TERMS)
    return meta


def oracle_vec(meta, vt, n_envs=N_ENVS):
    from oracle.lsm_oracle import OracleVecEnv
    return OracleVecEnv(meta, n_envs, seed=meta["seed"], value_table=table_dict(vt),
                        ttr_table=table_dict(ttr(meta["dynamics_type"])), integrator="restated")


def kernel_variants():
    """(dyn, N, reward case, label, kernel_select, the lsm_kernels.h row that must run)."""
    out = []
    for d, dyn, N, teams in ((0, DI, 8, (2, 4, 8)), (1, AT, 16, (2, 4))):
        for g in teams:
            out.append((dyn, N, False, "team%d" % g, dict(team=g), "rollout_team_kernel<%d, %d, %d, false>" % (d, N, g)))
            # the optional-reward block: collaborative, all four terms (the reward's own interp_value)
            out.append((dyn, N, True, "team%d" % g, dict(team=g), "rollout_team_kernel<%d, %d, %d, true>" % (d, N, g)))
        out.append((dyn, N, False, "wave64", dict(team=0, lanes_per_env=64), "rollout_kernel<%d, 64, %d>" % (d, N)))
        out.append((dyn, N, False, "wave32", dict(team=0, lanes_per_env=32), "rollout_kernel<%d, 32, %d>" % (d, N)))
        out.append((dyn, N, False, "generic64", dict(generic=1, lanes_per_env=64), "rollout_kernel<%d, 64, 0>" % d))
        if dyn == DI:   # 4 airtaxi envs of 16 agents per wave need 98 KB of LDS (> 64 KB per workgroup)
            out.append((dyn, N, False, "wave16", dict(lanes_per_env=16), "rollout_kernel<%d, 16, 0>" % d))
            out.append((dyn, N, True, "wave64", dict(team=0, lanes_per_env=64), "rollout_kernel<%d, 64, %d>" % (d, N)))
        out.append((dyn, N, False, "block", dict(workgroup_per_env=1), "rollout_block_kernel<%d, 0, true, false>" % d))
    for d, dyn, N in ((0, DI, 5), (1, AT, 6)):   # no compile-time row: the NT = 0 loop
        for lpe in (64, 32, 16):
            out.append((dyn, N, False, "wave%d" % lpe, dict(lanes_per_env=lpe), "rollout_kernel<%d, %d, 0>" % (d, lpe)))
        out.append((dyn, N, False, "block", dict(workgroup_per_env=1), "rollout_block_kernel<%d, 0, true, false>" % d))
    for d, dyn in ((0, DI), (1, AT)):
        out.append((dyn, 3, False, "default", None, "rollout_kernel<%d, 64, 3>" % d))
    return out


# ---- what the filter decides for one ego ----------------------------------------------------------------
def filter_status(env, i):
    """The branch that World.step takes for ego i of oracle env ``env`` at its current state
    (_inner_step / _filter_one up to the choice of a control): status (one of STATUSES), dec (the
    deconflicting agent, -1 without one), nearest, dist (to the nearest), value (the argmin's),
    ties (the active others whose value is bit-equal to the minimum, in index order)."""
    if env.done[i] or not env.departed[i]:
        return dict(status="inactive", dec=-1, nearest=-1, ties=[])
    others = [j for j in range(env.N) if j != i and not env.done[j] and env.departed[j]]
    if not others:
        return dict(status="alone", dec=-1, nearest=-1, ties=[])
    e = env.s[i]
    dists = [np.sqrt((env.s[j][0] - e[0]) ** 2 + (env.s[j][1] - e[1]) ** 2) for j in others]
    vals, inr = zip(*(env._value(env._rel_state(e, env.s[j])) for j in others))
    jd, jv = int(np.argmin(dists)), int(np.argmin(vals))
    if dists[jd] > env.coordination_range:
        status = "beyond_range"
    elif not inr[jv]:
        status = "out_of_grid"
    else:
        status = "optimal" if vals[jv] < OPTIMAL_BELOW else "qp"
    return dict(status=status, dec=others[jv], nearest=others[jd], dist=float(dists[jd]), value=float(vals[jv]),
                in_grid=int(sum(inr)), ties=[j for j, v in zip(others, vals) if v == vals[jv]])


def _with_states(env, states, reached=None):
    """A context that puts ``states`` into oracle env ``env`` and restores what it held."""
    class _Ctx:
        def __enter__(self):
            self.keep = (env.s.copy(), np.array(env.reached_goal, copy=True))
            M.inject(env, states, reached)
            return env

        def __exit__(self, *exc):
            M.inject(env, *self.keep)
    return _Ctx()


# ---- layouts (each a function of an oracle env just reset, and of its table) ---------------------------
def spike_pairs(dyn, vt, N):
    """M.spike_injections as it is, with the proof asserted: partner 1 is ego 0's exact argmin, and
    another agent is nearer (so the distance argmin in the value path answers otherwise)."""
    inj = M.spike_injections(dyn, vt, BSHIFT, N)
    for r in inj:
        assert r["argmin"] == 1, (dyn, N, r["name"], r["side"], r["argmin"])
        s = r["states"]
        d = np.hypot(s[1:, 0] - s[0, 0], s[1:, 1] - s[0, 1])
        assert N == 2 or int(np.argmin(d)) != 0, (dyn, N, r["name"], r["side"], d)
    return inj


def twin_indices(N):
    return (3, 5) if N >= 6 else (N - 2, N - 1)


def twins_proof(env, states):
    """Both twins are ego 0's value argmin with bit-equal finite values: np.argmin (first occurrence)
    answers the lower index, a rule where the higher index wins on a tie the upper one."""
    a, b = twin_indices(env.N)
    with _with_states(env, states):
        st = filter_status(env, 0)
    if st["status"] not in ("optimal", "qp") or st["ties"] != [a, b]:
        return False
    assert st["dec"] == a and max(st["ties"]) == b and np.isfinite(st["value"])
    return True


def twins_layout(env, tries=64):
    """Agents (3, 5) (the last two below N = 6) in one state, at offset default_rng(k).uniform(-0.6,
    0.6, 2) from ego 0's position, the first k = 0, 1, .. at which twins_proof holds. (states, k)."""
    a, b = twin_indices(env.N)
    for k in range(tries):
        s = env.s.copy()
        s[a, :2] = s[0, :2] + np.random.default_rng(k).uniform(-0.6, 0.6, 2)
        s[b] = s[a]
        if twins_proof(env, s):
            return s, k
    raise AssertionError("no twin offset in %d tries makes both twins ego 0's argmin" % tries)


def loner_proof(env, states, reached=None, first=1, want=("beyond_range", "out_of_grid")):
    """Every value of ego 0 is +inf: its deconflicting agent is the first active other and the filter
    is not applied, for all 25 actions."""
    with _with_states(env, states, reached):
        st = filter_status(env, 0)
        assert st["status"] in want and st["in_grid"] == 0 and st["dec"] == first, st
        for a in range(25):
            u, filtered, dec = env._filter_one(0, env.decode(np.full(env.N, a)))
            assert not filtered and dec == first, (a, filtered, dec)
    return st


def offgrid_layout(env):
    """Ego 0 beside agent 1, well within the coordination range, with a velocity that puts every one of
    its pairs outside the table: the double integrator's relative velocity beyond the grid's +-1 (0.6
    against -0.45), the airtaxi's own speed above the grid's top. The filter reaches its in-grid test
    (the loner stops at the range gate) and leaves the control alone."""
    s = env.s.copy()
    if env.di:
        s[0] = [s[1, 0] + 0.8, s[1, 1] + 0.3, 0.6, 0.0]
        s[1:, 2], s[1:, 3] = -0.45, 0.02 * np.arange(1, env.N)
    else:
        s[0, :2] = s[1, 0] + 1.0, s[1, 1] + 0.4
        s[0, 3] = 1.02 * float(env.hj_grid.hi[3])
    return s


def loner_retired_layout(dyn, vt, env, retire=1):
    """loner_layout with agent ``retire`` on its final goal: done after one step, so that from the second
    step on ego 0's first active other is the next agent. (states, reached)."""
    s = M.loner_layout(dyn, vt, env.N)
    arrived, r_all = M.arrive_subset(env, every=1)
    reached = np.asarray(env.reached_goal, dtype=np.int32).copy()
    s[retire], reached[retire] = arrived[retire], r_all[retire]
    return s, reached


def sole_survivor_layout(env, keep=SOLE_KEEP):
    """Every agent but ``keep`` on its final goal. (states, reached)."""
    s, reached = M.arrive_subset(env, every=1)
    s[keep], reached[keep] = env.s[keep], env.reached_goal[keep]
    return s, reached


def gate_layout(dyn, vt, env):
    """The "last" spike pair (lowered by GATE_DEPTH) with the crowd, ego 0's nearest agents, 0.1 beyond the
    coordination range."""
    spike = M.spike_nodes(dyn, vt.shape, BSHIFT)["last"]
    return M.spike_layout(dyn, vt, spike, "below", env.N, env.coordination_range + 0.1)


def gate_proof(env, states):
    """Every pair of ego 0 is in the grid, its argmin (partner 1) has a value below the optimal-control
    threshold, its nearest agent is beyond the coordination range: for all 25 actions _filter_one
    answers (not filtered, 1), and with an infinite coordination range it answers filtered."""
    with _with_states(env, states):
        st = filter_status(env, 0)
        assert st["status"] == "beyond_range" and st["dec"] == 1 and st["in_grid"] == env.N - 1, st
        assert st["value"] < OPTIMAL_BELOW and st["dist"] > env.coordination_range, st
        keep = env.coordination_range
        try:
            for rng_, want in ((keep, False), (np.inf, True)):
                env.coordination_range = rng_
                for a in range(25):
                    u, filtered, dec = env._filter_one(0, env.decode(np.full(env.N, a)))
                    assert (filtered, dec) == (want, 1), (rng_, a, filtered, dec)
        finally:
            env.coordination_range = keep
    return st


# ---- the oracle's run ---------------------------------------------------------------------------------
def injections(dyn, kind, envs):
    """The states to inject into the oracle envs ``envs`` (just reset), every layout's proof asserted:
    {env index: dict(name, states, reached)}, and the proofs' figures."""
    vt, N = table(dyn, kind), envs[0].N
    out, facts = {}, {}
    if kind == "spike":
        inj = spike_pairs(dyn, vt, N)
        for n, k in enumerate(ENV_SPIKES):
            r = inj[n % len(inj)]
            out[k] = dict(name="spike %s %s" % (r["name"], r["side"]), states=r["states"], reached=None)
        g = gate_layout(dyn, vt, envs[ENV_GATE])
        facts["gate"] = gate_proof(envs[ENV_GATE], g)
        out[ENV_GATE] = dict(name="gate", states=g, reached=None)
    s, k = twins_layout(envs[ENV_TWINS])
    facts["twins_k"] = k
    out[ENV_TWINS] = dict(name="twins", states=s, reached=None)
    s, r = sole_survivor_layout(envs[ENV_SOLE])
    out[ENV_SOLE] = dict(name="sole", states=s, reached=r)
    s = M.loner_layout(dyn, vt, N)
    facts["loner"] = loner_proof(envs[ENV_LONER], s)
    out[ENV_LONER] = dict(name="loner", states=s, reached=None)
    s = offgrid_layout(envs[ENV_OFFGRID])
    facts["offgrid"] = loner_proof(envs[ENV_OFFGRID], s, want=("out_of_grid",))
    out[ENV_OFFGRID] = dict(name="offgrid", states=s, reached=None)
    s, r = M.arrive_subset(envs[ENV_THIRD], every=3)
    out[ENV_THIRD] = dict(name="third", states=s, reached=r)
    s, r = loner_retired_layout(dyn, vt, envs[ENV_LONER2])
    out[ENV_LONER2] = dict(name="loner2", states=s, reached=r)
    return out, facts


def arrive_actions(a, N):
    """The agents that are to arrive hold their state (in place)."""
    a[ENV_SOLE, [i for i in range(N) if i != SOLE_KEEP]] = ARRIVE_ACTION
    a[ENV_THIRD, ::3] = ARRIVE_ACTION
    a[ENV_LONER2, 1] = ARRIVE_ACTION
    return a


def oracle_run(dyn, N, kind, rext=False):
    """The oracle's trajectory of (spec, table kind, reward case) over N_ENVS envs and STEPS steps,
    computed once per session and shared by every kernel variant: random actions, the layouts injected
    after the initial reset and again after the first auto-reset, action ARRIVE_ACTION for the agents
    that are to arrive. Per step: the injections made before it, the actions, every output (graph
    outputs as float32, the kernel's type), the states, each ego's filter_status before the step and
    the oracle's deconflicting / safety_filtered / action_diff after it."""
    key = (dyn, N, kind, bool(rext))
    if key in _RUNS:
        return _RUNS[key]
    meta, vt = spec_meta(dyn, N, rext), table(dyn, kind)
    ora = oracle_vec(meta, vt)
    f32 = lambda x: np.asarray(x, dtype=np.float32)   # noqa: E731
    o = ora.reset(EP)
    run = dict(meta=meta, reset=dict(obs=f32(o[0]), node=f32(o[2]), adj=f32(o[3]),
                                     state=np.stack([e.s.copy() for e in ora.envs])), steps=[], facts=[])
    rng = np.random.default_rng(5)
    for t in range(STEPS):
        inj = {}
        if t in INJECT_AT:
            inj, facts = injections(dyn, kind, ora.envs)
            run["facts"].append(facts)
            for k, r in inj.items():
                M.inject(ora.envs[k], r["states"], r["reached"])
        status = [[filter_status(e, i) for i in range(N)] for e in ora.envs]
        a = arrive_actions(rng.integers(0, 25, (N_ENVS, N)), N)
        o = ora.step(a, EP)
        reset = np.array([len(x) > N for x in o[6]])
        info = lambda name, dt: np.array([[d[name] for d in inf[:N]] for inf in o[6]], dtype=dt)   # noqa: E731
        run["steps"].append(dict(
            inject=inj, a=a, status=status, reset=reset, obs=f32(o[0]), node=f32(o[2]), adj=f32(o[3]),
            rew=np.asarray(o[4]), dones=np.asarray(o[5]), state=np.stack([e.s.copy() for e in ora.envs]),
            ind_rew=info("individual_reward", np.float64), min_rel=info("min_relative_distance", np.float64),
            filtered_info=info("Safety filtered", bool),
            # the oracle env's own per-step arrays (re-initialised where the env reset: skip those)
            dec=np.stack([e.deconflicting.copy() for e in ora.envs]),
            filtered=np.stack([e.safety_filtered.copy() for e in ora.envs]),
            action_diff=np.stack([e.action_diff.copy() for e in ora.envs])))
    _RUNS[key] = run
    return run


def check_run(run, kind):
    """The conditions on the inputs, from the oracle's run alone. Returns the figures."""
    meta = run["meta"]
    dyn, N = meta["dynamics_type"], meta["num_agents"]
    steps = run["steps"]
    resets = [t for t, r in enumerate(steps) if r["reset"].any()]
    assert resets == [EPISODE_LENGTH - 1, 2 * EPISODE_LENGTH - 1], resets
    assert all(steps[t]["reset"].all() for t in resets)       # every env, the sole survivor's included
    count = dict.fromkeys(STATUSES, 0)
    active = off_nearest = ties = 0
    for t, r in enumerate(steps):
        for k in range(N_ENVS):
            for i in range(N):
                st = r["status"][k][i]
                count[st["status"]] += 1
                if st["status"] in ("optimal", "qp"):   # the egos whose argmin feeds the filter's control
                    active += 1
                    off_nearest += st["dec"] != st["nearest"]
                    ties += len(st["ties"]) > 1
                if not r["reset"][k]:
                    # the status is the branch the oracle took
                    assert r["dec"][k, i] == st["dec"], (t, k, i, st, r["dec"][k, i])
                    assert not (r["filtered"][k, i] and st["status"] not in ("optimal", "qp")), (t, k, i, st)
                    assert r["filtered_info"][k, i] == r["filtered"][k, i]
        live = ~r["reset"]
        near = np.abs(r["action_diff"][live] - FILTER_THRESHOLD)
        assert near.size == 0 or near.min() > 1e-6, (t, near.min())   # no control on the "filtered" threshold
    for st, c in count.items():
        assert c > 0, (st, count)
    share = off_nearest / active
    if kind == "rough":
        assert share >= 0.01, share
    # filtered and unfiltered active egos in every episode (both sides of every auto-reset)
    for lo, hi in ((0, resets[0]), (resets[0] + 1, resets[1]), (resets[1] + 1, STEPS)):
        f = np.concatenate([steps[t]["filtered_info"].ravel() for t in range(lo, hi)])
        act = np.concatenate([[st["status"] not in ("inactive", "alone") for row in steps[t]["status"] for st in row]
                              for t in range(lo, hi)])
        assert (f & act).any() and (~f & act).any(), (lo, hi)
    # each layout in the step after its injection
    a, b = twin_indices(N)
    for t in INJECT_AT:
        r, nxt = steps[t], steps[t + 1]
        for k, inj in r["inject"].items():
            if inj["name"].startswith("spike"):
                assert r["dec"][k, 0] == 1 and r["status"][k][0]["nearest"] != 1, (t, k, r["status"][k][0])
        if kind == "spike":
            assert r["dec"][ENV_GATE, 0] == 1 and not r["filtered"][ENV_GATE, 0]
            assert r["status"][ENV_GATE][0]["status"] == "beyond_range"
        assert r["status"][ENV_TWINS][0]["ties"] == [a, b] and r["dec"][ENV_TWINS, 0] == a
        assert r["dec"][ENV_LONER, 0] == 1 and not r["filtered"][ENV_LONER, 0]
        assert r["status"][ENV_LONER][0]["in_grid"] == 0
        assert r["dec"][ENV_OFFGRID, 0] == 1 and not r["filtered"][ENV_OFFGRID, 0]
        assert r["status"][ENV_OFFGRID][0]["status"] == "out_of_grid"
        assert r["dones"][ENV_THIRD, ::3].all() and not r["dones"][ENV_THIRD].all()
        assert r["dones"][ENV_LONER2, 1] and nxt["status"][ENV_LONER2][0]["in_grid"] == 0
        assert nxt["dec"][ENV_LONER2, 0] == 2 and not nxt["filtered"][ENV_LONER2, 0]
        sole = [i for i in range(N) if i != SOLE_KEEP]
        assert r["dones"][ENV_SOLE, sole].all() and not r["dones"][ENV_SOLE, SOLE_KEEP] and not r["reset"][ENV_SOLE]
        assert (nxt["dec"][ENV_SOLE] == -1).all() and nxt["status"][ENV_SOLE][SOLE_KEEP]["status"] == "alone"
    return dict(count=count, active=active, off_nearest=off_nearest, share=share, ties=ties,
                twins_k=[f["twins_k"] for f in run["facts"]])
