"""The workgroup kernel's bound-pruned HJ argmin (rollout_block_kernel<D, 64, ...>, csrc/lsm_block.h)
against the full search, the device bounds table against its numpy model (tests/hj_bounds_model.py),
both against the CPU oracle, on tables where a wrong bound decides an argmin: noise per node, and
spikes on the nodes a bounds block shares with its neighbour, clips at the table's edge or reaches by
the periodic wrap. Every test checks from the model, before it trusts an equality, that the pruning
drops between 5 % and 95 % of the in-grid pairs it is given."""
import ctypes as C

import numpy as np
import pytest

import hj_bounds_model as M
from golden_replay import table_dict

pytestmark = pytest.mark.gpu

STATE_ATOL = 1e-9
F32_ATOL = 1e-5
N = 64
DI, AT = "double_integrator", "airtaxi"
# (shape, bounds_shift) pairs with a modelled pruned share within 5-95 % (coarser blocks prune nothing
# on the small tables: the wide shapes are for bounds_shift 3 and 4)
SHIFTS = {DI: ((M.DI_SMALL, 1), (M.DI_SMALL, 2), (M.DI_WIDE, 3), (M.DI_WIDE, 4)),
          AT: ((M.AT_SMALL, 1), (M.AT_SMALL, 2), (M.AT_WIDE, 2), (M.AT_WIDE, 3))}
# the finest block size per airtaxi shape: there a block without its wrap node is high enough for the
# model to prune the wrap spike's pair (coarser heading blocks hold lower nodes of their own)
WRAP_POWER = {(M.AT_SMALL, 1), (M.AT_WIDE, 2)}

_TABLES, _TTR, _SHARE = {}, {}, {}


def _table(dyn, kind, shape, bshift=None, separation=None):
    key = (dyn, kind, shape, bshift if kind == "spike" else None, separation)
    if key not in _TABLES:
        if len(_TABLES) >= 4:   # the wide airtaxi tables hold 50 MB of gradients each
            _TABLES.pop(next(iter(_TABLES)))
        _TABLES[key] = M.make_table(dyn, kind, shape, separation=separation, bshift=bshift)
    return _TABLES[key]


def _ttr(dyn):
    from lsm import hj_tables
    if dyn == DI:
        return None
    if dyn not in _TTR:
        _TTR[dyn] = hj_tables.ttr_table_from_stored(hj_tables.synthetic_ttr((25, 25, 24, 7)))
    return _TTR[dyn]


def _meta(dyn, episode_length, seed, **kw):
    return dict(dynamics_type=dyn, num_agents=N, num_landmarks=2, world_size=4 if dyn == DI else 6,
                episode_length=episode_length, num_env_steps=episode_length * 4, n_rollout_threads=1,
                use_safety_filter=True, use_masking=True, num_internal_step=1, seed=seed, env_seed=seed, **kw)


def _gpu_env(meta, vt, n_envs, ksel, **kw):
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    args = EnvArgs.from_namespace(type("A", (), meta)())
    args.seed = meta["seed"]
    env = GpuGraphVecEnv(args, num_envs=n_envs, device="cuda:0", value_table=vt, ttr_table=_ttr(meta["dynamics_type"]),
                         kernel_select=ksel, build_infos=False, **kw)
    want = "rollout_block_kernel<%d, 64, true, false>" % (0 if meta["dynamics_type"] == DI else 1)
    assert env.kernel_name == want, (env.kernel_name, want)   # the compile-time N = 64 workgroup kernel
    return env


def _oracle(meta, vt, n_envs=1, env_offset=0):
    from oracle.lsm_oracle import OracleVecEnv
    return OracleVecEnv(meta, n_envs, seed=meta["seed"], value_table=table_dict(vt),
                        ttr_table=table_dict(_ttr(meta["dynamics_type"])), integrator="restated",
                        seed_offset=env_offset)


def _info_col(name):
    from lsm import capi
    return capi.INFO_FIELDS.index(name)


def _assert_share(tag, st):
    print("%s: modelled pruned share %.3f (%d of %d in-grid pairs, %d out of grid)" % (
        tag, st["share"], st["n_pruned"], st["n_in"], st["n_out"]))
    assert 0.05 <= st["share"] <= 0.95, (tag, st["share"])


def _reset_share(dyn, kind, shape, bshift, vt, meta):
    """Pruned share of oracle env 0 at its reset state (the first GPU env's), cached per table: the pairs
    and their exact values do not depend on the block size."""
    key = (dyn, kind, shape, bshift if kind == "spike" else None, meta["seed"])
    if key not in _SHARE:
        ora = _oracle(meta, vt)
        ora.reset(4)
        _SHARE[key] = (ora.envs[0], M.pair_table(ora.envs[0]))
    env, pairs = _SHARE[key]
    return M.prune_stats(env, vt, bshift, pairs=pairs)


def _spike_injections(dyn, vt, shape, bshift):
    """The spike pairs' layouts, with the model's proof of power asserted: the partner is the exact argmin,
    the right bounds keep it, and bounds without the shared boundary node (without the wrap node)
    prune it, so the ego's argmin flips."""
    inj = M.spike_injections(dyn, vt, bshift, N)
    for r in inj:
        assert r["argmin"] == 1 and r["pruned_argmin"] == 1, r   # the spike pair is the true argmin
        if r["side"] == "below":
            assert r["flips"]["no_shared"] != 1, r               # a wrong-bounds model flips it
        if r["name"] == "wrap" and r["side"] == "below" and (shape, bshift) in WRAP_POWER:
            assert r["flips"]["no_wrap"] != 1, r
    assert any(r["flips"]["no_shared"] != 1 for r in inj)
    if dyn == AT and (shape, bshift) in WRAP_POWER:
        assert any(r["flips"]["no_wrap"] != 1 for r in inj)
    return inj


def _outputs(env, g=None):
    """Every output of the last reset / step, as the device tensors the kernel wrote."""
    return dict(obs=env.t_obs, node=env.t_node, adj=env.t_adj, reward=env.t_rew, dones=env.t_done, info=env.t_info,
                state=env.t_state, reset=env.t_reset, ep_info=env.t_epinfo)


def _assert_same(a, b, ctx):
    """Bit-equality on the device (a 24-env reference-layout adjacency is 226 MB as host float64)."""
    import torch
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k].contiguous().view(torch.uint8), b[k].contiguous().view(torch.uint8)
        if not torch.equal(x, y):
            np.testing.assert_array_equal(a[k].cpu().numpy(), b[k].cpu().numpy(), err_msg="%s: %s" % (ctx, k))
            raise AssertionError("%s: %s differs in bits only (NaN payload or signed zero)" % (ctx, k))


# ---- the device bounds table --------------------------------------------------------------------------
def _read_bounds(env):
    nb = (C.c_int32 * 5)()
    bs = C.c_int32(-1)
    one = np.zeros((1, 2), dtype=np.float32)
    # too small a capacity is refused, with the counts filled in
    assert env.lib.lsm_test_read_value_bounds(env.h, one.ctypes.data_as(C.c_void_p), 1, nb, C.byref(bs)) != 0
    counts = tuple(int(x) for x in nb if x)
    out = np.full((int(np.prod(counts)), 2), np.nan, dtype=np.float32)
    rc = env.lib.lsm_test_read_value_bounds(env.h, out.ctypes.data_as(C.c_void_p), out.shape[0], nb, C.byref(bs))
    assert rc == 0, env.lib.lsm_last_error(env.h)
    return out, counts, int(bs.value)


@pytest.mark.parametrize("kind", ["rough", "spike"])
@pytest.mark.parametrize("dyn,shape", [(DI, M.DI_SMALL), (DI, M.DI_WIDE), (AT, M.AT_SMALL), (AT, M.AT_WIDE)])
def test_device_bounds_table_matches_model(dyn, shape, kind):
    """bounds_kernel's table for bounds_shift 1..4 against block_bounds: equal block counts, every
    (lo, hi) bit-equal (float32, no contraction), and, whatever the formula, lo <= min and hi >= max of
    the block's nodes. Over the shapes: a partial last block, a dimension of one block, and a periodic
    dimension whose (partial) last block wraps onto node 0."""
    vt = _table(dyn, kind, shape, bshift=SHIFTS[dyn][-1][1] if shape == SHIFTS[dyn][-1][0] else 2)
    seen = dict(partial=False, single=False, wrap=False)
    for s in (1, 2, 3, 4):
        env = _gpu_env(_meta(dyn, 5, 11), vt, 1, dict(bounds_shift=s))
        dev, counts, bs = _read_bounds(env)
        env.close()
        lo_hi, nb, mn, mx = M.block_bounds(vt.values_hj, vt.periodic, s, return_minmax=True)
        assert bs == s and counts == nb, (bs, counts, nb)
        diff = (dev.view(np.uint32) != lo_hi.view(np.uint32)).any(axis=1)
        assert not diff.any(), "bshift %d: %d blocks differ, first %s" % (s, diff.sum(), np.flatnonzero(diff)[:8])
        assert (dev[:, 0].astype(np.float64) <= mn).all() and (dev[:, 1].astype(np.float64) >= mx).all()
        B = 1 << s
        for d, n in enumerate(shape):
            ncell = n if d in vt.periodic else n - 1
            seen["partial"] |= ncell % B != 0 and ncell > B
            seen["single"] |= nb[d] == 1
            seen["wrap"] |= d in vt.periodic
        print("%s %s %s bshift %d: %d blocks %s bit-equal" % (dyn, kind, shape, s, dev.shape[0], nb))
    assert seen["partial"]
    assert seen["single"] == (shape in (M.DI_WIDE, M.AT_WIDE, M.AT_SMALL))
    assert seen["wrap"] == (dyn == AT)


def test_read_value_bounds_without_table():
    """No value table (filter off): the hook refuses."""
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    meta = _meta(DI, 5, 11)
    meta["use_safety_filter"] = False
    env = GpuGraphVecEnv(EnvArgs.from_namespace(type("A", (), meta)()), num_envs=1, device="cuda:0")
    nb, bs, buf = (C.c_int32 * 5)(), C.c_int32(0), np.zeros((8, 2), dtype=np.float32)
    assert env.lib.lsm_test_read_value_bounds(env.h, buf.ctypes.data_as(C.c_void_p), 8, nb, C.byref(bs)) != 0
    assert b"no value table" in env.lib.lsm_last_error(env.h)
    env.close()


# ---- 1. pruned == full, bit for bit ---------------------------------------------------------------------
CASES_EQ = [(dyn, kind, shape, s) for dyn in (DI, AT) for kind in ("smooth", "rough", "spike")
            for shape, s in SHIFTS[dyn]]


@pytest.mark.parametrize("dyn,kind,shape,bshift", CASES_EQ)
def test_pruned_search_equals_full_search(dyn, kind, shape, bshift):
    """Two handles, same seed and actions: kernel_select(filter_search=1, bounds_shift=s) and
    (filter_search=0). 24 envs, episode_length 5, 12 steps (two auto-resets); after the initial reset
    and again after the first auto-reset the injected states go in: the spike pairs (spike table), the
    loner whose every pair is out of the grid, and (initial reset) a third of an env's agents on their
    final goals, so done agents, candidate-less egos and live egos share a wave. Every output of every
    call is bit-equal: the design claims the pruned argmin is exactly the full search's, and both runs
    are the same kernel binary with one runtime flag."""
    n_envs, epl, ep = 24, 5, 4
    vt = _table(dyn, kind, shape, bshift)
    meta = _meta(dyn, epl, 11)
    tag = "%s %s %s bshift %d" % (dyn, kind, shape, bshift)
    _assert_share(tag, _reset_share(dyn, kind, shape, bshift, vt, meta))
    inject = {}
    if kind == "spike":
        for k, r in enumerate(_spike_injections(dyn, vt, shape, bshift)):
            inject[1 + k] = (r["states"], None)
    loner = M.loner_layout(dyn, vt, N)
    view = M._StateView(dyn, vt, loner)
    st = M.prune_stats(view, vt, bshift, egos=[0])
    assert st["egos_all_out"] == 1 and st["n_in"] == 0 and np.isinf(st["upper"][0])
    inject[20] = (loner, None)
    ora21 = _oracle(meta, vt, env_offset=21)   # env 21's goals, for the agents to retire
    ora21.reset(ep)
    retire = M.arrive_subset(ora21.envs[0])

    envs = [_gpu_env(meta, vt, n_envs, dict(filter_search=1, bounds_shift=bshift), return_numpy=False),
            _gpu_env(meta, vt, n_envs, dict(filter_search=0), return_numpy=False)]
    print("%s: %s" % (tag, envs[0].kernel_name))
    outs = [_outputs(e, e.reset(ep)) for e in envs]
    _assert_same(outs[0], outs[1], tag + " reset")
    np.testing.assert_allclose(outs[0]["state"][21].cpu().numpy(), ora21.envs[0].s, rtol=0, atol=STATE_ATOL)
    for e in envs:
        for k, (s, r) in inject.items():
            e.set_agent_state(k, s, r)
        e.set_agent_state(21, *retire)
    rng = np.random.default_rng(5)
    c_dec, c_sf = _info_col("deconflicting_agent_index"), _info_col("Safety filtered")
    filtered = resets = 0
    for t in range(12):
        a = rng.integers(0, 25, (n_envs, N))
        a[21, ::3] = 12   # zero acceleration: the retired agents arrive
        outs = [_outputs(e, e.step(a, ep)) for e in envs]
        _assert_same(outs[0], outs[1], "%s step %d" % (tag, t))
        envs[1].check_actions()
        full = {k: outs[1][k].cpu().numpy() for k in ("info", "reset", "dones")}
        filtered += int(full["info"][:, :, c_sf].sum())
        resets += int(full["reset"].sum())
        if t in (0, epl):   # the step after an injection
            dec = full["info"][:, :, c_dec].astype(int)
            for k in inject:
                if k != 20:
                    assert dec[k, 0] == 1, (tag, k, dec[k, 0])   # the spike pair, as the model says
            if t == 0:
                assert full["dones"][21, ::3].all() and not full["dones"][21].all()
        if t == epl - 1:
            assert full["reset"].all()
            for e in envs:
                for k, (s, r) in inject.items():
                    e.set_agent_state(k, s, r)
    assert resets >= 2 * n_envs and filtered > 0, (resets, filtered)
    for e in envs:
        e.close()


# ---- 2. both searches anchored to the oracle ---------------------------------------------------------
def _assert_oracle_step(env, g, o, ora, ctx):
    np.testing.assert_array_equal(g[5], o[5], err_msg=ctx)
    np.testing.assert_array_equal(g[3] != 0, o[3] != 0, err_msg=ctx)
    np.testing.assert_allclose(g[0], o[0], rtol=0, atol=F32_ATOL, err_msg=ctx)
    np.testing.assert_allclose(g[2], o[2], rtol=0, atol=F32_ATOL, err_msg=ctx)
    np.testing.assert_allclose(g[3], o[3], rtol=0, atol=F32_ATOL, err_msg=ctx)
    np.testing.assert_allclose(g[4], o[4], rtol=1e-6, atol=1e-5, err_msg=ctx)
    st, info, reset = env.state().cpu().numpy(), env.t_info.cpu().numpy(), env.t_reset.cpu().numpy()
    for k, e in enumerate(ora.envs):
        np.testing.assert_allclose(st[k], e.s, rtol=0, atol=STATE_ATOL, err_msg=ctx)
        if reset[k]:
            continue   # the oracle env's per-step arrays were re-initialised by its reset
        np.testing.assert_array_equal(info[k, :, _info_col("deconflicting_agent_index")].astype(int),
                                      e.deconflicting, err_msg=ctx)
        np.testing.assert_array_equal(info[k, :, _info_col("Safety filtered")].astype(bool), e.safety_filtered,
                                      err_msg=ctx)


@pytest.mark.parametrize("kind", ["rough", "spike"])
@pytest.mark.parametrize("dyn", [DI, AT])
def test_full_and_pruned_search_match_oracle(dyn, kind):
    """filter_search=0 and filter_search=1 against OracleVecEnv on the rough and the spike table: 1 env,
    a reset plus 4 steps with episode_length 3 (one auto-reset inside), a spike pair (spike table)
    injected before each step. The project's tolerances: dones, adjacency pattern, deconflicting agent
    and 'Safety filtered' exact; obs / node / adj 1e-5; states 1e-9; rewards rtol 1e-6, atol 1e-5."""
    shape, bshift = SHIFTS[dyn][0]
    vt = _table(dyn, kind, shape, bshift)
    meta = _meta(dyn, 3, 11)
    ep = 4
    tag = "%s %s %s bshift %d" % (dyn, kind, shape, bshift)
    inj = _spike_injections(dyn, vt, shape, bshift) if kind == "spike" else []
    ora = _oracle(meta, vt)
    envs = [_gpu_env(meta, vt, 1, dict(filter_search=0)),
            _gpu_env(meta, vt, 1, dict(filter_search=1, bounds_shift=bshift))]
    print("%s: %s" % (tag, envs[0].kernel_name))
    o = ora.reset(ep)
    _assert_share(tag, M.prune_stats(ora.envs[0], vt, bshift))
    for e in envs:
        g = e.reset(ep)
        np.testing.assert_allclose(g[0], o[0], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g[2], o[2], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g[3], o[3], rtol=0, atol=F32_ATOL)
    rng = np.random.default_rng(6)
    resets = []
    for t in range(4):
        if inj:
            r = inj[t % len(inj)]
            M.inject(ora.envs[0], r["states"])
            for e in envs:
                e.set_agent_state(0, r["states"])
        a = rng.integers(0, 25, (1, N))
        o = ora.step(a, ep)
        for name, e in zip(("full", "pruned"), envs):
            _assert_oracle_step(e, e.step(a, ep), o, ora, "%s %s step %d" % (tag, name, t))
        resets.append(bool(envs[0].t_reset.cpu().numpy()[0]))
        if inj and not resets[-1]:   # (a reset re-initialises the oracle env's per-step arrays)
            assert ora.envs[0].deconflicting[0] == 1
    assert resets == [False, False, True, False], resets   # one auto-reset inside
    for e in envs:
        e.close()


# ---- 3. pruning under the separation chain -------------------------------------------------------------
def test_pruned_search_under_separation_chain():
    """Separation curriculum at N = 64 (table uploaded at separation 0): value_bounds shifts and re-widens
    the bounds by each env's own chain. Resets through the stair levels ep = 0, 4, 8, 12, 16, 12, 8, 4,
    8, 12, 16 (10 changes: past the record's 8 slots, so the bounds read the HBM overflow row too), 2 steps
    after each: pruned and full bit-equal on every output, and at the last two resets env 0 against the
    oracle (which followed every reset, so its table went through the same shifts)."""
    dyn, kind, (shape, bshift) = DI, "rough", SHIFTS[DI][1]
    vt = _table(dyn, kind, shape, separation=0)
    meta = _meta(dyn, 5, 1, separation_distance_curriculum=True)
    meta["num_env_steps"] = 5 * 20
    n_envs = 4
    envs = [_gpu_env(meta, vt, n_envs, dict(filter_search=1, bounds_shift=bshift)),
            _gpu_env(meta, vt, n_envs, dict(filter_search=0))]
    print("separation chain: %s" % envs[0].kernel_name)
    ora = _oracle(meta, vt)
    seq = [0, 4, 8, 12, 16, 12, 8, 4, 8, 12, 16]
    rng = np.random.default_rng(3)
    seps = []
    for k, ep in enumerate(seq):
        o = ora.reset(ep)
        seps.append(ora.envs[0].hj_sep)
        gs = [e.reset(ep) for e in envs]
        _assert_same(_outputs(envs[0]), _outputs(envs[1]), "reset %d (ep %d)" % (k, ep))
        np.testing.assert_allclose(gs[0][0][:1], o[0], rtol=0, atol=F32_ATOL)
        last = k >= len(seq) - 2
        if k == len(seq) - 1:
            _assert_share("separation chain, level of ep %d (separation %.3f)" % (ep, seps[-1]),
                          M.prune_stats(ora.envs[0], None, bshift))
        for t in range(2):
            a = rng.integers(0, 25, (n_envs, N))
            gs = [e.step(a, ep) for e in envs]
            _assert_same(_outputs(envs[0], gs[0]), _outputs(envs[1], gs[1]), "reset %d (ep %d) step %d" % (k, ep, t))
            if last:
                o = ora.step(a[:1], ep)
                for name, e, g in zip(("pruned", "full"), envs, gs):
                    ctx = "%s reset %d (ep %d) step %d" % (name, k, ep, t)
                    np.testing.assert_array_equal(g[5][:1], o[5], err_msg=ctx)
                    np.testing.assert_array_equal(g[3][:1] != 0, o[3] != 0, err_msg=ctx)
                    np.testing.assert_allclose(g[0][:1], o[0], rtol=0, atol=F32_ATOL, err_msg=ctx)
                    np.testing.assert_allclose(g[2][:1], o[2], rtol=0, atol=F32_ATOL, err_msg=ctx)
                    np.testing.assert_allclose(g[3][:1], o[3], rtol=0, atol=F32_ATOL, err_msg=ctx)
                    np.testing.assert_allclose(g[4][:1], o[4], rtol=1e-6, atol=1e-5, err_msg=ctx)
                    np.testing.assert_allclose(e.state().cpu().numpy()[0], ora.envs[0].s, rtol=0, atol=STATE_ATOL,
                                               err_msg=ctx)
                    info = e.t_info.cpu().numpy()[0]
                    np.testing.assert_array_equal(info[:, _info_col("deconflicting_agent_index")].astype(int),
                                                  ora.envs[0].deconflicting, err_msg=ctx)
    assert sum(a != b for a, b in zip(seps[:-1], seps[1:])) == 10, seps
    for e in envs:
        e.close()


# ---- 4. selectors are honoured or refused ---------------------------------------------------------------
def _small_env(n_agents, ksel):
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    meta = _meta(DI, 5, 11)
    meta["num_agents"] = n_agents
    return GpuGraphVecEnv(EnvArgs.from_namespace(type("A", (), meta)()), num_envs=2, device="cuda:0",
                          small_tables=True, kernel_select=ksel)


def test_team_selector_is_honoured_or_refused():
    """team > 0 where the configuration has no team kernel is an error, not a silent rollout_kernel."""
    from lsm import capi
    with pytest.raises(capi.LsmError, match="team"):
        _small_env(5, dict(team=4))
    with pytest.raises(capi.LsmError, match="team"):
        _small_env(8, dict(team=4, workgroup_per_env=1))
    with pytest.raises(capi.LsmError, match="team"):
        _small_env(8, dict(team=4, generic=1))
    with pytest.raises(capi.LsmError, match="team"):
        _small_env(8, dict(team=4, lanes_per_env=32))
    env = _small_env(8, dict(team=4))
    assert env.kernel_name.startswith("rollout_team_kernel<0, 8, 4,"), env.kernel_name
    env.close()
    env = _small_env(5, dict(team=0))      # "no team kernel" stays a valid request everywhere
    assert env.kernel_name.startswith("rollout_kernel<"), env.kernel_name
    env.close()


@pytest.mark.parametrize("ksel,word", [(dict(filter_search=2), "filter_search"), (dict(bounds_shift=5), "bounds_shift"),
                                       (dict(bounds_shift=-1), "bounds_shift")])
def test_search_selectors_out_of_range_are_refused(ksel, word):
    from lsm import capi
    with pytest.raises(capi.LsmError, match=word):
        _small_env(5, ksel)
