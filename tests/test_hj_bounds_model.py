"""CPU checks of the facts that make the bound-pruned HJ argmin exact (tests/hj_bounds_model.py): an
interpolated value never leaves its block's (lo, hi), the minimum is never above the smallest upper
bound, and the 4e-6 widening covers the float32 interpolation's excursion outside its corners' range."""
import numpy as np
import pytest

import hj_bounds_model as M
from golden_replay import table_dict
from oracle.hj_grid import Grid

F32 = np.float32


def _oracle_env(dyn, vt, seed=11):
    from lsm import hj_tables
    from oracle.lsm_oracle import OracleVecEnv
    di = dyn == "double_integrator"
    meta = dict(dynamics_type=dyn, num_agents=24, num_landmarks=2, world_size=4 if di else 6, episode_length=5,
                num_env_steps=20, n_rollout_threads=1, use_safety_filter=True, use_masking=True,
                num_internal_step=1, seed=seed, env_seed=seed)
    tt = None if di else hj_tables.ttr_table_from_stored(hj_tables.synthetic_ttr((25, 25, 24, 7)))
    ora = OracleVecEnv(meta, 1, seed=seed, value_table=table_dict(vt), ttr_table=table_dict(tt),
                       integrator="restated")
    ora.reset(4)
    return ora.envs[0]


@pytest.mark.parametrize("kind", ["smooth", "rough"])
@pytest.mark.parametrize("dyn,shape", [("double_integrator", M.DI_SMALL), ("airtaxi", M.AT_SMALL)])
def test_interpolated_value_within_block_bounds(dyn, shape, kind):
    """552 oracle pairs (24 agents at reset) per table, bounds_shift 1..4: every in-grid pair's float32
    interpolated value lies inside its block's [lo, hi], and each ego's minimum value is <= U, the
    smallest upper bound of its in-grid pairs -- so no pruned pair (lo > U) can be the argmin."""
    vt = M.make_table(dyn, kind, shape)
    env = _oracle_env(dyn, vt)
    pairs = M.pair_table(env)
    assert sum(len(r) for r in pairs.values()) == 24 * 23
    for s in (1, 2, 3, 4):
        st = M.prune_stats(env, vt, s, pairs=pairs)
        assert st["n_in"] > 200, st["n_in"]
        assert st["bound_violations"] == 0, (s, st["bound_violations"])
        for i, U in st["upper"].items():
            assert st["min_value"][i] <= U, (s, i)
            assert st["pruned_argmin"][i] == st["argmin"][i], (s, i)
        print("%s %s bshift %d: in-grid %d, out %d, pruned share %.3f" % (dyn, kind, s, st["n_in"], st["n_out"],
                                                                          st["share"]))


def test_block_bounds_layout_and_mutants():
    """Block node sets: clipped last block, shared boundary node, periodic wrap; C order over blocks."""
    sets = M.block_node_sets(7, False, 1)                      # 6 cells, B = 2
    assert [list(s) for s in sets] == [[0, 1, 2], [2, 3, 4], [4, 5, 6]]
    sets = M.block_node_sets(6, True, 2)                       # 6 cells (periodic), B = 4: partial last block wraps
    assert [list(s) for s in sets] == [[0, 1, 2, 3, 4], [4, 5, 0]]
    assert [list(s) for s in M.block_node_sets(6, True, 2, "no_wrap")] == [[0, 1, 2, 3, 4], [4, 5]]
    assert [list(s) for s in M.block_node_sets(7, False, 1, "no_shared")] == [[0, 1], [2, 3], [4, 5]]
    assert [list(s) for s in M.block_node_sets(3, False, 3)] == [[0, 1, 2]]   # one block
    v = np.arange(7 * 6, dtype=F32).reshape(7, 6)
    lo_hi, nb, mn, mx = M.block_bounds(v, (1,), 1, return_minmax=True)
    assert nb == (3, 3) and lo_hi.shape == (9, 2)
    # block (1, 2): rows 2..4, columns 4, 5, 0
    assert mn[1 * 3 + 2] == v[2, 0] and mx[1 * 3 + 2] == v[4, 5]
    m = F32(4e-6) * F32(v[4, 5])
    assert lo_hi[5, 0] == F32(v[2, 0] - m) and lo_hi[5, 1] == F32(v[4, 5] + m)


@pytest.mark.parametrize("ndim", [4, 5])
def test_interpolation_excursion_below_margin(ndim):
    """The float32 sum of 2^d weighted corners can leave [min, max] of the corners; the bounds are
    widened by 4e-6 max|v| for it. 20 000 random points each on a constant table (where every rounding
    error shows as an excursion: measured 3.4e-7 |v| in 4-D, 4.3e-7 |v| in 5-D) and on a rough one
    (measured 0), against the float64 convex combination's range."""
    shape = (5, 4, 6, 3, 4)[:ndim]
    per = (2,) if ndim == 5 else ()
    lo, hi = -np.ones(ndim), np.ones(ndim)
    grid = Grid(lo, hi, shape, per)
    rng = np.random.default_rng(ndim)
    worst = {}
    for name, vals in (("constant", np.full(shape, F32(-3.7), dtype=F32)),
                       ("rough", rng.uniform(-4, 4, shape).astype(F32))):
        flat = vals.reshape(-1).astype(np.float64)
        exc = dev = 0.0
        for p in rng.uniform(-1, 1, (20000, ndim)):
            idx, w = grid.corners(p)
            v32 = float(grid.interpolate(vals, p))
            c = flat[idx]
            scale = np.abs(c).max()
            exc = max(exc, max(0.0, c.min() - v32, v32 - c.max()) / scale)
            dev = max(dev, abs(v32 - float(np.dot(w.astype(np.float64), c))) / scale)
        worst[name] = exc
        print("%d-D %s table: largest excursion outside the corners' range %.3g max|v| "
              "(float32 sum vs float64 sum of the same weights: %.3g max|v|); margin 4e-6" % (ndim, name, exc, dev))
        assert exc < 4e-6, (name, exc)
    assert worst["constant"] > 0.0   # the measurement has teeth: roundings do leave the range


@pytest.mark.parametrize("dyn,shape,bshift", [("double_integrator", M.DI_SMALL, 1), ("airtaxi", M.AT_SMALL, 1)])
def test_spike_injections_have_power(dyn, shape, bshift):
    """The injected spike pairs: the partner is the exact argmin, the right bounds keep it, and bounds
    that forget the shared / last / wrap node prune it (the argmin flips)."""
    vt = M.make_table(dyn, "spike", shape, bshift=bshift)
    inj = M.spike_injections(dyn, vt, bshift, 64)
    assert {(r["name"], r["side"]) for r in inj} >= {("shared", "below"), ("shared", "above"), ("last", "below")}
    for r in inj:
        assert r["argmin"] == 1 and r["pruned_argmin"] == 1, r
        if r["side"] == "below":
            assert r["flips"]["no_shared"] != 1, r
        if r["name"] == "wrap" and r["side"] == "below":
            assert r["flips"]["no_wrap"] != 1, r
