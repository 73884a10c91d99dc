"""Which step kernel a configuration gets (csrc/lsm_kernels.h's table, lsm_host.hip's choose_kernel):
``lsm_kernel_name_for`` is the pure selection function behind ``lsm_create_select``, so the rules are
checked here without a GPU. The expected names and error texts were recorded from
``lsm_create_select`` + ``lsm_kernel_name`` / ``lsm_last_error`` of the commit before the kernel table
existed; the GPU test at the end ties the handle to the pure function."""
import ctypes as C

import pytest

from lsm import capi

DI, AT = capi.LSM_DOUBLE_INTEGRATOR, capi.LSM_AIRTAXI
LAYOUT, DEPART = capi.LSM_SCENARIO_LAYOUT, capi.LSM_SCENARIO_DEPARTURES

# defaults of every case: L = 2, the training scenario, num_internal_step = 0, no reward terms
BASE = dict(dynamics=DI, num_envs=1, num_agents=8, num_landmarks=2, episode_length=25, use_safety_filter=0,
            use_masking=1, auto_reset=1, emit_edges=0, adj_layout=capi.ADJ_REFERENCE, world_size=2.0, seed=1,
            env_offset=0, collision_forces=0, scenario=capi.LSM_SCENARIO_TRAIN, rng=capi.LSM_RNG_MT19937,
            num_internal_step=0, reward_terms=0, collaborative=0)

TEAM_TEXT = ("kernel select: team > 0 needs a team kernel instantiation (double integrator N = 8 or "
             "airtaxi N = 16, 2 landmarks, lanes_per_env 64, num_internal_step <= 1, the training "
             "scenario, neither generic nor workgroup_per_env)")
TEAM_LANES_TEXT = "kernel select: team * num_agents must be <= 64"
LANES_TEXT = "kernel select: lanes_per_env must be 16, 32 or 64 and >= num_agents"
AT16_LAYOUT = dict(dynamics=AT, num_agents=16, scenario=LAYOUT, auto_reset=0)

# (id, lsm_config overrides, lsm_kernel_select overrides, kernel name)
NAMES = [
    ("di8", dict(), dict(), "rollout_team_kernel<0, 8, 4, false>"),
    ("di8-collab", dict(collaborative=1), dict(), "rollout_team_kernel<0, 8, 4, true>"),
    ("di8-rw1", dict(reward_terms=1), dict(), "rollout_team_kernel<0, 8, 4, true>"),
    ("di8-team0", dict(), dict(team=0), "rollout_kernel<0, 64, 8>"),
    ("di8-team2", dict(), dict(team=2), "rollout_team_kernel<0, 8, 2, false>"),
    ("di8-team8", dict(), dict(team=8), "rollout_team_kernel<0, 8, 8, false>"),
    ("di8-lpe32", dict(), dict(lanes_per_env=32), "rollout_kernel<0, 32, 8>"),
    ("di8-lpe16", dict(), dict(lanes_per_env=16), "rollout_kernel<0, 16, 0>"),
    ("di8-generic", dict(), dict(generic=1), "rollout_kernel<0, 64, 0>"),
    ("di8-nis2", dict(num_internal_step=2), dict(), "rollout_kernel<0, 64, 8>"),
    ("di8-nis1", dict(num_internal_step=1), dict(), "rollout_team_kernel<0, 8, 4, false>"),
    ("di8-l3", dict(num_landmarks=3), dict(), "rollout_kernel<0, 64, 0>"),
    ("di3", dict(num_agents=3), dict(), "rollout_kernel<0, 64, 3>"),
    ("di4", dict(num_agents=4), dict(), "rollout_kernel<0, 64, 0>"),
    ("di8-wg", dict(), dict(workgroup_per_env=1), "rollout_block_kernel<0, 0, true, false>"),
    ("di33", dict(num_agents=33), dict(), "rollout_block_kernel<0, 0, true, false>"),
    ("di16-l4", dict(num_agents=16, num_landmarks=4), dict(), "rollout_block_kernel<0, 0, true, false>"),
    ("di64", dict(num_agents=64), dict(), "rollout_block_kernel<0, 64, true, false>"),
    ("di64-rw15", dict(num_agents=64, reward_terms=15), dict(), "rollout_block_kernel<0, 64, true, true>"),
    ("di64-nis3", dict(num_agents=64, num_internal_step=3), dict(), "rollout_block_kernel<0, 64, false, true>"),
    ("di64-generic", dict(num_agents=64), dict(generic=1), "rollout_block_kernel<0, 0, true, false>"),
    ("at64", dict(dynamics=AT, num_agents=64), dict(), "rollout_block_kernel<1, 64, true, false>"),
    ("at16", dict(dynamics=AT, num_agents=16), dict(), "rollout_team_kernel<1, 16, 4, false>"),
    ("at16-team2", dict(dynamics=AT, num_agents=16), dict(team=2), "rollout_team_kernel<1, 16, 2, false>"),
    ("at16-team0", dict(dynamics=AT, num_agents=16), dict(team=0), "rollout_kernel<1, 64, 16>"),
    ("at16-lpe32", dict(dynamics=AT, num_agents=16), dict(lanes_per_env=32), "rollout_kernel<1, 32, 16>"),
    ("at16-lpe16", dict(dynamics=AT, num_agents=16), dict(lanes_per_env=16), "rollout_kernel<1, 16, 0>"),
    ("at3", dict(dynamics=AT, num_agents=3), dict(), "rollout_kernel<1, 64, 3>"),
    ("at16-layout", AT16_LAYOUT, dict(), "rollout_kernel<1, 64, 0>"),
    # E = 96 entities: the workgroup kernel, where lanes_per_env does not apply
    ("di32-lpe16", dict(num_agents=32), dict(lanes_per_env=16), "rollout_block_kernel<0, 0, true, false>"),
]

# (id, lsm_config overrides, lsm_kernel_select overrides, error text)
ERRORS = [
    # kernel choices that are refused
    ("di4-team4", dict(num_agents=4), dict(team=4), TEAM_TEXT),
    ("di8-wg-team4", dict(), dict(workgroup_per_env=1, team=4), TEAM_TEXT),
    ("at16-team8", dict(dynamics=AT, num_agents=16), dict(team=8), TEAM_LANES_TEXT),
    ("at16-layout-team4", AT16_LAYOUT, dict(team=4), TEAM_TEXT),
    ("di20-lpe16", dict(num_agents=20), dict(lanes_per_env=16), LANES_TEXT),
    # lsm_config validation, one case per message
    ("dynamics", dict(dynamics=2), dict(), "dynamics must be LSM_DOUBLE_INTEGRATOR or LSM_AIRTAXI"),
    ("agents-1", dict(num_agents=1), dict(), "num_agents must be in [2, 64]"),
    ("agents-65", dict(num_agents=65), dict(), "num_agents must be in [2, 64]"),
    ("landmarks-1", dict(num_landmarks=1), dict(),
     "num_landmarks must be in [2, 8] (the training scenario asserts > 1, utils.py:31; layout scenarios: [1, 8])"),
    ("entities-257", dict(num_agents=64, num_landmarks=4), dict(), "N * (1 + L) must be <= 256"),
    ("landmark-ids", dict(num_agents=32, num_landmarks=5), dict(),
     "landmark ids go through np.int8 (navigation_graph_safe.py:581)"),
    ("adj-layout", dict(adj_layout=2), dict(), "adj_layout must be LSM_ADJ_REFERENCE or LSM_ADJ_COMPACT"),
    ("scenario", dict(scenario=3), dict(), "scenario must be LSM_SCENARIO_TRAIN, _LAYOUT or _DEPARTURES"),
    ("rng", dict(rng=2), dict(), "rng must be LSM_RNG_MT19937 or LSM_RNG_PHILOX"),
    ("layout-auto-reset", dict(scenario=LAYOUT, auto_reset=1), dict(),
     "layout scenarios are evaluation paths (GraphDummyVecEnv, scripts/eval_mpe.py): auto_reset must be 0"),
    ("layout-philox", dict(scenario=LAYOUT, auto_reset=0, rng=capi.LSM_RNG_PHILOX), dict(),
     "layout scenarios draw on the host: rng must be LSM_RNG_MT19937"),
    ("departures-di", dict(scenario=DEPART, auto_reset=0), dict(),
     "departure timers need airtaxi dynamics (RealisticScenario calls reset_velocity(theta, speed), "
     "KinematicVehicleXYState only, core.py:137)"),
    ("envs-0", dict(num_envs=0), dict(), "num_envs must be >= 1"),
    ("nis-65", dict(num_internal_step=65), dict(), "num_internal_step must be in [0, 64] (0 and 1: one inner step)"),
    ("episode-0", dict(episode_length=0), dict(), "episode_length must be >= 1"),
    ("reward-bit", dict(reward_terms=16), dict(),
     "reward_terms: unknown LSM_REWARD_* bits (RewardBinaryConfig has four optional terms, "
     "multiagent/config.py:78-83)"),
    ("collab-2", dict(collaborative=2), dict(), "collaborative must be 0 or 1"),
    # lsm_kernel_select validation, one case per field
    ("sel-wg", dict(), dict(workgroup_per_env=2), "kernel select: workgroup_per_env must be 0 or 1"),
    ("sel-generic", dict(), dict(generic=2), "kernel select: generic must be 0 or 1"),
    ("sel-lanes", dict(), dict(lanes_per_env=8), "kernel select: lanes_per_env must be 0, 16, 32 or 64"),
    ("sel-team", dict(), dict(team=3), "kernel select: team must be -1, 0, 2, 4 or 8"),
    ("sel-lean", dict(), dict(lean=2), "kernel select: lean must be -1, 0 or 1"),
    ("sel-search", dict(), dict(filter_search=2), "kernel select: filter_search must be -1, 0 or 1"),
    ("sel-bounds", dict(), dict(bounds_shift=5), "kernel select: bounds_shift must be in [0, 4]"),
]

# the 34 instantiated step kernels (csrc/lsm_kernels.h)
TABLE = (
    ["rollout_kernel<%d, %d, 0>" % (d, lpe) for d in (0, 1) for lpe in (64, 32, 16)] +
    ["rollout_kernel<0, 32, 8>", "rollout_kernel<0, 64, 3>", "rollout_kernel<0, 64, 8>",
     "rollout_kernel<1, 32, 16>", "rollout_kernel<1, 64, 3>", "rollout_kernel<1, 64, 16>"] +
    ["rollout_team_kernel<0, 8, %d, %s>" % (g, r) for g in (8, 4, 2) for r in ("false", "true")] +
    ["rollout_team_kernel<1, 16, %d, %s>" % (g, r) for g in (4, 2) for r in ("false", "true")] +
    ["rollout_block_kernel<%d, %d, %s>" % (d, nt, c) for d in (0, 1) for nt in (64, 0)
     for c in ("false, true", "true, true", "true, false")])


def _ids(cases):
    return [c[0] for c in cases]


def config(overrides):
    return capi.LsmConfig(**dict(BASE, **overrides))


def name_for(lib, cfg_over, sel_over, default_sel_as_null=True):
    """(rc, text) of lsm_kernel_name_for; an empty select goes as NULL (the defaults, as in lsm_create)."""
    buf = C.create_string_buffer(512)
    cfg = config(cfg_over)
    sel = None if (not sel_over and default_sel_as_null) else C.byref(capi.kernel_select(**sel_over))
    rc = lib.lsm_kernel_name_for(C.byref(cfg), sel, buf, len(buf))
    return rc, buf.value.decode()


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("cfg,sel,want", [c[1:] for c in NAMES], ids=_ids(NAMES))
def test_kernel_name(lib, cfg, sel, want):
    assert name_for(lib, cfg, sel) == (0, want)


@pytest.mark.parametrize("cfg,sel,want", [c[1:] for c in ERRORS], ids=_ids(ERRORS))
def test_refusal_text(lib, cfg, sel, want):
    assert name_for(lib, cfg, sel) == (1, want)


def test_null_select_is_the_default_select(lib):
    for _, cfg, sel, _ in NAMES + ERRORS:
        if not sel:
            assert name_for(lib, cfg, sel) == name_for(lib, cfg, sel, default_sel_as_null=False)


def test_names_come_from_the_table_and_cover_it(lib):
    assert len(set(TABLE)) == 34
    got = {name_for(lib, cfg, sel)[1] for _, cfg, sel, _ in NAMES}
    assert got <= set(TABLE)
    for dyn in (0, 1):
        for family in ("rollout_kernel", "rollout_team_kernel", "rollout_block_kernel"):
            assert any(n.startswith("%s<%d," % (family, dyn)) for n in got), (family, dyn)


def test_short_buffer_is_refused_not_overrun(lib):
    buf = C.create_string_buffer(b"\xff" * 16, 16)
    cfg = config({})
    assert lib.lsm_kernel_name_for(C.byref(cfg), None, buf, 8) == 1
    assert buf.raw[8:] == b"\xff" * 8 and b"\0" in buf.raw[:8]


# one row per family and dynamics, and two refusals: the handle agrees with the pure function
HANDLE_NAMES = ["di8", "di3", "di64-nis3", "at16", "at16-lpe32", "at64"]
HANDLE_ERRORS = ["di4-team4", "at16-team8"]


@pytest.mark.gpu
def test_handle_agrees_with_pure_function(lib):
    cases = {c[0]: c for c in NAMES + ERRORS}
    families = set()
    for key in HANDLE_NAMES + HANDLE_ERRORS:
        _, cfg_over, sel_over, want = cases[key]
        rc, text = name_for(lib, cfg_over, sel_over)
        assert text == want
        cfg = config(cfg_over)
        h = C.c_void_p()
        got_rc = lib.lsm_create_select(C.byref(cfg), C.byref(capi.kernel_select(**sel_over)), C.byref(h))
        try:
            assert got_rc == rc == (1 if key in HANDLE_ERRORS else 0)
            got = lib.lsm_last_error(h) if rc else lib.lsm_kernel_name(h)
            assert got.decode() == text
        finally:
            lib.lsm_destroy(h)
        if not rc:
            families.add((text.split("<")[0], cfg.dynamics))
    assert len(families) == 6
