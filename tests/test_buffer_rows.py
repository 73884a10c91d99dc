"""CPU conditions on the runs of tests/test_gpu_buffer_kernels.py, from the oracle alone: the replayed runs
can tell right replay-buffer rows from wrong ones, and the cases name every kernel the library has."""
import numpy as np
import pytest

import buffer_rows as BR
import filter_layouts as FL

SPECS = sorted({(v[0], v[1], v[2]) for v in FL.kernel_variants()})
# envs that share a wave (2 or 4 envs per wave) or a team workgroup with a live env
SHARED = ((4, 5, 6, 7), (FL.ENV_THIRD, FL.ENV_LONER2))


def test_cases_name_every_kernel_row():
    """Sections 1 and 2 together run every row of csrc/lsm_kernels.h, W, T and B, each exactly as the host's
    kernel table spells it; the extra runs of section 1 are rows of FL.kernel_variants()."""
    rows = BR.header_rows()
    assert len(rows) == len(set(rows)) == 34, sorted(rows)
    blocks = [c[6] for c in BR.block_cases()]
    named = {v[5] for v in FL.kernel_variants()}
    assert len(blocks) == len(set(blocks)) == 10 and not named & set(blocks)
    assert named | set(blocks) == set(rows), sorted(set(rows) ^ (named | set(blocks)))
    dec, comp = BR.pick(BR.NOT_CENTRALIZED), BR.pick(BR.COMPACT)
    # not centralized: an airtaxi N = 16 team row, a 4-envs-per-wave row, the generic workgroup row
    assert [v[5] for v in dec] == ["rollout_team_kernel<1, 16, 4, false>", "rollout_kernel<0, 16, 0>",
                                   "rollout_block_kernel<0, 0, true, false>"]
    # compact adjacency: one per family
    assert [v[5].split("<")[0] for v in comp] == ["rollout_kernel", "rollout_team_kernel", "rollout_block_kernel"]


def test_block_case_meta_selects_the_rows():
    """lsm_kernel_name_for (the pure selection function) answers each block case's row for its configuration."""
    import ctypes as C
    from lsm import build, capi
    build.build(verbose=False)
    lib = capi.load_library()
    for dyn, N, label, meta, ksel, layout, kernel in BR.block_cases():
        cfg = capi.LsmConfig(dynamics=capi.LSM_DOUBLE_INTEGRATOR if dyn == FL.DI else capi.LSM_AIRTAXI,
                             num_envs=BR.B_ENVS, num_agents=N, num_landmarks=2, episode_length=BR.B_EPISODE,
                             use_safety_filter=1, use_masking=1, auto_reset=1, emit_edges=0,
                             adj_layout=capi.ADJ_COMPACT if layout == "compact" else capi.ADJ_REFERENCE,
                             world_size=float(meta["world_size"]), seed=meta["seed"], env_offset=0,
                             collision_forces=0, scenario=capi.LSM_SCENARIO_TRAIN, rng=capi.LSM_RNG_MT19937,
                             num_internal_step=meta["num_internal_step"],
                             reward_terms=sum(capi.REWARD_BITS[k] for k in meta.get("reward_terms", ())),
                             collaborative=int(meta.get("collaborative", False)))
        buf = C.create_string_buffer(256)
        sel = C.byref(capi.kernel_select(**ksel)) if ksel else None
        assert lib.lsm_kernel_name_for(C.byref(cfg), sel, buf, len(buf)) == 0, buf.value
        assert buf.value.decode() == kernel, (label, N)


@pytest.mark.parametrize("dyn,N,rext", SPECS, ids=["%s%d%s" % (d[:2], n, "-rext" if r else "") for d, n, r in SPECS])
def test_run_holds_every_mask_state_and_both_reset_rows(dyn, N, rext):
    """FL.oracle_run into a buffer of length BUF_T: the expected masks / active_masks rows hold live (1, 1),
    done in a live env (0, 0) and done in an all-done env (0, 1); (0, 0) occurs in envs 4..7 and in envs 9, 10,
    next to envs with live agents in the same step; the auto-resets land in a middle row and in row T."""
    run = FL.oracle_run(dyn, N, "rough", rext)
    dones = [r["dones"] for r in run["steps"]]
    states = BR.mask_states(dones)
    assert all(states.values()), {k: len(v) for k, v in states.items()}
    for group in SHARED:
        hits = [(t, k) for t, k, _ in states["done_in_live_env"] if k in group]
        assert hits, group
        # in such a step another env of the group is wholly live or holds live agents
        assert any((~dones[t][[g for g in group if g != k]]).any() for t, k in hits), group
    assert {k for _, k, _ in states["done_in_live_env"]} >= {FL.ENV_SOLE, FL.ENV_THIRD, FL.ENV_LONER2}
    # (0, 1): every agent of an env that auto-resets; both states in one step (the wave's all_done differs per env)
    resets = [t for t, r in enumerate(run["steps"]) if r["reset"].any()]
    assert resets == [FL.EPISODE_LENGTH - 1, 2 * FL.EPISODE_LENGTH - 1]
    for t in resets:
        assert dones[t].all() and {(t, k, i) for k in range(FL.N_ENVS) for i in range(N)} <= set(
            states["done_in_done_env"])
    rows = BR.reset_rows(resets, BR.BUF_T)
    assert rows == [2, BR.BUF_T] and 0 < rows[0] < BR.BUF_T
    assert BR.BUF_T != FL.EPISODE_LENGTH and FL.STEPS > 2 * BR.BUF_T   # after_update moves row T to row 0, twice
    print("%s N=%d rext=%d: %s; auto-resets in rows %s of %d" % (
        dyn, N, rext, {k: len(v) for k, v in states.items()}, rows, BR.BUF_T + 1))


@pytest.mark.parametrize("case", [c for c in BR.block_cases() if c[1] < 64],
                         ids=lambda c: "%s%d-%s" % (c[0][:2], c[1], c[2]))
def test_block_run_holds_every_mask_state(case):
    """Section 2's run at the small agent counts, through the oracle: the agents injected after the reset and
    after the first auto-reset are done after the next step and no other agent is (BR.arrived_only), the
    auto-resets fall on steps 2 and 5 (rows 1 and T of a buffer of length 2), and the dones hold all three
    mask states. At N = 64 the GPU test asserts the same of the plain env's dones."""
    dyn, N, label, meta, ksel, layout, kernel = case
    ora = FL.oracle_vec(meta, FL.table(dyn, "rough"), n_envs=BR.B_ENVS)
    ora.reset(FL.EP)
    inj, acts = BR.block_injections(meta), BR.block_actions(N)
    dones, resets = [], []
    for t in range(BR.B_STEPS):
        if t in BR.B_INJECT_AT:
            s, r = inj[BR.B_INJECT_AT.index(t)]
            # the never-stepped oracle env's reset is this env's: only the arrived agents differ
            keep = np.ones(N, bool)
            keep[::BR.B_EVERY] = False
            np.testing.assert_array_equal(s[keep], ora.envs[0].s[keep])
            FL.M.inject(ora.envs[0], s, r)
        o = ora.step(acts[t], FL.EP)
        d = np.asarray(o[5])
        if t in BR.B_INJECT_AT:
            assert BR.arrived_only(d[0]), (t, d[0])
        dones.append(d)
        if any(len(x) > N for x in o[6]):
            resets.append(t)
    assert resets == [BR.B_EPISODE - 1, 2 * BR.B_EPISODE - 1]
    assert BR.reset_rows(resets, BR.B_BUF_T) == [1, BR.B_BUF_T]
    states = BR.mask_states(dones)
    assert all(states.values()), {k: len(v) for k, v in states.items()}
