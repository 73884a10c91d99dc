"""Replay-buffer rows written in place through every step kernel (tests/buffer_rows.py has the cases and
the checks; tests/test_buffer_rows.py the CPU conditions on them).

The learner reads the buffer's rows only. DeviceGraphBuffer ring-binds the env's obs / node_obs / adj /
reward slots to them and, with a centralized critic, has the step kernel write share_obs (write_obs'
second loop), masks and active_masks (write_masks) as well. Here every row of csrc/lsm_kernels.h fills a
buffer next to a plainly bound env of the same kernel: 2 and 4 envs per wave with a partly filled last
wave, the generic kernels, airtaxi's OBS = 6, the team kernels at every G, the workgroup kernels up to
N = 64, the REXT kernels' (n, N, 1) rewards under the reward ring's offset of -1; then the ring's KParams
array rebuilt under a selected index (the separation chain's overflow rows, a re-uploaded table), and the
ring ABI itself on slots, strides, counts and offsets that DeviceGraphBuffer does not use."""
import ctypes as C

import numpy as np
import pytest

import buffer_rows as BR
import filter_layouts as FL

pytestmark = pytest.mark.gpu

VARIANTS = FL.kernel_variants()
RUNS = ([v + (True, "reference") for v in VARIANTS] +
        [v + (False, "reference") for v in BR.pick(BR.NOT_CENTRALIZED)] +
        [v + (True, "compact") for v in BR.pick(BR.COMPACT)])


def _run_id(c):
    return BR.variant_id(c) + ("" if c[6] else "-decentralized") + ("-compact" if c[7] == "compact" else "")


@pytest.mark.parametrize("dyn,N,rext,label,ksel,kernel,centralized,layout", RUNS, ids=[_run_id(c) for c in RUNS])
def test_gpu_buffer_rows_through_every_kernel(dyn, N, rext, label, ksel, kernel, centralized, layout):
    """FL.oracle_run's 15 envs x 14 steps (auto-resets at steps 5 and 11, every third agent done in env 9, a
    sole survivor in env 5, one retired agent in env 10) into a buffer of length 4: the auto-resets land in
    row 2 and in the carry row 4. After warmup and after every step: the row written bit-equal to the plain
    env's outputs and to runner_insert of them; masks / active_masks exactly, share_obs within 1e-5 of
    runner_insert of the oracle's own obs and dones; every other row byte for byte as before the call; the
    ring-bound env's own tensors still the sentinel. After detach() the env writes its own tensors again."""
    run = FL.oracle_run(dyn, N, "rough", rext)
    pair = BR.Pair(run["meta"], FL.N_ENVS, ksel, kernel, BR.BUF_T, centralized, layout)
    try:
        pair.warmup(FL.EP)
        pair.check_oracle(0, run["reset"]["obs"], None, "warmup")
        rows = []
        for t, r in enumerate(run["steps"]):
            for k, inj in r["inject"].items():
                pair.inject(k, inj["states"], inj["reached"])
            ctx = "%s step %d" % (label, t)
            row, dones = pair.step(r["a"], FL.EP, ctx)
            np.testing.assert_array_equal(dones, r["dones"], err_msg=ctx)
            pair.check_oracle(row, r["obs"], r["dones"], ctx)
            rows.append(row)
            if pair.buf.step == 0:
                pair.after_update(ctx)
        assert rows == [t % BR.BUF_T + 1 for t in range(FL.STEPS)]
        a = np.random.default_rng(6).integers(0, 25, (FL.N_ENVS, N))
        pair.detach_and_step(a, FL.EP)
    finally:
        pair.close()


BLOCK_CASES = BR.block_cases()


@pytest.mark.parametrize("dyn,N,label,meta,ksel,layout,kernel", BLOCK_CASES,
                         ids=["%s%d-%s" % (c[0][:2], c[1], c[2]) for c in BLOCK_CASES])
def test_gpu_buffer_rows_workgroup_kernels(dyn, N, label, meta, ksel, layout, kernel):
    """B(DYN, 64, ., .) and B(DYN, 0, false | true, true): 2 envs, episode_length 3, buffer length 2, 8 steps
    (auto-resets at steps 2 and 5: row 1 and the carry row 2), every third agent of env 0 on its final goal
    after warmup and after the first auto-reset. The reference is the plain env (pinned at these sizes by
    test_gpu_large_n_matches_oracle) and runner_insert of its outputs and dones; the run must hold all three
    mask states."""
    inj = BR.block_injections(meta)
    acts = BR.block_actions(N)
    pair = BR.Pair(meta, BR.B_ENVS, ksel, kernel, BR.B_BUF_T, True, layout)
    try:
        pair.warmup(FL.EP)
        all_dones, resets = [], []
        for t in range(BR.B_STEPS):
            if t in BR.B_INJECT_AT:
                pair.inject(0, *inj[BR.B_INJECT_AT.index(t)])
            ctx = "%s step %d" % (label, t)
            row, dones = pair.step(acts[t], FL.EP, ctx)
            assert row == t % BR.B_BUF_T + 1
            if t in BR.B_INJECT_AT:   # injected agents arrived, the others did not: done agents in a live env
                assert BR.arrived_only(dones[0]), (ctx, dones[0])
            all_dones.append(dones)
            if pair.plain.t_reset.cpu().numpy().any():
                resets.append(t)
            if pair.buf.step == 0:
                pair.after_update(ctx)
        assert resets == [BR.B_EPISODE - 1, 2 * BR.B_EPISODE - 1], resets
        assert BR.reset_rows(resets, BR.B_BUF_T) == [1, BR.B_BUF_T]
        states = BR.mask_states(all_dones)
        assert all(states.values()), {k: len(v) for k, v in states.items()}
        pair.detach_and_step(acts[BR.B_STEPS], FL.EP)
    finally:
        pair.close()


# ---- the ring rebuilt under a selected index ---------------------------------------------------------
CHAIN = {"wave": (4, None, "rollout_kernel<0, 64, 0>"),
         "team": (8, None, "rollout_team_kernel<0, 8, 4, false>"),
         "block": (4, dict(workgroup_per_env=1), "rollout_block_kernel<0, 0, true, false>")}


@pytest.mark.parametrize("family", sorted(CHAIN))
def test_gpu_ring_rebuilt_under_selected_index(family):
    """The configurations and stair sequence of test_gpu_separation_chain_unbounded with the ring bound and an
    index selected throughout: three rounds of [0, 4, 8, 12, 16, 12, 8, 4, 8] change the separation 26 times
    (27 if episode 0's differs from the table's). The record holds 8 shifts (KSEP); change 9 allocates the
    per-env overflow rows s.sepx (16 per env), change 25 reallocates them (lsm_host.hip's sep_check), each
    time setting params_dirty with ring index 0 selected by warmup's reset, and every ring entry must then
    carry the new pointer: the steps that follow read the shifts through ring indices 1..3. Then the value
    table is uploaded again with the ring bound (new table pointers). Buffer rows bit-equal to the plain env's
    outputs after every call."""
    from golden_replay import tables_for
    N, ksel, kernel = CHAIN[family]
    meta = dict(dynamics_type="double_integrator", num_agents=N, num_landmarks=2, world_size=4, episode_length=5,
                num_env_steps=5 * 20, n_rollout_threads=1, use_safety_filter=True, use_masking=True,
                num_internal_step=1, seed=1, env_seed=1, separation_distance_curriculum=True)
    n = 3
    pair = BR.Pair(meta, n, ksel, kernel, 5, tables=tables_for(meta))
    seq = [0, 4, 8, 12, 16, 12, 8, 4, 8] * 3
    assert sum(a != b for a, b in zip(seq, seq[1:])) == 26   # >= 25: allocated, then reallocated
    rng = np.random.default_rng(3)
    try:
        for k, ep in enumerate(seq + [12]):
            if k == len(seq):   # a new HjDataHandle under the bound ring, ring index 3 still selected
                pair.plain._upload_value_table()
                pair.ringed._upload_value_table()
            pair.warmup(ep)
            for t in range(3):
                a = rng.integers(0, 25, (n, N))
                row, _ = pair.step(a, ep, "reset %d (ep %d) step %d" % (k, ep, t))
                assert row == t + 1
    finally:
        pair.close()


# ---- the ring ABI itself -----------------------------------------------------------------------------
def test_gpu_ring_abi_strides_counts_offsets_and_refusals():
    """lsm_bind_output_ring / lsm_select_ring as include/lsm_rollout.h states them, on every ring-able slot
    (DONE, INFO, STATE and COLLISION_FORCE included), strides 64 bytes above the output, counts 2..4, offsets
    0, -1 and +1: each slot's output lands at base + (i + off) * stride when that is a row of its ring, else
    in the plain tensor; padding and every other row keep their bytes; ring_len = max(count - off); the
    refusals' return codes and texts; unbinding under an index that falls out of range, and index -1, write
    the plain tensors only."""
    import torch
    from lsm import capi
    n, N = 5, 3
    meta = FL.spec_meta(FL.DI, N)
    plain = BR.make_env(meta, n, collision_forces=True)
    env = BR.make_env(meta, n, collision_forces=True)
    lib, h = env.lib, env.h
    own = {capi.OUT_OBS: "t_obs", capi.OUT_NODE_OBS: "t_node", capi.OUT_ADJ: "t_adj", capi.OUT_REWARD: "t_rew",
           capi.OUT_DONE: "t_done", capi.OUT_INFO: "t_info", capi.OUT_STATE: "t_state",
           capi.OUT_COLLISION_FORCE: "t_cforce"}
    # slot: (count, offset); STATE alone gives ring_len = max(count - offset) = 5
    plan = {capi.OUT_OBS: (3, 0), capi.OUT_NODE_OBS: (2, -1), capi.OUT_ADJ: (4, 1), capi.OUT_REWARD: (3, -1),
            capi.OUT_DONE: (2, 1), capi.OUT_INFO: (4, 0), capi.OUT_STATE: (4, -1), capi.OUT_COLLISION_FORCE: (3, 1)}
    ring_len = max(c - o for c, o in plan.values())
    assert ring_len == 5 and sorted(c - o for c, o in plan.values())[-2] == 4
    assert {c for c, _ in plan.values()} == {2, 3, 4} and {o for _, o in plan.values()} == {0, -1, 1}
    PAD = 64

    def error():
        return lib.lsm_last_error(h).decode()

    def bind(slot, base, stride, count, off):
        return lib.lsm_bind_output_ring(h, slot, C.c_void_p(base) if base else None, stride, count, off)

    try:
        assert env.kernel_name == plain.kernel_name == "rollout_kernel<0, 64, 3>"
        rings, nbytes = {}, {}
        for slot, (count, off) in plan.items():
            nbytes[slot] = int(lib.lsm_output_bytes(h, slot))
            t = getattr(env, own[slot])
            assert nbytes[slot] == t.numel() * t.element_size() > 0
            rings[slot] = torch.full((count, nbytes[slot] + PAD), BR.SENTINEL, dtype=torch.uint8, device="cuda:0")
            assert bind(slot, rings[slot].data_ptr(), nbytes[slot] + PAD, count, off) == 0, error()
        plain.reset(FL.EP)
        env.reset(FL.EP)   # no index selected yet: plain bindings
        for slot in plan:
            assert (BR.raw(rings[slot]) == BR.SENTINEL).all()
            np.testing.assert_array_equal(BR.raw(getattr(env, own[slot])), BR.raw(getattr(plain, own[slot])))

        # refusals leave the bindings as they are
        assert bind(capi.OUT_OBS, rings[capi.OUT_OBS].data_ptr(), nbytes[capi.OUT_OBS] - 4, 3, 0) != 0
        assert error() == "ring stride smaller than slot 0's output"
        for slot in (capi.OUT_RESET_FLAG, capi.OUT_EP_INFO, capi.OUT_EDGES, capi.OUT_DEBUG_STAMPS, capi.OUT_DEPARTED,
                     capi.OUT_ADJ_NNZ):
            assert bind(slot, rings[capi.OUT_OBS].data_ptr(), 1 << 20, 2, 0) != 0
            assert error() == "slot %d cannot be ring-bound" % slot
        for slot in (-1, capi.NUM_OUT):
            assert bind(slot, rings[capi.OUT_OBS].data_ptr(), 1 << 20, 2, 0) != 0
            assert error() == "bad output slot"
        assert lib.lsm_select_ring(h, -2) != 0
        assert error() == "ring index -2 outside [-1, %d)" % ring_len
        assert lib.lsm_select_ring(h, ring_len) != 0
        assert error() == "ring index %d outside [-1, %d)" % (ring_len, ring_len)
        assert lib.lsm_select_ring(h, ring_len - 1) == 0, error()

        g = torch.Generator(device="cuda:0").manual_seed(4)

        def step(index, ctx):
            """One step of both envs; index None: no ring row may be written."""
            before = {s: BR.raw(r) for s, r in rings.items()}
            own_before = {s: BR.raw(getattr(env, own[s])) for s in plan}
            a = torch.randint(0, 25, (n, N), generator=g, device="cuda:0", dtype=torch.int32)
            plain.step(a, FL.EP)
            env.step(a, FL.EP)
            for slot, (count, off) in plan.items():
                want, now = BR.raw(getattr(plain, own[slot])).reshape(-1), BR.raw(rings[slot])
                j = -1 if index is None or slot not in bound else index + off
                expect = before[slot].copy()
                if 0 <= j < count:
                    expect[j, :nbytes[slot]] = want
                    np.testing.assert_array_equal(BR.raw(getattr(env, own[slot])), own_before[slot],
                                                  err_msg="%s slot %d: the plain tensor was written too" % (ctx, slot))
                else:
                    np.testing.assert_array_equal(BR.raw(getattr(env, own[slot])).reshape(-1), want,
                                                  err_msg="%s slot %d: fall-back to the plain pointer" % (ctx, slot))
                np.testing.assert_array_equal(now, expect, err_msg="%s slot %d ring" % (ctx, slot))
                assert (now[:, nbytes[slot]:] == BR.SENTINEL).all(), (ctx, slot)

        bound = set(plan)
        for i in range(ring_len):
            assert lib.lsm_select_ring(h, i) == 0, error()
            step(i, "ring index %d" % i)
        for slot, (count, off) in plan.items():   # the rows no index reaches still hold the sentinel
            reached = {i + off for i in range(ring_len)}
            for j in range(count):
                if j not in reached:
                    assert (BR.raw(rings[slot][j]) == BR.SENTINEL).all(), (slot, j)

        # unbinding the slot that set ring_len under an index that is then out of range: plain bindings
        assert lib.lsm_select_ring(h, ring_len - 1) == 0, error()
        assert bind(capi.OUT_STATE, None, 0, 0, 0) == 0, error()
        bound.discard(capi.OUT_STATE)
        step(None, "after unbinding STATE under index %d" % (ring_len - 1))
        assert lib.lsm_select_ring(h, ring_len - 1) != 0
        assert error() == "ring index %d outside [-1, %d)" % (ring_len - 1, ring_len - 1)
        assert lib.lsm_select_ring(h, ring_len - 2) == 0, error()
        step(ring_len - 2, "ring index %d, STATE unbound" % (ring_len - 2))
        assert lib.lsm_select_ring(h, -1) == 0, error()
        step(None, "index -1 with rings bound")
    finally:
        plain.close()
        env.close()
