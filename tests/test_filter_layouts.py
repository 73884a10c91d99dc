"""CPU proofs that the injected layouts and the oracle runs of tests/filter_layouts.py can tell a wrong
filter from a right one, from the oracle alone (pair values, OracleEnv._filter_one), for every (dynamics,
agent count) that tests/test_gpu_filter_choice.py runs; and that the cases of that file name every
one-wave and team kernel the library has."""
import os
import re

import numpy as np
import pytest

import filter_layouts as FL
import hj_bounds_model as M

SPEC_IDS = ["%s%d" % (d[:2], n) for d, n in FL.SPECS]


def test_variants_name_every_wave_and_team_row():
    """The parity cases' expected kernel names are exactly the W and T rows of csrc/lsm_kernels.h plus
    the generic workgroup kernel B(DYN, 0, true, false), as the host's kernel table spells them."""
    path = os.path.join(M.ROOT, "layered-safe-marl_amd", "csrc", "lsm_kernels.h")
    rows = set()
    for line in open(path):
        if not re.match(r"#define LSM_KERNELS_\d", line):
            continue
        for d, lpe, nt in re.findall(r"\bW\((\d), (\d+), (\d+)\)", line):
            rows.add("rollout_kernel<%s, %s, %s>" % (d, lpe, nt))
        for d, nt, g, rext in re.findall(r"\bT\((\d), (\d+), (\d+), (true|false)\)", line):
            rows.add("rollout_team_kernel<%s, %s, %s, %s>" % (d, nt, g, rext))
    assert len(rows) == 22, sorted(rows)
    rows |= {"rollout_block_kernel<0, 0, true, false>", "rollout_block_kernel<1, 0, true, false>"}
    named = {v[5] for v in FL.kernel_variants()}
    assert named == rows, sorted(rows ^ named)


def test_spike_depth_defaults_and_gate_table():
    """make_table's depth: the default reproduces the spike table bit for bit, and the gate table
    differs from it in the "last" node alone, lower by a further GATE_DEPTH - SPIKE_DEPTH."""
    for dyn in (FL.DI, FL.AT):
        base = M.make_table(dyn, "spike", FL.SHAPES[dyn], bshift=FL.BSHIFT)
        same = M.make_table(dyn, "spike", FL.SHAPES[dyn], bshift=FL.BSHIFT, depth={})
        assert base.values_hj.tobytes() == same.values_hj.tobytes()
        assert base.grads_hj.tobytes() == same.grads_hj.tobytes()
        gate = FL.table(dyn, "spike")
        diff = np.argwhere(gate.values_hj != base.values_hj)
        node = M.spike_nodes(dyn, FL.SHAPES[dyn], FL.BSHIFT)["last"][0]
        assert [tuple(x) for x in diff] == [node]
        assert gate.values_hj[node] == np.float32(base.values_hj[node] + M.SPIKE_DEPTH - np.float32(FL.GATE_DEPTH))


@pytest.mark.parametrize("kind", FL.KINDS)
@pytest.mark.parametrize("dyn,N", FL.SPECS, ids=SPEC_IDS)
def test_layout_proofs(dyn, N, kind):
    """Every layout's proof of power on envs just reset (injections asserts each): spike pairs and gate
    (spike table), twins, loner, the pair-less ego within range."""
    ora = FL.oracle_vec(FL.spec_meta(dyn, N), FL.table(dyn, kind))
    ora.reset(FL.EP)
    inj, facts = FL.injections(dyn, kind, ora.envs)
    a, b = FL.twin_indices(N)
    s = inj[FL.ENV_TWINS]["states"]
    assert a < b < N and s[a].tobytes() == s[b].tobytes()
    if kind == "spike":
        names = [inj[k]["name"] for k in FL.ENV_SPIKES if k in inj]
        assert len(names) == len(FL.ENV_SPIKES) and len(set(names)) == (3 if dyn == FL.DI else 5), names
        g = facts["gate"]
        print("%s N=%d gate: nearest agent at %.2f (range %.3f), argmin value %.3f" % (
            dyn, N, g["dist"], ora.envs[0].coordination_range, g["value"]))
    print("%s N=%d %s: twins (%d, %d) at offset k = %d" % (dyn, N, kind, a, b, facts["twins_k"]))


@pytest.mark.parametrize("kind", FL.KINDS)
@pytest.mark.parametrize("dyn,N", FL.SPECS, ids=SPEC_IDS)
def test_oracle_run_conditions(dyn, N, kind):
    """The conditions on the parity run's inputs (check_run): two auto-resets, each filter status at least
    once, filtered and unfiltered egos in every episode, argmin != nearest for at least 1 % of the active
    egos on the rough table, no control within 1e-6 of the 'filtered' threshold, and each layout's
    expected outcome in the step after its injection."""
    figs = FL.check_run(FL.oracle_run(dyn, N, kind), kind)
    print("%s N=%d %s: statuses %s; argmin != nearest for %d of %d active egos (%.1f %%); %d ties; twins k %s" % (
        dyn, N, kind, figs["count"], figs["off_nearest"], figs["active"], 100 * figs["share"], figs["ties"],
        figs["twins_k"]))
