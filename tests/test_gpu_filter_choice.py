"""The safety filter's choice of a deconflicting agent and its control in every one-wave kernel
(rollout_kernel<DYN, LPE, NT>: the select chain of compile-time N, the NT = 0 loop), every team kernel
(rollout_team_kernel<DYN, NT, G, REXT>: the 8-lane butterflies, the gathered gradient, the status slot
from phase A to phase B) and the small-N workgroup kernel, against the CPU oracle on the hard tables
of tests/hj_bounds_model.py with the layouts of tests/filter_layouts.py injected: spike pairs whose
argmin is not the nearest agent, twins that tie exactly, egos with no in-grid pair, one partner or
none, every third agent done, and an argmin that only the coordination-range gate keeps unfiltered.
Envs in these states share one agent wave of the team kernel (envs 4..7 at 4 and 8 envs per
workgroup). The oracle's run and the conditions on it (filter_layouts.check_run: each filter status
occurs, each layout's proof holds in the step after its injection) are computed once per (spec,
table kind, reward case) and shared by the variants; every case asserts the kernel it ran."""
import numpy as np
import pytest

import filter_layouts as FL

pytestmark = pytest.mark.gpu

STATE_ATOL = 1e-9
F32_ATOL = 1e-5

VARIANTS = FL.kernel_variants()
CASES = [v + (kind,) for v in VARIANTS for kind in (("rough",) if v[2] else FL.KINDS)]


def _gpu_env(meta, vt, ksel):
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    args = EnvArgs.from_namespace(type("A", (), meta)())
    args.seed = meta["seed"]
    return GpuGraphVecEnv(args, num_envs=FL.N_ENVS, device="cuda:0", value_table=vt,
                          ttr_table=FL.ttr(meta["dynamics_type"]), kernel_select=ksel, build_infos=False)


def _info_col(name):
    from lsm import capi
    return capi.INFO_FIELDS.index(name)


@pytest.mark.parametrize("dyn,N,rext,label,ksel,kernel,kind", CASES,
                         ids=["%s%d-%s%s-%s" % (c[0][:2], c[1], c[3], "-rext" if c[2] else "", c[6]) for c in CASES])
def test_gpu_filter_choice_matches_oracle(dyn, N, rext, label, ksel, kernel, kind):
    """15 envs, episode_length 6, 14 steps (two auto-resets), the layouts injected after the initial
    reset and after the first auto-reset. Every step against the oracle at the project's tolerances:
    dones, reset flags, adjacency pattern, deconflicting agent and 'Safety filtered' exact; obs / node
    / adj 1e-5; rewards rtol 1e-6, atol 1e-5, individual_reward 1e-9; states and min_relative_distance
    1e-9; action_diff (the only float64 view of the filtered control, hence of the gradient) 1e-12."""
    run = FL.oracle_run(dyn, N, kind, rext)
    figs = FL.check_run(run, kind)
    print("%s N=%d %s rext=%d: statuses %s; argmin != nearest for %d of %d active egos (%.1f %%); %d ties; twins k %s"
          % (dyn, N, kind, rext, figs["count"], figs["off_nearest"], figs["active"], 100 * figs["share"],
             figs["ties"], figs["twins_k"]))
    env = _gpu_env(run["meta"], FL.table(dyn, kind), ksel)
    try:
        assert env.kernel_name == kernel, (env.kernel_name, kernel)
        g, o = env.reset(FL.EP), run["reset"]
        np.testing.assert_allclose(g[0], o["obs"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g[2], o["node"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(g[3], o["adj"], rtol=0, atol=F32_ATOL)
        np.testing.assert_allclose(env.state().cpu().numpy(), o["state"], rtol=0, atol=STATE_ATOL)
        c_dec, c_sf, c_ad = _info_col("deconflicting_agent_index"), _info_col("Safety filtered"), _info_col("action_diff")
        c_mr, c_ir = _info_col("min_relative_distance"), _info_col("individual_reward")
        for t, r in enumerate(run["steps"]):
            for k, inj in r["inject"].items():
                env.set_agent_state(k, inj["states"], inj["reached"])
            g = env.step(r["a"], FL.EP)
            ctx = "%s %s step %d" % (label, kind, t)
            info, reset = env.t_info.cpu().numpy(), env.t_reset.cpu().numpy().astype(bool)
            np.testing.assert_array_equal(g[5], r["dones"], err_msg=ctx)
            np.testing.assert_array_equal(reset, r["reset"], err_msg=ctx)
            np.testing.assert_array_equal(g[3] != 0, r["adj"] != 0, err_msg=ctx)
            live = ~r["reset"]   # the oracle env's per-step arrays were re-initialised by its reset
            np.testing.assert_array_equal(info[live][:, :, c_dec].astype(int), r["dec"][live], err_msg=ctx)
            np.testing.assert_array_equal(info[:, :, c_sf].astype(bool), r["filtered_info"], err_msg=ctx)
            np.testing.assert_allclose(info[live][:, :, c_ad], r["action_diff"][live], rtol=0, atol=1e-12, err_msg=ctx)
            np.testing.assert_allclose(env.state().cpu().numpy(), r["state"], rtol=0, atol=STATE_ATOL, err_msg=ctx)
            np.testing.assert_allclose(info[:, :, c_mr], r["min_rel"], rtol=0, atol=1e-9, err_msg=ctx)
            np.testing.assert_allclose(g[0], r["obs"], rtol=0, atol=F32_ATOL, err_msg=ctx)
            np.testing.assert_allclose(g[2], r["node"], rtol=0, atol=F32_ATOL, err_msg=ctx)
            np.testing.assert_allclose(g[3], r["adj"], rtol=0, atol=F32_ATOL, err_msg=ctx)
            np.testing.assert_allclose(g[4], r["rew"], rtol=1e-6, atol=1e-5, err_msg=ctx)
            np.testing.assert_allclose(info[:, :, c_ir], r["ind_rew"], rtol=1e-9, atol=1e-9, err_msg=ctx)
    finally:
        env.close()
