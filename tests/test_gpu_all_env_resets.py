"""Every env's every reset against the oracle, through every step-kernel family, in both streams.

The oracle draws random numbers only while it resets (tests/test_reset_truth.py), so what env k
shows after its r-th reset depends only on (seed + 1000 k, r, ep): the truth of all envs comes from
oracles that do nothing but reset (oracle_pool.run_all_resets), and the device runs 20 steps (54 at
N = 3 and N = 5) of random actions with episodes of 6 (reset_cases.CONFIGS); double-integrator envs that
share a workgroup or a wave with others are driven all-done early, so that resetting and
non-resetting envs sit side by side. At every launch, every env whose reset flag
is set is compared with its own next reset index: obs, node_obs, adjacency (nonzero pattern exact)
and env.state(). Nothing is sampled. Under "philox" the truth is the same oracle fed from
lsm_host_philox_uniforms(seed + 1000 k, r), so the counter word "reset index" is compared at every r.

By-product: the families of one config run the same seeds and actions. The first family's outputs
of every step stay on the device and every other family is compared with them at every step, for
all envs (dones, reset flags and adjacency pattern exact; float32 outputs, states and rewards
within twice the parity tests' bounds: each family is held to those against the oracle, so twice
is the triangle inequality). A disagreement is settled by replaying that env's episode (at most 6
steps) through the oracle from its reset index (reset_cases.replay, itself checked on the CPU in
tests/test_reset_truth.py); the family outside the project's tolerance fails. The "first family" is
whichever case of a config and stream ran first in this session (the module global _FIRST): a run
that selects one case, or whose first family failed before its end, makes no such comparison.

Tolerances (tests/test_gpu_parity.py): pattern / dones exact, float32 outputs 1e-5, states 1e-9,
rewards rtol 1e-6 + atol 1e-5. The comparisons run on the device, with one host read per step.
"""
import numpy as np
import pytest

import test_gpu_parity
from reset_cases import EP, EPISODE_LENGTH, F32_ATOL, GPU_CASES, REW_ATOL, REW_RTOL, SEED, STATE_ATOL, actions, \
    arrive_all_state, case, n_resets, replay, reset_schedule, within_project_tolerance
from test_gpu_parity import _gpu_env

pytestmark = pytest.mark.gpu

assert (F32_ATOL, STATE_ATOL) == (test_gpu_parity.F32_ATOL, test_gpu_parity.STATE_ATOL)   # the project's bounds
MAX_REPLAYS = 4
MIN_EARLY_RESETS = 8

DEVICE = "cuda:0"
_TRUTH = {}   # (config, rng) -> the oracle's resets: host arrays + device tensors
_FIRST = {}   # (config, rng) -> (family, per-step outputs of the first family that ran, on the device)


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    yield
    import torch
    _TRUTH.clear()
    _FIRST.clear()
    torch.cuda.empty_cache()


def _truth(name, rng):
    import torch
    from oracle_pool import run_all_resets
    key = (name, rng)
    if key not in _TRUTH:
        cfg = case(name, rng)
        host = run_all_resets(cfg["meta"], SEED, cfg["n_envs"], EP, n_resets(cfg), rng=rng)
        dev = {k: torch.as_tensor(host[k], device=DEVICE) for k in ("obs", "node", "adj", "state")}
        _TRUTH[key] = (host, dev)
    return _TRUTH[key]


def _amax(x):
    """Largest |x| per env ([n, ...] -> [n]); NaN stays NaN."""
    return x.abs().flatten(1).amax(dim=1)


def _snapshot(env, rew, dones):
    return dict(obs=env.t_obs.clone(), node=env.t_node.clone(), adj=env.reference_adj().clone(),
                state=env.state().clone(), rew=rew.reshape(rew.shape[0], -1).clone(), dones=dones.clone(),
                reset=env.t_reset.clone())


def _disagree(a, b):
    """Envs whose two families' outputs of one step differ by more than twice the project's bounds."""
    import torch
    rb = 2 * (REW_ATOL + REW_RTOL * torch.maximum(a["rew"].abs(), b["rew"].abs()))
    return ((a["dones"] != b["dones"]).any(dim=1) | (a["reset"] != b["reset"])
            | ((a["adj"] != 0) != (b["adj"] != 0)).flatten(1).any(dim=1)
            | ~(_amax(a["obs"] - b["obs"]) <= 2 * F32_ATOL) | ~(_amax(a["node"] - b["node"]) <= 2 * F32_ATOL)
            | ~(_amax(a["adj"] - b["adj"]) <= 2 * F32_ATOL) | ~(_amax(a["state"] - b["state"]) <= 2 * STATE_ATOL)
            | ~((a["rew"] - b["rew"]).abs() <= rb).all(dim=1))


def _read(named):
    """The named device tensors as float64 host arrays, in one host read."""
    import torch
    flat = torch.cat([v.double().flatten() for v in named.values()]).cpu().numpy()
    out, i = {}, 0
    for k, v in named.items():
        out[k] = flat[i:i + v.numel()]
        i += v.numel()
    return out


@pytest.mark.parametrize("name,fam,rng", GPU_CASES, ids=["%s-%s-%s" % c for c in GPU_CASES])
def test_gpu_every_env_reset_matches_oracle(name, fam, rng):
    """One family of one config (reset_cases.CONFIGS) in one stream: see the module docstring."""
    import torch
    cfg = case(name, rng)
    f = cfg["families"][fam]
    meta = cfg["meta"]
    n, N, T, R = cfg["n_envs"], meta["num_agents"], cfg["steps"], n_resets(cfg)
    host, tr = _truth(name, rng)
    env = _gpu_env(meta, n_envs=n, seed=SEED, adj_layout=f["layout"], kernel_select=f["ksel"] or None, rng=rng,
                   return_numpy=False, build_infos=False)
    assert env.kernel_name == f["kernel"], env.kernel_name
    if f["stage"] is not None:
        assert env.lib.lsm_test_set_mt_stage(env.h, f["stage"]) == 0
    dev = env.device
    acts_h = actions(name, rng)
    acts = torch.as_tensor(acts_h, device=dev)
    ar = torch.arange(n, device=dev)
    count = torch.zeros(n, dtype=torch.int64, device=dev)    # each env's own count of set reset flags
    count_h = np.zeros(n, dtype=np.int64)
    last_reset = np.full(n, -1)                                 # the step of each env's latest reset
    # the reset flags every step must show: the common episode ends, and the injected envs' own
    sched = reset_schedule(cfg)
    expect = np.zeros((T, n), dtype=bool)
    expect[sched[None]] = True
    for k, steps in sched.items():
        if k is not None:
            expect[:, k] = False
            expect[steps, k] = True
    first = _FIRST.get((name, rng)) if len(cfg["families"]) > 1 else None
    keep = [] if (len(cfg["families"]) > 1 and first is None) else None
    dev_max = np.zeros(4)     # largest deviation from the oracle at a compared reset: obs, node, adj, state
    diff_max = np.zeros(5)    # largest deviation from the first family: obs, node, adj, state, reward
    compared = replays = early_resets = 0
    notes = []

    def compare_resets(m):
        """Envs with m set against the truth of their reset index count[k]: the numbers to read
        (envs outside the tolerance, envs past the truth's last index, envs compared, the largest
        deviation in obs, node, adj, state) and the mask of the envs outside the tolerance."""
        r = count.clamp(max=R - 1)
        adj, want_adj = env.reference_adj(), tr["adj"][ar, r][:, None]   # one matrix for a reset's N egos
        d = torch.stack([_amax(env.t_obs - tr["obs"][ar, r]), _amax(env.t_node - tr["node"][ar, r]),
                         _amax(adj - want_adj), _amax(env.state() - tr["state"][ar, r])])
        pat = ((adj != 0) != (want_adj != 0)).flatten(1).any(dim=1)
        tol = torch.tensor([F32_ATOL, F32_ATOL, F32_ATOL, STATE_ATOL], dtype=torch.float64, device=dev)[:, None]
        bad = (pat | ~(d.double() <= tol).all(dim=0)) & m
        dm = torch.where(m[None], d.double(), torch.zeros((), dtype=torch.float64, device=dev)).amax(dim=1)
        return dict(outside=bad.sum(), past_truth=(m & (count >= R)).sum(), compared=m.sum(), dev=dm), bad

    def settle(h, bad, ctx):
        nonlocal compared
        assert h["past_truth"][0] == 0, "%s: an env reset more often than the truth holds (%d indices)" % (ctx, R)
        if h["outside"][0] != 0:
            ks = bad.nonzero().flatten().cpu().numpy()
            pytest.fail("%s: %d of %d resetting envs differ from the oracle's reset, first envs %s at reset "
                        "indices %s; largest deviations obs %.3g node %.3g adj %.3g state %.3g"
                        % (ctx, int(h["outside"][0]), int(h["compared"][0]), ks[:8].tolist(),
                           count_h[ks[:8]].tolist(), *h["dev"]))
        compared += int(h["compared"][0])
        np.maximum(dev_max, h["dev"], out=dev_max)

    env.reset(EP)
    named, bad = compare_resets(torch.ones(n, dtype=torch.bool, device=dev))
    settle(_read(named), bad, "%s/%s/%s first reset" % (name, fam, rng))
    count += 1
    count_h += 1
    for t in range(T):
        ctx = "%s/%s/%s step %d" % (name, fam, rng, t)
        obs, aid, node, adj, rew, dones, (info, reset, epinfo) = env.step(acts[t], EP)
        m = reset.bool()
        named, bad = compare_resets(m)
        named["flag_is_all_done"] = (m == dones.all(dim=1)).all()   # the worker resets iff every agent is done
        snap = dis = None
        if keep is not None or first is not None:
            snap = _snapshot(env, rew, dones)
        if first is not None:
            base = first[1][t]
            dis = _disagree(snap, base)
            named["disagreeing"] = dis.sum()
            named["diff"] = torch.stack([_amax(snap[q] - base[q]).amax().double()
                                         for q in ("obs", "node", "adj", "state", "rew")])
        named["reset"] = m
        h = _read(named)                                            # the step's one host read
        m_h = h["reset"] != 0
        assert h["flag_is_all_done"][0] == 1, ctx + ": a reset flag is set without every agent done, or the reverse"
        wrong = np.nonzero(m_h != expect[t])[0]
        assert wrong.size == 0, "%s: envs %s reset, or did not, against the schedule" % (ctx, wrong[:8].tolist())
        settle(h, bad, ctx)
        if first is not None:
            np.fmax(diff_max, h["diff"], out=diff_max)
            if h["disagreeing"][0] != 0:   # rare: a disagreement between two families is settled by the oracle
                for k in dis.nonzero().flatten().cpu().numpy().tolist():
                    replays += 1
                    assert replays <= MAX_REPLAYS, "%s: more than %d oracle replays: %s" % (ctx, MAX_REPLAYS, notes)
                    r_k = int(count_h[k]) - 1
                    want = replay(name, rng, k, r_k, int(last_reset[k]), t, acts_h)
                    ok_me, why_me = within_project_tolerance({q: v[k].cpu().numpy() for q, v in snap.items()}, want)
                    ok_first, why_first = within_project_tolerance({q: v[k].cpu().numpy() for q, v in base.items()},
                                                                   want)
                    notes.append("env %d step %d (reset index %d%s): %s %s, %s %s" % (
                        k, t, r_k, ", resetting" if m_h[k] else "", fam, "ok" if ok_me else "OUT", first[0],
                        "ok" if ok_first else "OUT"))
                    assert ok_me, "%s env %d: %s is outside the project's tolerance of the oracle's replay " \
                                  "(%s agrees: %s)\n%s" % (ctx, k, fam, first[0], ok_first, why_me)
                    assert ok_first, "%s env %d: the first family %s is outside the project's tolerance of " \
                                     "the oracle's replay, %s is inside\n%s" % (ctx, k, first[0], fam, why_first)
        if keep is not None:
            keep.append(snap)
        if (t + 1) % EPISODE_LENGTH:   # resets off the common episode boundary
            early_resets += int(m_h.sum())
        last_reset[m_h] = t
        count += m
        count_h += m_h
        for k in cfg["early"].get(t, ()):   # env k all-done at the next step: an off-phase reset
            st, reached = arrive_all_state(host["lm"][k, count_h[k] - 1], N, meta["num_landmarks"])
            env.set_agent_state(k, st, reached)
    env.check_actions()
    assert compared == int(count_h.sum()) == n + int(expect.sum())   # every env, every reset
    if cfg["early"]:
        assert early_resets >= MIN_EARLY_RESETS, early_resets
    if keep is not None:
        _FIRST[(name, rng)] = (fam, keep)
    print("reset_parity %s/%s/%s kernel=%s envs=%d resets_compared=%d early_resets=%d max_dev obs=%.3g node=%.3g "
          "adj=%.3g state=%.3g" % (name, fam, rng, env.kernel_name, n, compared, early_resets, *dev_max))
    if first is not None:
        print("family_diff %s/%s/%s vs %s env_steps=%d replays=%d max_diff obs=%.3g node=%.3g adj=%.3g state=%.3g "
              "rew=%.3g %s" % (name, fam, rng, first[0], n * T, replays, *diff_max, notes))
    env.close()
