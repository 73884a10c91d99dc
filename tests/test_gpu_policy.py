"""GPU tests of the fused actor / critic heads (csrc/lsm_policy.hip through include/lsm_policy.h and
lsm/policy.py): the kernel against tests/policy_model.py's float64 model within the tolerance measured per
case and output tensor (4 * e32 + 4 * 2^-23 * s), the sampler's discrete outputs exact on decidable rows, on
tests/policy_cases.py's cases -- a few rows each, around the 64-row tile's edges -- with canaries behind
every output; then the public surface and three closed collect steps on a 4-env, N = 3 env."""
import numpy as np
import pytest

import device_policy_cases as dp
import policy_abi as pa
import policy_cases as pc
import policy_model as pm
from lsm import capi, policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("M", pc.SHAPE_M)
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_shapes(lib, kind, M):
    pc.check(lib, pc.shape_case(kind, M), DEV)


@pytest.mark.parametrize("name", sorted(pc.OPTIONS))
def test_options(lib, name):
    pc.check(lib, pc.option_case(name), DEV)


@pytest.mark.parametrize("name", sorted(pc.PLAN_OPTIONS))
def test_plan_cases(lib, name):
    """The forward's largest tile (in 256, hidden 128: the bytes its LDS limit is raised to) and its narrowest
    input row (in0 + in1 = 1, with x0 or x1 null)."""
    pc.check(lib, pc.plan_case(name), DEV)


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_masked_state_does_not_leak(lib, kind):
    pc.masks_checks(lib, kind, DEV)


def test_available_actions(lib):
    pc.avail_checks(lib, DEV)


def test_stratified_sampler(lib):
    pc.stratified_checks(lib, DEV)


def test_same_call_twice_and_null_outputs(lib):
    pc.twice_and_null_checks(lib, DEV)


def test_bad_uniforms(lib):
    pc.bad_u_checks(lib, DEV)


def test_refusals_write_nothing_on_the_device(lib):
    """The argument checks are the host entry point's (tests/test_policy_capi.py runs every one); here two of
    them with device pointers: nothing is launched, no output byte changes."""
    case = pc.shape_case("actor", 65)
    pa.run(lib, case.cfg, case.blob, case.inp, DEV, expect_rc=1, bad_init=3, alias=("rnn_out", "rnn_states", 0))
    pa.run(lib, case.cfg, case.blob, case.inp, DEV, expect_rc=1, bad_init=3, over=dict(M=-1))
    inp = {k: (v[:0] if v is not None else None) for k, v in case.inp.items()}
    got, bad = pa.run(lib, case.cfg, case.blob, inp, DEV)
    assert got == {} and bad == 0


@pytest.mark.parametrize("which", ["actor 257", "critic 65", "option recurrent_N 2", "option tanh", "option hidden5 A5",
                                   "option A64 in 250"])
def test_device_matches_host(lib, which):
    """The kernel and lsm_host_head_forward run one per-row text; exp / tanh / rsqrt and the FMA contraction
    differ, so each stays within the case's bound of the float64 model (pc.check), and the two are
    compared with that bound, not for bit equality. Decidable rows give the same action."""
    kind, rest = which.split(" ", 1)
    case = pc.option_case(rest) if kind == "option" else pc.shape_case(kind, int(rest))
    host = pc.check(lib, case, None)
    dev = pc.check(lib, case, DEV)
    for mode in host:
        for k, (tol, _) in case.tol.items():
            if k not in host[mode]:
                continue
            sel = case.fin if k == "logits" else slice(None)
            if k == "log_probs":
                same = host[mode]["actions_i32"] == dev[mode]["actions_i32"]
                sel = same
            err = float(np.abs(dev[mode][k][sel].astype(np.float64) - host[mode][k][sel]).max())
            print("head device vs host %s %s: %.3e (tol %.3e)" % (which, k, err, tol))
            assert err <= tol, (which, k, err, tol)
        if case.cfg.kind == "actor":
            dec = case.dec_mode if mode else case.dec_sample
            np.testing.assert_array_equal(dev[mode]["actions_i32"][dec], host[mode]["actions_i32"][dec])


def _check_head(cfg, sd, inp, got, what):
    """One head's device outputs (torch tensors) against the float64 model fed the same inputs. The
    actions follow tests/policy_cases.py's rule (exact on decidable rows, adjacent or tied otherwise).
    Returns (undecidable rows, rows) of an actor, (0, 0) of a critic."""
    M = inp["x1"].shape[0]
    w64, w32 = pm.model64(cfg, sd, inp), pm.model32(cfg, sd, inp)
    np_ = lambda t: t.detach().cpu().numpy()
    pm.assert_close(np_(got["features"]), w64["features"], *pm.tensor_bound(w64["features"], w32["features"]),
                    what + " features")
    if cfg.recurrent_N:
        pm.assert_close(np_(got["rnn_states"]), w64["rnn_out"], *pm.tensor_bound(w64["rnn_out"], w32["rnn_out"]),
                        what + " rnn_states")
    if cfg.kind == "critic":
        pm.assert_close(np_(got["values"]).reshape(M), w64["values"], *pm.tensor_bound(w64["values"], w32["values"]),
                        what + " values")
        return 0, 0
    act = np_(got["actions_env"]).reshape(M)
    np.testing.assert_array_equal(np_(got["actions"]).reshape(M), act.astype(np.float32))
    assert act.dtype == np.int32 and ((act >= 0) & (act < cfg.num_actions)).all()
    lb = pm.tensor_bound(w64["logits"], w32["logits"])[0]
    undecidable = pc.assert_actions(w64, act, lb, inp.get("u"), what)
    pm.assert_close(np_(got["action_log_probs"]).reshape(M), w64["logp"][np.arange(M), act],
                    *pm.tensor_bound(w64["logp"], w32["logp"]), what + " log_probs")
    return undecidable, M


def _bounded(tally):
    """At most 5 % of a test's actor rows may be undecidable (tests/policy_cases.py's condition, over all
    of the test's rounds: one round has 12 rows)."""
    bad, rows = sum(t[0] for t in tally), sum(t[1] for t in tally)
    assert rows > 0 and bad <= pc.MAX_UNDECIDABLE * rows, (bad, rows)


def test_public_surface(lib):
    """PolicyHead.forward and DevicePolicy.get_actions on a 4-env, N = 3 env after one step (no buffer: the
    env's own tensors), sampled and deterministic; load() changes the output; non-CUDA tensors, a 'node'
    critic and mismatched widths are refused; check=True raises on a bad uniform and clears the word."""
    import torch
    env = dp.env()
    env.reset(0)
    env.step(torch.full((4, 3), 7, dtype=torch.int32, device=DEV), 0)
    pol, (ah, asd), (ch, csd) = dp.heads(env)
    n, N, M = 4, 3, 12
    rng = np.random.default_rng(3)
    st = torch.as_tensor((0.5 * rng.normal(size=(M, 1, 64))).astype(np.float32), device=DEV)
    stc = torch.as_tensor((0.5 * rng.normal(size=(M, 1, 64))).astype(np.float32), device=DEV)
    masks = torch.ones((M, 1), device=DEV)
    masks[5] = 0
    tally = []
    for det in (False, True):
        g = torch.Generator(device=DEV).manual_seed(17)
        out = pol.get_actions(env, st, stc, masks, deterministic=det, generator=g)
        assert out["actions_env"].dtype == torch.int32 and tuple(out["actions_env"].shape) == (n, N)
        assert out["actions_env"].is_contiguous() and tuple(out["values"].shape) == (M, 1)
        assert tuple(out["actions"].shape) == tuple(out["action_log_probs"].shape) == (M, 1)
        assert tuple(out["rnn_states"].shape) == tuple(out["rnn_states_critic"].shape) == (M, 1, 64)
        u = None if det else torch.rand(M, generator=torch.Generator(device=DEV).manual_seed(17), device=DEV).cpu().numpy()
        a_feat = env.gnn_features(pol.actor_encoder).cpu().numpy()
        c_feat = env.gnn_features(pol.critic_encoder).cpu().numpy()
        obs = env.t_obs.view(M, -1).cpu().numpy()
        share = np.repeat(env.t_obs.view(n, 1, -1).cpu().numpy(), N, axis=1).reshape(M, -1)
        a_in = dict(x0=obs, x1=a_feat, states=st.cpu().numpy(), masks=masks.cpu().numpy(), u=u, avail=None)
        c_in = dict(x0=share, x1=c_feat, states=stc.cpu().numpy(), masks=masks.cpu().numpy(), u=None, avail=None)
        tally.append(_check_head(ah, asd, a_in, dict(features=pol.last_actor["features"], rnn_states=out["rnn_states"],
                                                     actions_env=out["actions_env"], actions=out["actions"],
                                                     action_log_probs=out["action_log_probs"]),
                                 "get_actions actor det=%s" % det))
        _check_head(ch, csd, c_in, dict(features=pol.last_critic["features"],
                                        rnn_states=out["rnn_states_critic"], values=out["values"]),
                    "get_actions critic det=%s" % det)
        env.step_async(out["actions_env"], 0)      # the zero-op fast path takes them as they are
        env.step_wait()
        env.check_actions()
    _bounded(tally)
    # load(): new weights, new values
    before = pol.get_actions(env, st, stc, masks, deterministic=True)["values"].clone()
    pol.critic_head.load(pm.random_head_weights(ch, 99))
    after = pol.get_actions(env, st, stc, masks, deterministic=True)["values"]
    assert float((after - before).abs().max()) > 1e-3
    # refusals of the Python layer
    head = pol.actor_head
    x1 = torch.zeros((M, 16), device=DEV)
    with pytest.raises(policy.PolicyError):
        head.forward(env.t_obs.cpu(), x1, st, masks)
    with pytest.raises(policy.PolicyError):
        head.forward(env.t_obs, x1.cpu(), st, masks)
    with pytest.raises(policy.PolicyError):
        head.forward(env.t_obs, x1, None, None)
    with pytest.raises(policy.PolicyError):
        head.forward(env.t_obs, x1, st[:5], masks)
    with pytest.raises(policy.PolicyError):
        policy.PolicyHead(ah, head.weights, "cpu")
    with pytest.raises(policy.PolicyError, match="node"):
        policy.DevicePolicy(pol.actor_encoder, pol.actor_head, pol.actor_encoder, pol.critic_head)
    with pytest.raises(policy.PolicyError, match="in1"):
        narrow = policy.HeadConfig(kind="actor", in0=env.OBS, in1=8, num_actions=25)
        policy.DevicePolicy(pol.actor_encoder,
                            policy.PolicyHead(narrow, np.zeros(policy.head_weights_floats(narrow), np.float32), DEV),
                            pol.critic_encoder, pol.critic_head)
    bad_u = torch.full((M,), 1.5, device=DEV)
    with pytest.raises(policy.PolicyError):
        head.forward(env.t_obs, x1, st, masks, u=bad_u, check=True)
    assert int(head.bad.item()) == 0
    got = head.forward(env.t_obs, x1, st, masks, u=bad_u)
    assert int(got["actions_env"].max()) < 25
    env.close()


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_closed_loop_with_the_replay_buffer(lib, layout):
    """Three rounds of get_actions -> insert_step on a DeviceGraphBuffer with policy_rows: the step takes
    the int32 actions as they are (check_actions passes), the buffer's rows hold the returned tensors
    (the states zeroed where the step's dones are set), and each round's outputs match the float64 model
    fed the same encoder output, row t's obs / share_obs, states and masks, and the same uniforms."""
    import torch
    from lsm.buffer import DeviceGraphBuffer
    env = dp.env(layout)
    pol, (ah, asd), (ch, csd) = dp.heads(env, seed=1)
    n, N, M = 4, 3, 12
    buf = DeviceGraphBuffer(env, episode_length=4, policy_rows=dict(hidden_size=64, recurrent_N=1, act_dim=1,
                                                                    num_actions=None))
    buf.warmup(0)
    g = torch.Generator(device=DEV).manual_seed(5)
    g2 = torch.Generator(device=DEV).manual_seed(5)
    np_ = lambda t: t.detach().cpu().numpy()
    tally = []
    for t in range(3):
        assert buf.step == t
        out = pol.get_actions(env, buf.rnn_states[t], buf.rnn_states_critic[t], buf.masks[t], generator=g, buffer=buf)
        u = np_(torch.rand(M, generator=g2, device=DEV))
        kept = {k: v.clone() for k, v in out.items()}
        feats = (pol.last_actor["features"].clone(), pol.last_critic["features"].clone())
        # the model's inputs: row t as the buffer holds it, and the encoders' outputs on it
        row_mask = None if buf.adj_mask is None else buf.adj_mask[t]
        a_feat = np_(pol.actor_encoder.forward_step(buf.node_obs[t], buf.adj[t], row_mask, N, env.agent_id))
        c_feat = np_(pol.critic_encoder.forward_step(buf.node_obs[t], buf.adj[t], row_mask, N, env.agent_id))
        a_in = dict(x0=np_(buf.obs[t]).reshape(M, -1), x1=a_feat, states=np_(buf.rnn_states[t]).reshape(M, 1, 64),
                    masks=np_(buf.masks[t]).reshape(M, 1), u=u, avail=None)
        c_in = dict(x0=np_(buf.share_obs[t]).reshape(M, -1), x1=c_feat,
                    states=np_(buf.rnn_states_critic[t]).reshape(M, 1, 64), masks=np_(buf.masks[t]).reshape(M, 1),
                    u=None, avail=None)
        assert np.abs(a_in["x0"]).max() > 0 and c_in["x0"].shape[1] == N * env.OBS
        tally.append(_check_head(ah, asd, a_in, dict(features=feats[0], rnn_states=kept["rnn_states"],
                                                     actions_env=kept["actions_env"], actions=kept["actions"],
                                                     action_log_probs=kept["action_log_probs"]),
                                 "closed loop %s t%d actor" % (layout, t)))
        _check_head(ch, csd, c_in, dict(features=feats[1], rnn_states=kept["rnn_states_critic"], values=kept["values"]),
                    "closed loop %s t%d critic" % (layout, t))
        dones, _ = buf.insert_step(out["actions_env"], 0, value_preds=out["values"],
                                   policy={k: out[k] for k in ("actions", "action_log_probs", "rnn_states",
                                                               "rnn_states_critic")})
        np.testing.assert_array_equal(np_(buf.actions[t]).reshape(M), np_(kept["actions"]).reshape(M))
        np.testing.assert_array_equal(np_(buf.actions[t]).reshape(n, N), np_(kept["actions_env"]).astype(np.float32))
        np.testing.assert_array_equal(np_(buf.action_log_probs[t]).reshape(M), np_(kept["action_log_probs"]).reshape(M))
        np.testing.assert_array_equal(np_(buf.value_preds[t]).reshape(M), np_(kept["values"]).reshape(M))
        done = np_(dones).reshape(M).astype(bool)
        for row, key in ((buf.rnn_states, "rnn_states"), (buf.rnn_states_critic, "rnn_states_critic")):
            want = np.where(done[:, None, None], np.float32(0), np_(kept[key]))
            np.testing.assert_array_equal(np_(row[t + 1]).reshape(M, 1, 64), want)
        assert np.abs(np_(kept["rnn_states"])).max() > 0
    _bounded(tally)
    env.check_actions()
    buf.detach()
    env.close()
