"""GPU tests of the heads' sequence form (csrc/lsm_evaluate.hip through include/lsm_evaluate.h and
lsm/policy.py): the kernel against tests/evaluate_model.py's float64 model within the tolerance measured per
case and output tensor (4 * e32 + 4 * 2^-23 * s) on tests/evaluate_cases.py's cases -- a few chunks of a few
steps each, around the 64-chunk tile's edges -- with canaries around every output; then the public surface:
evaluate_actions reproducing a collected minibatch's stored log-probabilities and values (ratio 1 before any
update), and get_values / act as the two halves of get_actions."""
import numpy as np
import pytest

import device_policy_cases as dp
import evaluate_cases as ec
import evaluate_model as em
import policy_model as pm
from lsm import capi, policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "C%d-T%d" % s)
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_shapes(lib, kind, shape):
    ec.check(lib, ec.shape_case(kind, *shape), DEV)


@pytest.mark.parametrize("name", sorted(ec.OPTIONS))
def test_options(lib, name):
    ec.check(lib, ec.option_case(name), DEV)


@pytest.mark.parametrize("name", sorted(ec.PLAN_OPTIONS))
def test_plan_cases(lib, name):
    """One case per size limit and width class (evaluate_cases.PLAN_OPTIONS, the limits found through
    lsm_head_plan): hidden 128, the widest inputs, the largest recurrent hidden (a tile of exactly 163840
    bytes), layer_N 3 and 4, widths around 64 and 128, A above both widths and in0 + in1 = 1; past an LDS limit
    the call is refused and writes nothing."""
    ec.plan_checks(lib, name, DEV)


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_masked_state_does_not_leak(lib, kind):
    ec.masks_checks(lib, kind, DEV)


def test_available_actions_and_active_masks(lib):
    ec.avail_checks(lib, DEV)


def test_nan_features_are_read_as_zero(lib):
    ec.nan_checks(lib, DEV)


def test_bad_actions(lib):
    ec.bad_action_checks(lib, DEV)


def test_single_step_agrees_with_the_forward(lib):
    ec.t1_checks(lib, DEV)


def test_same_call_twice_and_null_outputs(lib):
    ec.twice_and_null_checks(lib, DEV)


def test_refusals_write_nothing_on_the_device(lib):
    """The argument checks are the host entry point's (tests/test_evaluate_capi.py runs every one); here three
    of them with device pointers: nothing is launched, no output byte changes. And the empty minibatch."""
    case = ec.shape_case("actor", 65, 10)
    run = lambda **kw: ec.run(lib, case.cfg, case.blob, case.inp, case.C, case.T, DEV, expect_rc=1, bad_init=3, **kw)
    run(alias=("rnn_out", "rnn_states", 0))
    run(over=dict(T=0))
    run(over=dict(scratch=None))
    inp = {k: (v[:0] if v is not None else None) for k, v in case.inp.items()}
    got, bad = ec.run(lib, case.cfg, case.blob, inp, 0, 3, DEV)
    assert got == {} and bad == 0


@pytest.mark.parametrize("which", ["actor 65 10", "critic 129 2", "option recurrent_N 2"])
def test_device_matches_host(lib, which):
    """The kernel and lsm_host_head_evaluate run one per-chunk text; exp / tanh / rsqrt and the FMA contraction
    differ, so each stays within the case's bound of the float64 model (ec.check), and the two are compared
    with that bound, not for bit equality."""
    kind, rest = which.split(" ", 1)
    case = ec.option_case(rest) if kind == "option" else ec.shape_case(kind, *map(int, rest.split()))
    host = ec.check(lib, case, None)
    dev = ec.check(lib, case, DEV)
    for k, (tol, _) in case.tol.items():
        sel = case.fin if k == "logits" else slice(None)
        err = float(np.abs(dev[k][sel].astype(np.float64) - host[k][sel]).max())
        print("evaluate device vs host %s %s: %.3e (tol %.3e)" % (which, k, err, tol))
        assert err <= tol, (which, k, err, tol)
    if case.cfg.kind == "actor":
        assert abs(float(dev["dist_entropy"][0]) - float(host["dist_entropy"][0])) <= case.tol["entropy"][0]


# ---- the public surface ---------------------------------------------------------------------------------------

def _reproduces(pol, heads, mb, L, what):
    """evaluate_actions(mb, L) against the minibatch's stored log-probabilities and values, within twice the
    tolerance of the minibatch as a case (the two models on the same inputs and encoder outputs)."""
    (ah, asd), (ch, csd) = heads
    np_ = lambda t: t.detach().cpu().numpy()
    R = int(mb["obs"].shape[0])
    T = L or 1
    Cn = R // T
    out = pol.evaluate_actions(mb, L)
    assert tuple(out["values"].shape) == tuple(out["action_log_probs"].shape) == (R, 1)
    assert tuple(out["entropy"].shape) == (R,) and out["dist_entropy"].dim() == 0
    a_feat = np_(pol.actor_encoder.forward(mb["node_obs"], mb["adj"], mb["agent_id"]))
    c_feat = np_(pol.critic_encoder.forward(mb["node_obs"], mb["adj"], mb["agent_id"]))
    rec = ah.recurrent_N > 0
    a_in = dict(x0=np_(mb["obs"]), x1=a_feat, states=np_(mb["rnn_states"]) if rec else None,
                masks=np_(mb["masks"]) if rec else None, actions=np_(mb["actions"]).reshape(R), avail=None,
                active=np_(mb["active_masks"]))
    c_in = dict(x0=np_(mb["share_obs"]), x1=c_feat, states=np_(mb["rnn_states_critic"]) if rec else None,
                masks=np_(mb["masks"]) if rec else None, actions=None, avail=None, active=None)
    assert c_in["x0"].shape[1] == ch.in0 and np.abs(a_in["x0"]).max() > 0
    a64, a32 = em.model64(ah, asd, a_in, Cn, T), em.model32(ah, asd, a_in, Cn, T)
    c64, c32 = em.model64(ch, csd, c_in, Cn, T), em.model32(ch, csd, c_in, Cn, T)
    assert max(a64["amp"].max(), c64["amp"].max()) <= ec.MAX_AMP
    tl, el = pm.tensor_bound(a64["log_probs"], a32["log_probs"])
    tv, ev = pm.tensor_bound(c64["values"], c32["values"])
    te, ee = pm.tensor_bound(a64["entropy"], a32["entropy"])
    logp, val = np_(out["action_log_probs"]).reshape(R), np_(out["values"]).reshape(R)
    pm.assert_close(logp, a64["log_probs"], tl, el, what + " log_probs vs model")
    pm.assert_close(val, c64["values"], tv, ev, what + " values vs model")
    pm.assert_close(np_(out["entropy"]), a64["entropy"], te, ee, what + " entropy vs model")
    de = float(out["dist_entropy"])
    assert abs(de - a64["dist_entropy"]) <= te + ec.EPS * abs(a64["dist_entropy"]), (de, a64["dist_entropy"])
    old_logp, old_val = np_(mb["action_log_probs"]).reshape(R), np_(mb["value_preds"]).reshape(R)
    for name, new, old, tol in (("log_probs", logp, old_logp, tl), ("values", val, old_val, tv)):
        err = float(np.abs(new.astype(np.float64) - old).max())
        print("%s %s vs the stored rows: %.3e (2 tol %.3e) bit-exact %s ratio max %.9f"
              % (what, name, err, 2 * tol, bool((new.view(np.int32) == old.view(np.int32)).all()),
                 float(np.exp(np.abs(logp.astype(np.float64) - old_logp)).max())))
        assert err <= 2 * tol, (what, name, err, tol)


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_evaluate_actions_reproduces_a_collected_recurrent_minibatch(lib, layout):
    """Six collect steps, recurrent_generator with data_chunk_length 3 (it divides T, so no chunk crosses an
    agent's series) and one minibatch of 24 chunks: with unchanged weights evaluate_actions gives the stored
    old_action_log_probs and value_preds back -- importance ratio 1 before any update."""
    import torch
    env = dp.env(layout)
    pol, ah, ch = dp.heads(env, seed=1)
    buf = dp.collect(env, pol, 6)
    adv = torch.zeros(6 * 4 * 3, dtype=torch.float32, device=DEV)
    batches = list(buf.recurrent_generator(adv, 1, 3))
    assert len(batches) == 1 and tuple(batches[0]["rnn_states"].shape) == (24, 1, 64)
    _reproduces(pol, (ah, ch), batches[0], 3, "closed loop %s recurrent" % layout)
    # GMPERunner.compute: the critic on the last row. buf.step has wrapped to 0, so compute() names row -1;
    # after_update() carries that row to row 0, where the default reads the same bytes
    assert buf.step == 0
    last = pol.get_values(env, buf.rnn_states_critic[-1], buf.masks[-1], buffer=buf, row=-1).clone()
    first = pol.get_values(env, buf.rnn_states_critic[0], buf.masks[0], buffer=buf).clone()
    assert float((last - first).abs().max()) > 1e-4
    buf.after_update()
    again = pol.get_values(env, buf.rnn_states_critic[0], buf.masks[0], buffer=buf)
    assert torch.equal(again.view(torch.int32), last.view(torch.int32))
    buf.detach()
    env.close()


def test_evaluate_actions_reproduces_a_collected_feed_forward_minibatch(lib):
    """The same through feed_forward_generator with non-recurrent heads: the learner gathers its own policy
    rows with the yielded indices."""
    import torch
    env = dp.env()
    pol, ah, ch = dp.heads(env, recurrent_N=0, seed=2)
    T = 6
    buf = dp.collect(env, pol, T)
    adv = torch.zeros(T * 4 * 3, dtype=torch.float32, device=DEV)
    mb = dict(next(iter(buf.feed_forward_generator(adv, num_mini_batch=1))))
    idx = mb["indices"]
    mb["actions"] = buf.actions[:T].reshape(T * 12, 1)[idx]
    mb["action_log_probs"] = buf.action_log_probs[:T].reshape(T * 12, 1)[idx]
    _reproduces(pol, (ah, ch), mb, None, "closed loop feed-forward")
    # and what the Python layer refuses
    with pytest.raises(policy.PolicyError, match="actions"):
        pol.evaluate_actions({k: v for k, v in mb.items() if k != "actions"})
    with pytest.raises(policy.PolicyError, match="adj"):
        pol.evaluate_actions(dict(mb, adj=None))
    with pytest.raises(policy.PolicyError, match="chunks of T"):
        pol.evaluate_actions(mb, 5)
    bad = dict(mb, actions=torch.full_like(mb["actions"], 25.0))
    with pytest.raises(policy.PolicyError, match="stored action"):
        pol.evaluate_actions(bad, check=True)
    assert int(pol.actor_head.bad.item()) == 0
    buf.detach()
    env.close()


@pytest.mark.parametrize("with_buffer", [False, True])
def test_get_values_and_act_are_the_halves_of_get_actions(lib, with_buffer):
    """On the same env state get_values equals get_actions()['values'] and act(deterministic=True) equals
    get_actions(deterministic=True)'s actions, actions_env and rnn_states, bit for bit (the same kernels on
    the same inputs); sampled, act draws what get_actions draws from the same generator state."""
    import torch
    from lsm.buffer import DeviceGraphBuffer
    env = dp.env()
    pol, _, _ = dp.heads(env, seed=3)
    M = 12
    buf = None
    if with_buffer:
        buf = DeviceGraphBuffer(env, episode_length=4, policy_rows=dict(hidden_size=64, recurrent_N=1, act_dim=1,
                                                                        num_actions=None))
        buf.warmup(0)
    else:
        env.reset(0)
        env.step(torch.full((4, 3), 7, dtype=torch.int32, device=DEV), 0)
    rng = np.random.default_rng(3)
    st = torch.as_tensor((0.5 * rng.normal(size=(M, 1, 64))).astype(np.float32), device=DEV)
    stc = torch.as_tensor((0.5 * rng.normal(size=(M, 1, 64))).astype(np.float32), device=DEV)
    masks = torch.ones((M, 1), device=DEV)
    masks[5] = 0
    for det in (True, False):
        gen = lambda: None if det else torch.Generator(device=DEV).manual_seed(9)
        full = {k: v.clone() for k, v in pol.get_actions(env, st, stc, masks, deterministic=det, generator=gen(),
                                                         buffer=buf).items()}
        values = pol.get_values(env, stc, masks, buffer=buf).clone()
        half = pol.act(env, st, masks, deterministic=det, generator=gen(), buffer=buf)
        assert tuple(values.shape) == (M, 1) and set(half) == {"actions", "actions_env", "rnn_states"}
        assert torch.equal(values.view(torch.int32), full["values"].view(torch.int32))
        assert half["actions_env"].dtype == torch.int32 and tuple(half["actions_env"].shape) == (4, 3)
        for k in half:
            assert torch.equal(half[k], full[k]), k
    assert float(full["values"].abs().max()) > 0 and int(full["actions_env"].max()) > 0
    if buf is not None:
        buf.detach()
    env.close()
