"""GPU tests of the PPO loss (csrc/lsm_loss.hip through include/lsm_loss.h, lsm/loss.py and lsm/policy.py): the
kernels against tests/loss_model.py's float64 model within the tolerance measured per case and output tensor
(4 * e32 + 4 * 2^-23 * s) on tests/loss_cases.py's cases -- a few hundred rows around the 256-row group's edges --
with canaries around every output, the scratch and the normaliser's state, and twice bit-equal; the
log-probability recomputed bit for bit from lsm_head_evaluate's logits; then the public surface:
DevicePolicy.ppo_loss on a collected minibatch with unchanged weights (ratio 1), with a DeviceValueNorm through
compute_returns and advantages."""
import numpy as np
import pytest

import device_policy_cases as dp
import evaluate_cases as ec
import evaluate_model as em
import loss_cases as lc
import loss_model as lm
import policy_model as pm
from lsm import capi, policy
from lsm.loss import DeviceValueNorm, LossConfig, LossError, PPOLoss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("M", lc.MS)
def test_rows(lib, M):
    lc.check(lib, lc.shape_case(M, 25), DEV)


def test_more_groups_than_one_stage(lib):
    """258 groups: the one-workgroup launches stage the groups' sums twice; the sums are the host's, which adds
    them in one plain loop, to the bit (the normaliser's state)."""
    case = lc.shape_case(lc.MANY, 5)
    dev, host = lc.check(lib, case, DEV), lc.check(lib, case)
    np.testing.assert_array_equal(dev["vn_state"].view(np.int32), host["vn_state"].view(np.int32))
    np.testing.assert_array_equal(dev["dvalues"].view(np.int32), host["dvalues"].view(np.int32))


@pytest.mark.parametrize("A", lc.AS)
def test_actions(lib, A):
    lc.check(lib, lc.shape_case(65, A), DEV)


@pytest.mark.parametrize("flag", lc.FLAGS + ("all",))
def test_flags_off(lib, flag):
    flags = {f: False for f in lc.FLAGS} if flag == "all" else {flag: False}
    lc.check(lib, lc.shape_case(65 if flag == "all" else 257, 25, **flags), DEV)


@pytest.mark.parametrize("half", ["actor", "critic"])
def test_one_half_alone(lib, half):
    full = lc.shape_case(257, 25)
    both, _, _ = lc.run(lib, full.cfg, full.inp, DEV)
    got = lc.check(lib, lc.Case("only " + half, full.cfg, full.inp, actor=half == "actor", critic=half == "critic"), DEV)
    for k in got:
        if k == "stats":
            keep = [0, 2, 3] if half == "actor" else [1]
            np.testing.assert_array_equal(got[k][keep].view(np.int32), both[k][keep].view(np.int32))
        elif k != "vn_state":
            np.testing.assert_array_equal(got[k].view(np.int32), both[k].view(np.int32), err_msg=k)


def test_available_actions_and_active_masks(lib):
    case = lc.shape_case(65, 25, avail="some")
    got = lc.check(lib, case, DEV)
    assert (got["dlogits"][2] == 0).all() and got["imp_weights"][3] == 0
    got = lc.check(lib, lc.shape_case(65, 25, active="zero"), DEV)
    assert np.isnan(got["stats"][:3]).all() and np.isnan(got["dlogits"]).all() and (got["dvalues"] == 0).any()
    lc.check(lib, lc.shape_case(65, 25, active="ones"), DEV)


def test_bad_actions_and_named_branch_points(lib):
    case = lc.shape_case(257, 25)
    clean, bad, _ = lc.run(lib, case.cfg, case.inp, DEV)
    assert bad == 0
    acts = case.inp["actions"].copy()
    acts[[3, 130, 200, 256]] = [2.5, -1.0, 25.0, np.nan]
    bcase = lc.Case("bad actions", case.cfg, dict(case.inp, actions=acts))
    assert bcase.w64["bad"].sum() == 4
    got = lc.check(lib, bcase, DEV)       # asserts *bad == 1
    keep = ~bcase.w64["bad"]
    np.testing.assert_array_equal(got["imp_weights"][keep].view(np.int32), clean["imp_weights"][keep].view(np.int32))
    cfg, inp, names = lc.named_inputs()
    inp = {k: (np.asarray(v, np.float32) if v is not None else None) for k, v in inp.items()}
    got = lc.check(lib, lc.Case("named", cfg, inp), DEV)
    assert got["dvalues"][names.index("e < -delta")] == 0 and got["dvalues"][names.index("d = +c")] != 0


def test_device_matches_host_and_the_sums_are_the_same_bits(lib):
    """The kernels and lsm_host_ppo_loss run one per-row text; expf / logf differ between the two, so each stays
    within the case's bound of the float64 model and the two are compared with that bound. The normaliser,
    whose float64 sums run in one order on both and whose float32 formulas have no transcendental but sqrtf,
    is bit-equal."""
    case = lc.shape_case(2 * lc.GROUP + 1, 25)
    host, dev = lc.check(lib, case), lc.check(lib, case, DEV)
    for k, (tol, _) in case.tol.items():
        err = float(np.abs(dev[k].astype(np.float64) - host[k]).max())
        print("loss device vs host %s: %.3e (tol %.3e)" % (k, err, tol))
        assert err <= tol, (k, err, tol)
    for k in ("vn_state", "denorm"):
        np.testing.assert_array_equal(dev[k].view(np.int32), host[k].view(np.int32), err_msg=k)


def test_refusals_write_nothing_on_the_device_and_empty_is_legal(lib):
    """The argument checks are the host entry point's (tests/test_loss_capi.py runs every one); here three of
    them with device pointers: nothing is launched, no output byte changes. And the empty minibatch."""
    case = lc.shape_case(65, 25)
    run = lambda **kw: lc.run(lib, case.cfg, case.inp, DEV, expect_rc=1, bad_init=3, **kw)
    run(alias=("dlogits", "logits", 0))
    run(over=dict(scratch=None))
    run(over=dict(M=-1))
    inp = {k: (v[:0] if isinstance(v, np.ndarray) and k != "vn_state" else v) for k, v in case.inp.items()}
    got, bad, _ = lc.run(lib, case.cfg, inp, DEV, M=0)
    assert got == {} and bad == 0


@pytest.mark.parametrize("which", ["plain", "avail"])
def test_the_log_probability_is_lsm_head_evaluates_bit_for_bit(lib, which):
    """old_log_probs := the log_probs lsm_head_evaluate writes, logits := the logits it writes: the loss
    recomputes the same bits, so the ratio is exactly 1.0 on every row with a finite log-probability, and so is
    its mean."""
    ecase = ec.shape_case("actor", 65, 10) if which == "plain" else ec.avail_case("some")
    ev, bad = ec.run(lib, ecase.cfg, ecase.blob, ecase.inp, ecase.C, ecase.T, DEV, outputs=("log_probs", "logits"))
    assert bad == 0
    R, A = ecase.R, ecase.cfg.num_actions
    rng = np.random.default_rng(3)
    cfg = LossConfig(num_actions=A)
    inp = {"logits": ev["logits"], "actions": ecase.inp["actions"], "avail": ecase.inp.get("avail"),
           "old": ev["log_probs"], "adv": rng.normal(size=R).astype(np.float32),
           "active": np.ones(R, np.float32), "values": rng.normal(size=R).astype(np.float32),
           "vpreds": rng.normal(size=R).astype(np.float32), "returns": rng.normal(size=R).astype(np.float32),
           "vn_state": lc.VN_STATE.copy()}
    got, bad, _ = lc.run(lib, cfg, inp, DEV)
    finite = ev["log_probs"] > -1e37
    assert bad == 0 and finite.sum() >= R - 1 and (which == "plain") == bool(finite.all())
    assert (got["imp_weights"][finite] == 1.0).all()
    if finite.all():
        assert got["stats"][3] == 1.0
    want = -(inp["adv"].astype(np.float64)[finite]).sum() / R
    if finite.all():   # policy_loss is then -mean(adv), rounded once
        assert got["stats"][0] == np.float32(want)


def test_evaluate_with_logits_returns_the_same_bytes(lib):
    """PolicyHead.evaluate(..., logits=True) against the default call on the same inputs: every output the
    default call returns is bit-equal, the default dict has no logits, and the logits are the model's."""
    import torch
    case = ec.avail_case("some")
    head = policy.PolicyHead(case.cfg, case.blob, DEV)
    t = lambda k: None if case.inp.get(k) is None else torch.as_tensor(case.inp[k], device=DEV)
    args = (t("x0"), t("x1"), t("states"), t("masks"), case.T)
    kw = dict(actions=t("actions"), available_actions=t("avail"), active_masks=t("active"))
    plain = head.evaluate(*args, **kw)
    assert "logits" not in plain
    keys = ("action_log_probs", "entropy", "dist_entropy", "features", "rnn_states")
    first = {k: plain[k].clone() for k in keys}
    kept = head.evaluate(*args, logits=True, **kw)
    assert set(kept) - {"logits"} == set(plain) | {"_logits"} and tuple(kept["logits"].shape) == (case.R, 25)
    for k in keys:
        assert torch.equal(kept[k].view(torch.int32), first[k].view(torch.int32)), k
    again = head.evaluate(*args, **kw)
    assert "logits" not in again
    for k in keys:
        assert torch.equal(again[k].view(torch.int32), first[k].view(torch.int32)), k
    lg = kept["logits"].cpu().numpy()
    pm.assert_close(lg, case.w64["logits"], *case.tol["logits"], "evaluate(logits=True) logits", sel=case.fin)
    assert (lg[~case.fin] == np.float32(pm.FLT_MIN)).all()
    critic = ec.shape_case("critic", 65, 10)
    chead = policy.PolicyHead(critic.cfg, critic.blob, DEV)
    tc = lambda k: None if critic.inp.get(k) is None else torch.as_tensor(critic.inp[k], device=DEV)
    assert "logits" not in chead.evaluate(tc("x0"), tc("x1"), tc("states"), tc("masks"), critic.T, logits=True)


# ---- the public surface ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_ppo_loss_closes_the_loop_on_a_collected_minibatch(lib, layout):
    """Six collect steps with get_actions(buffer=...), compute_returns and advantages with a DeviceValueNorm,
    one recurrent_generator minibatch with data_chunk_length 3, DevicePolicy.ppo_loss with unchanged weights:
    the ratio is 1 on every row (up to the two forward kernels' rounding), policy_loss is -sum w adv / sum w,
    the four scalars and both gradients are the float64 model's on the same tensors, and so is the
    DeviceValueNorm's state."""
    import torch
    env = dp.env(layout)
    pol, (ah, asd), _ = dp.heads(env, seed=1)
    buf = dp.collect(env, pol, 6)
    vn = DeviceValueNorm(DEV)
    vn.load_state_dict({"running_mean": torch.tensor([0.1]), "running_mean_sq": torch.tensor([0.75]),
                        "debiasing_term": torch.tensor(0.5)})
    np.testing.assert_allclose(vn.denorm.cpu().numpy(), [np.sqrt(1.5 - 0.04), 0.2], rtol=1e-6)
    sd = vn.state_dict()
    assert tuple(sd["running_mean"].shape) == (1,) and sd["debiasing_term"].dim() == 0
    next_value = pol.get_values(env, buf.rnn_states_critic[-1], buf.masks[-1], buffer=buf, row=-1)
    buf.compute_returns(next_value, vn, gamma=0.99, gae_lambda=0.95)
    adv, _ = buf.advantages(vn)
    mb = next(iter(buf.recurrent_generator(adv, 1, 3)))
    R = int(mb["obs"].shape[0])
    assert R == 72 and tuple(mb["rnn_states"].shape) == (24, 1, 64)
    loss = PPOLoss(LossConfig(num_actions=25), DEV)
    state0 = vn.state.cpu().numpy().copy()
    out = pol.ppo_loss(mb, loss, vn, data_chunk_length=3)
    for k in ("policy_loss", "value_loss", "dist_entropy", "ratio"):
        assert out[k].dim() == 0 and out[k].is_cuda, k
    assert tuple(out["dlogits"].shape) == (R, 25) and tuple(out["dvalues"].shape) == tuple(out["imp_weights"].shape) == (R, 1)
    np_ = lambda x: x.detach().cpu().numpy()
    inp = {"logits": np_(out["logits"]), "actions": np_(mb["actions"]).reshape(R), "avail": None,
           "old": np_(mb["action_log_probs"]).reshape(R), "adv": np_(mb["advantages"]).reshape(R),
           "active": np_(mb["active_masks"]).reshape(R), "values": np_(out["values"]).reshape(R),
           "vpreds": np_(mb["value_preds"]).reshape(R), "returns": np_(mb["returns"]).reshape(R), "vn_state": state0}
    case = lc.Case("closed loop " + layout, loss.cfg, inp)
    assert not lc.near_branch(loss.cfg, case.w64).any()
    got = {"dlogits": np_(out["dlogits"]), "dvalues": np_(out["dvalues"]).reshape(R),
           "imp_weights": np_(out["imp_weights"]).reshape(R), "stats": np_(out["stats"]), "vn_state": np_(vn.state),
           "denorm": np_(vn.denorm)}
    for k, (tol, e32) in case.tol.items():
        lc.assert_close(got[k], case.w64[k], tol, e32, "closed loop %s %s" % (layout, k))
    for i, k in enumerate(("policy_loss", "value_loss", "dist_entropy", "ratio")):
        assert float(out[k]) == float(got["stats"][i])
    # ratio 1: the stored log-probability is the one-step kernel's, the new one the sequence kernel's; each is
    # within the minibatch's bound tl of the float64 model (tests/test_gpu_evaluate.py), so |ratio - 1| <=
    # expm1(2 tl) and one rounding
    a_feat = np_(pol.actor_encoder.forward(mb["node_obs"], mb["adj"], mb["agent_id"]))
    a_in = dict(x0=np_(mb["obs"]), x1=a_feat, states=np_(mb["rnn_states"]), masks=np_(mb["masks"]),
                actions=inp["actions"], avail=None, active=np_(mb["active_masks"]))
    a64, a32 = em.model64(ah, asd, a_in, 24, 3), em.model32(ah, asd, a_in, 24, 3)
    tl, _ = pm.tensor_bound(a64["log_probs"], a32["log_probs"])
    rb = float(np.expm1(2 * tl)) + lc.EPS
    dev1 = float(np.abs(got["imp_weights"].astype(np.float64) - 1).max())
    print("closed loop %s: max |ratio - 1| %.3e (bound %.3e)" % (layout, dev1, rb))
    assert dev1 <= rb and abs(float(out["ratio"]) - 1) <= rb
    w, a = inp["active"].astype(np.float64), inp["adv"].astype(np.float64)
    want = -(w * a).sum() / w.sum()
    pbound = rb * (w * np.abs(a)).sum() / w.sum() + 4 * lc.EPS * np.abs(a).max()
    print("closed loop %s: policy_loss %.7f, -sum w adv / sum w %.7f (bound %.3e)" % (layout, float(out["policy_loss"]), want, pbound))
    assert abs(float(out["policy_loss"]) - want) <= pbound
    # the learner's side: the seeds fit torch.autograd.backward, the critic half alone leaves the actor's alone
    lg = out["logits"].clone().requires_grad_(True)
    torch.autograd.backward([lg * 1.0], [out["dlogits"]])
    assert torch.equal(lg.grad, out["dlogits"])
    first = {k: out[k].clone() for k in ("dvalues", "stats")}
    vn.state.copy_(torch.as_tensor(state0, device=DEV))
    half = pol.ppo_loss(mb, loss, vn, data_chunk_length=3, update_actor=False)
    assert "dlogits" not in half and "policy_loss" not in half
    assert torch.equal(half["dvalues"].view(torch.int32), first["dvalues"].view(torch.int32))
    assert torch.equal(half["value_loss"].view(torch.int32), first["stats"][1].view(torch.int32))
    with pytest.raises(LossError, match="value_norm"):
        pol.ppo_loss(mb, loss, None, data_chunk_length=3)
    with pytest.raises(policy.PolicyError, match="actions"):
        pol.ppo_loss(mb, PPOLoss(LossConfig(num_actions=5), DEV), vn, data_chunk_length=3)
    buf.detach()
    env.close()
