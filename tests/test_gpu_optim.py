"""GPU tests of the device optimiser (csrc/lsm_optim.hip through include/lsm_optim.h, lsm/optim.py and
lsm/policy.py): lsm_optim_step on tests/optim_cases.py's cases -- bit-equal to tests/optim_model.py's numpy
float32 model and to lsm_host_optim_step, canaries around every segment, the workspace, state and info -- then the
public surface: DeviceAdam over an encoder and a head, its refusals and its state_dict, the modules' state_dict, and
DevicePolicy.ppo_update closing the loop on a collected minibatch in both adjacency layouts."""
import dataclasses
import functools

import numpy as np
import pytest

import device_policy_cases as dp
import gnn_abi as ga
import gnn_cases as gc
import gnn_model as gm
import optim_cases as oc
import optim_model as om
import policy_model as pm
from lsm import capi, gnn, optim, policy
from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H = oc.H


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.fixture(scope="module")
def runner(lib):
    return functools.partial(oc.run, lib, dev=DEV)


# ---- the kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", oc.SIZES)
def test_segment_sizes(runner, n):
    oc.check_size(runner, n)


def test_three_segments_at_odd_offsets(runner):
    oc.check_odd_offsets(runner)


def test_device_equals_host(lib, runner):
    host = functools.partial(oc.run, lib)
    A = oc.group(dataclasses.replace(H, max_grad_norm=0.5, weight_decay=0.01), oc.data(oc.ODD, 81))
    B = oc.group(H, oc.data([oc.CHUNK - 1, 1], 82, 1e-3, 1e-5), goff=1)
    for step in range(2):
        d, h = runner([A, B]), host([A, B])
        for i in range(2):
            oc.same_groups(d[i], h[i], "device against host, step %d, group %d" % (step + 1, i))
        A, B = oc.next_group(A, d[0], oc.grads(oc.ODD, 83)), oc.next_group(B, d[1], oc.grads([oc.CHUNK - 1, 1], 84, 1e-5))


def test_two_groups_in_one_call(runner):
    oc.check_two_groups(runner)


def test_clipping(runner):
    oc.check_clipping(runner)


def test_weight_decay(runner):
    oc.check_weight_decay(runner)


def test_six_steps_with_a_changed_lr(runner):
    oc.check_six_steps(runner)


def test_small_magnitudes(runner):
    oc.check_small_magnitudes(runner)


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_nonfinite_gradient(runner, value):
    oc.check_nonfinite(runner, value)


def test_gradient_of_1e20(runner):
    oc.check_huge_gradient(runner)


def test_twice_and_on_a_second_stream(lib, runner):
    import torch
    oc.check_twice(runner, functools.partial(oc.run, lib, dev=DEV, stream=torch.cuda.Stream(DEV)))


# ---- DeviceAdam -------------------------------------------------------------------------------------------------

HEAD = policy.HeadConfig(kind="critic", in0=5, in1=16, feature_norm=False)
ADAM = optim.AdamConfig(lr=7e-4, max_grad_norm=0.5)
np_ = lambda t: t.detach().cpu().numpy()
bits_of = lambda t: np_(t).view(np.int32 if t.element_size() == 4 else np.int64)


def encoder_inputs():
    """(config without layer norm, node_obs [5, 24, F], dense adj, agent ids, the weight blob) on the host."""
    cfg = dataclasses.replace(gc.DEFAULT, layer_norm=False)
    x, table, bits = gm.random_graphs(5, 24, cfg.F, seed=9, density=0.4, N=5)
    full = ga.sources(table, bits, 5, None)["reference"].full
    return cfg, x, full, gc.ego_ids(5, 24), gm.default_weights(cfg, 9)[1]


def modules(enc_blob=None, head_blob=None):
    """An encoder without layer norm and a head without feature norm, and what runs their backward."""
    import torch
    cfg, x, full, aid, blob = encoder_inputs()
    enc = gnn.GraphEncoder(cfg, blob if enc_blob is None else enc_blob, DEV)
    blob = policy.pack_head_weights(pm.random_head_weights(HEAD, 3), HEAD) if head_blob is None else head_blob
    head = policy.PolicyHead(HEAD, blob, DEV)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    rng = np.random.default_rng(5)
    x, full, aid = t(x), t(full), t(aid)
    dout = t(rng.standard_normal((x.shape[0], cfg.out_dim)).astype(np.float32))
    f = lambda *shape: t(rng.standard_normal(shape).astype(np.float32))
    hx0, hx1, hh, dv = f(6, 5), f(6, 16), f(2, 1, 64), f(6, 1)
    masks = torch.ones(6, 1, device=DEV)

    def backward(embed=True):
        enc.backward(x, full, dout, aid, embed=embed)
        head.backward(hx0, hx1, hh, masks, 3, dvalues=dv)
    return enc, head, backward


def host_segments(opt):
    """[(w, g, m, v)] numpy copies of the optimiser's segments."""
    out = []
    for i, o, n in opt.segments():
        mod = opt.modules[i]
        out.append(tuple(np_(a)[o:o + n].copy() for a in (mod.weights, mod._last_dweights, opt.exp_avg[i],
                                                          opt.exp_avg_sq[i])))
    return out


def test_device_adam_steps_the_parameters_only(lib):
    import torch
    enc, head, backward = modules()
    opt = optim.DeviceAdam(ADAM, [enc, head], DEV)
    backward()
    ecfg = enc.cfg
    Hd, K = ecfg.embed_hidden, ecfg.F - 1 + ecfg.embedding_size + 1
    ln0 = ecfg.num_embeddings * ecfg.embedding_size + Hd * K + Hd       # the encoder's layer_norm entries
    fn = HEAD.in0 + HEAD.in1                                            # the head's feature_norm entries
    assert opt.segments() == [(0, 0, ln0), (0, ln0 + 2 * Hd, enc.weights.numel() - ln0 - 2 * Hd),
                              (1, 2 * fn, head.weights.numel() - 2 * fn)]
    enc._last_dweights[ln0:ln0 + 2 * Hd] = 1e30      # garbage where there is no parameter
    head._last_dweights[:2 * fn] = float("nan")
    for step in range(2):
        segs = host_segments(opt)
        state = np_(opt.state).copy()
        want = om.model32(om.Hyper(lr=7e-4, max_grad_norm=0.5), segs, state)
        res = opt.step()
        assert all(v.dim() == 0 and v.is_cuda for v in res.values()) and set(res) == {"grad_norm", "clip_coef", "skipped"}
        got = dict(segs=host_segments(opt), state=np_(opt.state), info=np_(opt.info))
        oc.same(got, want, "DeviceAdam, step %d" % (step + 1))
        assert float(res["grad_norm"]) == want[2][0] and 0 < float(res["clip_coef"]) < 1 and float(res["skipped"]) == 0
        one, zero = np.float32(1).view(np.int32), 0
        assert (bits_of(enc.weights[ln0:ln0 + Hd]) == one).all() and (bits_of(enc.weights[ln0 + Hd:ln0 + 2 * Hd]) == zero).all()
        assert (bits_of(head.weights[:fn]) == one).all() and (bits_of(head.weights[fn:2 * fn]) == zero).all()
        assert not bits_of(opt.exp_avg[0][ln0:ln0 + 2 * Hd]).any() and not bits_of(opt.exp_avg_sq[1][:2 * fn]).any()
    assert opt.lr_decay(3, 10) == 7e-4 - 7e-4 * (3 / 10.0) == opt.lr
    assert torch.equal(opt.step(lr=0.0)["skipped"].cpu(), torch.tensor(0.0))


def test_device_adam_refusals(lib):
    enc, head, backward = modules()
    opt = optim.DeviceAdam(ADAM, [enc, head], DEV)
    with pytest.raises(optim.OptimError, match="no gradient"):
        opt.step()
    backward(embed=False)
    with pytest.raises(optim.OptimError, match="without embed=True"):
        opt.step()
    backward()
    opt.step()
    backward(embed=False)
    with pytest.raises(optim.OptimError, match="without embed=True"):
        opt.step()
    with pytest.raises(optim.OptimError, match="CUDA"):
        optim.DeviceAdam(ADAM, [enc], "cpu")
    with pytest.raises(optim.OptimError, match="GraphEncoder and PolicyHead"):
        optim.DeviceAdam(ADAM, [object()], DEV)
    with pytest.raises(optim.OptimError, match="lr must be finite"):
        backward()
        opt.step(lr=-1.0)
    args = type("A", (), dict(lr=1e-3, critic_lr=2e-3, opti_eps=1e-5, weight_decay=0.0, max_grad_norm=10.0,
                              use_max_grad_norm=True))
    assert optim.AdamConfig.from_args(args).lr == 1e-3 and optim.AdamConfig.from_args(args, critic=True).lr == 2e-3
    assert optim.AdamConfig.from_args(args) == optim.AdamConfig(lr=1e-3)


def test_state_dict_round_trip(lib):
    import torch
    enc, head, backward = modules()
    opt = optim.DeviceAdam(ADAM, [enc, head], DEV)
    for _ in range(2):
        backward()
        opt.step()
    # the modules' state_dict is unpack_* of the blob
    esd, hsd = enc.state_dict(), head.state_dict()
    for sd, want in ((esd, gnn.unpack_weights(np_(enc.weights), enc.cfg)),
                     (hsd, policy.unpack_head_weights(np_(head.weights), HEAD))):
        assert set(sd) == set(want)
        for k in want:
            assert torch.equal(sd[k].view(torch.int32), torch.from_numpy(want[k]).view(torch.int32)), k
    assert not any("layer_norm" in k for k in esd) and not any("feature_norm" in k for k in hsd)
    assert "p.gnn1.lin_key.weight" in enc.state_dict(prefix="p.")
    sd = opt.state_dict()
    assert sd["step"] == 2 and set(sd["exp_avg"]) == set(sd["exp_avg_sq"]) == set(esd) | set(hsd)
    enc2, head2, backward2 = modules(gnn.pack_weights(esd, enc.cfg), policy.pack_head_weights(hsd, HEAD))
    assert torch.equal(enc2.weights.view(torch.int32), enc.weights.view(torch.int32))
    opt2 = optim.DeviceAdam(ADAM, [enc2, head2], DEV)
    opt2.load_state_dict(sd)
    assert torch.equal(opt2.state.view(torch.int64), opt.state.view(torch.int64))
    backward()
    backward2()
    opt.step()
    opt2.step()
    for a, b in [(enc.weights, enc2.weights), (head.weights, head2.weights), (opt.state, opt2.state),
                 (opt.info, opt2.info)] + list(zip(opt.exp_avg + opt.exp_avg_sq, opt2.exp_avg + opt2.exp_avg_sq)):
        np.testing.assert_array_equal(bits_of(a), bits_of(b))
    assert float(opt.state[0]) == 3.0
    del sd["exp_avg"]["gnn.gnn1.lin_key.weight"]
    with pytest.raises(optim.OptimError, match="gnn.gnn1.lin_key.weight is missing"):
        opt2.load_state_dict(sd)


# ---- the closed loop ----------------------------------------------------------------------------------------------

class Yardstick:
    """torch.optim.Adam + clip_grad_norm_ on the CPU and the float64 truth for one DeviceAdam, fed after each
    call with the weights before it and the gradients it used."""

    def __init__(self, opt, what):
        self.opt, self.what = opt, what
        self.h = om.Hyper(lr=opt.cfg.lr, max_grad_norm=opt.cfg.max_grad_norm)
        self.t32 = None
        self.m64 = self.v64 = None
        self.steps = 0

    def weights(self):
        return [np_(self.opt.modules[i].weights)[o:o + n].copy() for i, o, n in self.opt.segments()]

    def check(self, before, res):
        opt = self.opt
        grads = [np_(opt.modules[i]._last_dweights)[o:o + n].copy() for i, o, n in opt.segments()]
        if self.t32 is None:
            self.t32 = om.Torch32(self.h, before)
            self.m64 = [np.zeros(g.size) for g in grads]
            self.v64 = [np.zeros(g.size) for g in grads]
        ref, norm32 = self.t32.step(grads, weights=before)
        t64, norm64 = om.truth64(self.h, [(w.astype(np.float64), g.astype(np.float64), m, v)
                                          for w, g, m, v in zip(before, grads, self.m64, self.v64)], self.steps)
        self.m64, self.v64 = [s[2] for s in t64], [s[3] for s in t64]
        self.steps += 1
        om.within([float(res["grad_norm"])], [norm64], [norm32], "%s grad_norm, call %d" % (self.what, self.steps))
        assert float(res["skipped"]) == 0.0 and float(opt.state[0]) == self.steps
        for si, ((i, o, n), w) in enumerate(zip(opt.segments(), self.weights())):
            label = "%s call %d segment %d" % (self.what, self.steps, si)
            om.within(w, t64[si][0], ref[si][0], label + " weights")
            om.within(np_(opt.exp_avg[i])[o:o + n], t64[si][2], ref[si][1], label + " exp_avg")
            om.within(np_(opt.exp_avg_sq[i])[o:o + n], t64[si][3], ref[si][2], label + " exp_avg_sq")


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_ppo_update_closes_the_loop_on_a_collected_minibatch(lib, layout):
    """Six collect steps, one recurrent_generator minibatch of chunk length 3, ppo_update twice: after each call
    the weights, the moments and both norms are within the criterion of clip_grad_norm_ + torch.optim.Adam on
    the CPU, from the weights before the call and the gradients it used; evaluate_actions sees the new weights
    and equals a fresh DevicePolicy built from the state_dict()s; a third call with update_actor=False leaves
    the actor untouched to the bit."""
    import torch
    env = dp.env(layout)
    pol, _, _ = dp.heads(env, seed=1)
    buf = dp.collect(env, pol, 6)
    vn = DeviceValueNorm(DEV)
    next_value = pol.get_values(env, buf.rnn_states_critic[-1], buf.masks[-1], buffer=buf, row=-1)
    buf.compute_returns(next_value, vn, gamma=0.99, gae_lambda=0.95)
    adv, _ = buf.advantages(vn)
    mb = next(iter(buf.recurrent_generator(adv, 1, 3)))
    loss = PPOLoss(LossConfig(num_actions=25), DEV)
    aopt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [pol.actor_encoder, pol.actor_head], DEV)
    copt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [pol.critic_encoder, pol.critic_head], DEV)
    with pytest.raises(policy.PolicyError, match="actor_opt must be"):
        pol.optimizer_step(copt, copt)
    keys = ("values", "action_log_probs", "entropy")
    ev0 = {k: v.clone() for k, v in pol.evaluate_actions(mb, 3).items() if k in keys}
    yards = {"actor": Yardstick(aopt, layout + " actor"), "critic": Yardstick(copt, layout + " critic")}
    for call in range(2):
        before = {w: y.weights() for w, y in yards.items()}
        res = pol.ppo_update(mb, loss, vn, aopt, copt, data_chunk_length=3)
        assert set(res) == {"value_loss", "critic_grad_norm", "policy_loss", "dist_entropy", "actor_grad_norm",
                            "imp_weights", "skipped"}
        assert all(res[k].is_cuda for k in res if k != "skipped") and tuple(res["imp_weights"].shape) == (72, 1)
        for w, y in yards.items():
            y.check(before[w], {"grad_norm": res[w + "_grad_norm"], "skipped": res["skipped"][w]})
    ev1 = {k: v.clone() for k, v in pol.evaluate_actions(mb, 3).items() if k in keys}
    for k in keys:
        assert not torch.equal(ev1[k], ev0[k]), "%s did not move with the weights" % k
    sds = [m.state_dict() for m in (pol.actor_encoder, pol.actor_head, pol.critic_encoder, pol.critic_head)]
    fresh = policy.DevicePolicy(
        gnn.GraphEncoder(pol.actor_encoder.cfg, gnn.pack_weights(sds[0], pol.actor_encoder.cfg), DEV),
        policy.PolicyHead(pol.actor_head.cfg, policy.pack_head_weights(sds[1], pol.actor_head.cfg), DEV),
        gnn.GraphEncoder(pol.critic_encoder.cfg, gnn.pack_weights(sds[2], pol.critic_encoder.cfg), DEV),
        policy.PolicyHead(pol.critic_head.cfg, policy.pack_head_weights(sds[3], pol.critic_head.cfg), DEV))
    ev2 = fresh.evaluate_actions(mb, 3)
    for k in keys:
        assert torch.equal(ev2[k].view(torch.int32), ev1[k].view(torch.int32)), k
    # the critic alone
    held = [t.clone() for t in (pol.actor_encoder.weights, pol.actor_head.weights, aopt.state, *aopt.exp_avg,
                                *aopt.exp_avg_sq)]
    critic = [pol.critic_encoder.weights.clone(), pol.critic_head.weights.clone()]
    res = pol.ppo_update(mb, loss, vn, aopt, copt, data_chunk_length=3, update_actor=False)
    assert res["actor_grad_norm"] is None and res["policy_loss"] is None and res["skipped"]["actor"] is None
    now = (pol.actor_encoder.weights, pol.actor_head.weights, aopt.state, *aopt.exp_avg, *aopt.exp_avg_sq)
    for a, b in zip(now, held):
        np.testing.assert_array_equal(bits_of(a), bits_of(b), "update_actor=False touched the actor")
    assert not torch.equal(pol.critic_encoder.weights, critic[0]) and not torch.equal(pol.critic_head.weights, critic[1])
    assert float(copt.state[0]) == 3.0 and float(aopt.state[0]) == 2.0 and float(res["critic_grad_norm"]) > 0
    buf.detach()
    env.close()
