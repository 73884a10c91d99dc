"""GPU tests of the graph encoder's backward pass (csrc/lsm_gnn_backward.hip through include/lsm_gnn_backward.h,
lsm/gnn.py and lsm/policy.py): the kernel against tests/gnn_backward_model.py's float64 model within the tolerance
measured per case and gradient tensor (4 * e32 + 4 * 2^-23 * s) on tests/gnn_backward_cases.py's cases, in both
adjacency layouts (bit-equal to each other) with canaries around every output and the workspace; twice bit-equal;
ego_only; a second stream; every launch plan; then the public surface: ppo_loss, heads_backward(dx=True) and
encoders_backward on a collected minibatch."""
import dataclasses

import numpy as np
import pytest

import device_policy_cases as dp
import gnn_abi as ga
import gnn_backward_cases as bc
import gnn_backward_model as gbm
import gnn_model as gm
from lsm import capi, gnn, policy
from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("E", bc.SHAPE_E)
@pytest.mark.parametrize("which", range(3))
def test_shapes(lib, E, which):
    bc.check(lib, bc.shape_case(E, which), DEV)


@pytest.mark.parametrize("name", bc.OPTION_NAMES)
def test_options(lib, name):
    bc.check(lib, bc.option_case(name), DEV)


@pytest.mark.parametrize("aggr", ["node", "global_mean", "global_max", "global_add"])
def test_readouts(lib, aggr):
    bc.check(lib, bc.readout_case(aggr), DEV)


def test_structure(lib):
    bc.structure_checks(lib, DEV)


def test_bad_inputs(lib):
    bc.bad_input_checks(lib, DEV)


@pytest.mark.parametrize("B", bc.SLAB_B)
def test_slabs(lib, B):
    """Around the slab's edge; the sum order is the contract, so the kernel's conv gradients are the host entry
    point's up to what expf and the fused multiply-adds differ by: both within the case's bound."""
    bc.check(lib, bc.slab_case(B), DEV, layouts=("reference",))


def test_every_launch_plan(lib):
    for key in bc.plan_sizes():
        bc.check(lib, bc.plan_case(key), DEV, layouts=("reference",))


def test_largest_E_and_the_refusal_beyond(lib):
    case = bc.max_E_case()
    bc.check(lib, case, DEV)
    E = case.E + 1
    x, table, bits = gm.random_graphs(1, E, case.cfg.F, seed=1)
    src = ga.sources(table, bits, 1, DEV)["reference"]
    r = bc.call(lib, case.cfg, case.blob, x, src, None, np.zeros((1, case.cfg.out_dim), np.float32), expect_rc=1)
    assert "bytes of LDS per graph" in r["err"]


def test_twice_ego_only_and_a_second_stream(lib):
    import torch
    case = bc.shape_case(24, 2)
    src = case.sources(DEV)["compact"]
    run = lambda cfg=case.cfg, **kw: bc.call(lib, cfg, case.blob, case.x, src, case.agent_id, case.dout, **kw)
    a = run()
    others = [run(), run(dataclasses.replace(case.cfg, ego_only=True))]
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        others.append(run(stream=s))
    torch.cuda.synchronize()
    for o in others:
        np.testing.assert_array_equal(a["dweights"].view(np.int32), o["dweights"].view(np.int32))
        np.testing.assert_array_equal(a["dh0"].view(np.int32), o["dh0"].view(np.int32))


def test_wrapper(lib):
    """GraphEncoder.backward / backward_compact / backward_step and gradients(): the ctypes call's bytes."""
    import torch
    case = bc.shape_case(24, 1)
    srcs = case.sources(DEV)
    want = bc.call(lib, case.cfg, case.blob, case.x, srcs["reference"], case.agent_id, case.dout)
    enc = gnn.GraphEncoder(case.cfg, case.blob, DEV)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    x, dout, aid = t(case.x), t(case.dout), t(case.agent_id)
    with pytest.raises(gnn.GnnError, match="follows a backward"):
        enc.gradients()
    out = enc.backward(x, t(case.full), dout, aid, dh0=True, check=True)
    np.testing.assert_array_equal(out["dweights"].cpu().numpy().view(np.int32), want["dweights"].view(np.int32))
    np.testing.assert_array_equal(out["dh0"].cpu().numpy().view(np.int32), want["dh0"].view(np.int32))
    grads = enc.gradients()
    got = bc.split(case.cfg, want["dweights"])
    assert set(grads) == {"gnn." + n for n in got}
    for n, g in got.items():
        assert tuple(grads["gnn." + n].shape) == g.shape
        np.testing.assert_array_equal(grads["gnn." + n].cpu().numpy().view(np.int32), g.view(np.int32))
    assert enc.backward(x, t(case.full), dout, aid)["dh0"] is None
    table, bits, N = case._found["compact"]
    import recurrent_model as rcm
    masks = t(rcm.pack_bits(bits).view(np.int64))
    for o in (enc.backward_compact(x, t(table), masks, N, dout, aid, dh0=True),
              enc.backward_step(x.reshape(-1, N, case.E, case.cfg.F), t(table), masks.reshape(-1, N, 1), N, dout,
                                aid.reshape(-1, N), dh0=True)):
        np.testing.assert_array_equal(o["dweights"].cpu().numpy().view(np.int32), want["dweights"].view(np.int32))
        np.testing.assert_array_equal(o["dh0"].cpu().numpy().view(np.int32), want["dh0"].view(np.int32))
    with pytest.raises(gnn.GnnError, match="dout"):
        enc.backward(x, t(case.full), dout[:, :3], aid)
    with pytest.raises(gnn.GnnError, match="agent_id"):
        enc.backward(x, t(case.full), dout)


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_encoders_backward_closes_the_loop_on_a_collected_minibatch(lib, layout):
    """Six collect steps, compute_returns and advantages, one recurrent_generator minibatch with
    data_chunk_length 3, ppo_loss, heads_backward(dx=True), encoders_backward: both encoders' conv gradients and
    dh0 are the float64 model's on the same tensors copied to the host (dout: each head's dx1)."""
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
    with pytest.raises(policy.PolicyError, match="follows ppo_loss"):
        policy.DevicePolicy.encoders_backward(_Fresh(pol), mb, {})
    out = pol.ppo_loss(mb, loss, vn, data_chunk_length=3)
    heads = pol.heads_backward(mb, out, data_chunk_length=3, dx=True)
    with pytest.raises(policy.PolicyError, match="dx1"):
        pol.encoders_backward(mb, pol.heads_backward(mb, out, data_chunk_length=3))
    heads = pol.heads_backward(mb, out, data_chunk_length=3, dx=True)
    got = pol.encoders_backward(mb, heads, dh0=True)
    np_ = lambda x: x.detach().cpu().numpy()
    x, full, aid = np_(mb["node_obs"]), np_(mb["adj"]), np_(mb["agent_id"]).reshape(-1)
    assert x.shape[0] == 72
    for who, enc, seed in (("actor", pol.actor_encoder, 5), ("critic", pol.critic_encoder, 6)):
        sd, blob = gm.default_weights(enc.cfg, seed)
        truth = gbm.Truth(enc.cfg, sd, x, full, np_(heads[who]["dx1"]), aid)
        assert truth.why_not is None, truth.why_not
        dw = np_(got[who]["dweights"])
        assert not dw[:bc.conv0(enc.cfg)].view(np.int32).any()
        parts = bc.split(enc.cfg, dw)
        grads = enc.gradients()
        for name in truth.names():
            o = np_(got[who]["dh0"]) if name == "dh0" else parts[name]
            bc.assert_close(o, truth, name, "closed loop %s %s" % (layout, who))
            if name != "dh0":
                assert torch.equal(grads["gnn." + name].view(torch.int32).cpu(),
                                   torch.as_tensor(parts[name]).view(torch.int32))
    half = pol.encoders_backward(mb, heads, update_actor=False)
    assert half["actor"] is None and half["critic"]["dh0"] is None
    assert torch.equal(half["critic"]["dweights"].view(torch.int32), got["critic"]["dweights"].view(torch.int32))
    buf.detach()
    env.close()


class _Fresh:
    """A policy object that has not evaluated anything yet."""

    def __init__(self, pol):
        self.last_head_inputs = None
        self.actor_encoder, self.critic_encoder = pol.actor_encoder, pol.critic_encoder
