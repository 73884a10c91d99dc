"""GPU tests of the spilled tier of the graph encoder's backward pass (csrc/lsm_gnn_backward.hip through
include/lsm_gnn_backward_large.h, lsm/gnn.py, lsm/policy.py and lsm/trainer.py): every spill level bit-equal to
level 0 and to lsm_gnn_backward (the sum order is the contract, so a region addressed wrongly, a missed barrier
or a scratch overlap shows as a changed bit); the scratch across groups and slabs; sizes beyond the old limit
against tests/gnn_backward_model.py's float64 model within the case's own tolerance; GraphEncoder's wrappers;
and one training iteration at 16 agents with wide encoders, where the device learner used to refuse."""
import dataclasses

import numpy as np
import pytest

import gnn_abi as ga
import gnn_backward_cases as bc
import gnn_backward_large_cases as lc
import gnn_embed_backward_cases as ec
import gnn_model as gm
import policy_model as pm
from lsm import capi, gnn, optim, policy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return bc._lib()


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


# ---- the levels agree bit for bit ---------------------------------------------------------------------------------

LEVEL_CASES = {"shape E24 B G+1": lambda: bc.shape_case(24, 2), "node": lambda: bc.readout_case("node"),
               "global_mean": lambda: bc.readout_case("global_mean"), "global_max": lambda: bc.readout_case("global_max"),
               "global_add": lambda: bc.readout_case("global_add"), "structure": bc.structure_case,
               "wideB E16": lambda: lc.case("wideB", 16, B=3)}


@pytest.mark.parametrize("name", sorted(LEVEL_CASES))
def test_levels_agree_bit_for_bit(lib, name):
    """min_spill 0 .. 4 in both layouts, the workspace sized exactly between canaries (at the odd levels only
    8-byte aligned); then level 4 again and on a second stream."""
    import torch
    case = LEVEL_CASES[name]()
    aid = case.agent_id if case.cfg.aggr == "node" else None
    srcs = case.sources(DEV)
    want = bc.call(lib, case.cfg, case.blob, case.x, srcs["reference"], aid, case.dout)
    assert want["bad"] == 0
    run = lambda k, layout, **kw: lc.call(lib, case.cfg, case.blob, case.x, srcs[layout], aid, case.dout, min_spill=k,
                                          ws_off=2 * (k & 1), **kw)
    for k in range(5):
        p = lc.plan(case.cfg, case.B, case.E, min_spill=k)[0]
        assert p["spill"] == k and (p["scratch_bytes"] > 0) == (k > 0), p
        print("large plan %s min_spill %d: %s" % (case.name, k, p))
        for layout in bc.LAYOUTS:
            lc.same_bits(want, run(k, layout), "%s level %d %s" % (case.name, k, layout))
    lc.same_bits(want, run(4, "compact"), "level 4 twice")
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        other = run(2, "reference", stream=s)
    torch.cuda.synchronize()
    lc.same_bits(want, other, "level 2 on a second stream")


@pytest.mark.parametrize("B", [bc.SLAB + 1, 2 * bc.SLAB + 3])
def test_scratch_reuse_and_the_slab_edge(lib, B):
    """A slab's teams reuse their scratch regions group after group; the last slab is short, its idle teams
    recompute graph B - 1 into their own regions. The canaries sit directly behind the last slab's scratch."""
    case = bc.slab_case(B)
    src = case.sources(DEV)["reference"]
    p = lc.plan(case.cfg, B, case.E, min_spill=4)[0]
    assert p["spill"] == 4 and p["slabs"] == (B + bc.SLAB - 1) // bc.SLAB and p["G"] > 1
    assert p["ws_bytes"] == lc.ws_bytes(case.cfg, B, case.E, 4)
    want = lc.call(lib, case.cfg, case.blob, case.x, src, None, case.dout, min_spill=0)
    lc.same_bits(want, bc.call(lib, case.cfg, case.blob, case.x, src, None, case.dout), "level 0 is lsm_gnn_backward")
    for off in (0, 2):
        lc.same_bits(want, lc.call(lib, case.cfg, case.blob, case.x, src, None, case.dout, min_spill=4, ws_off=off),
                     "B %d level 4" % B)


# ---- beyond the old limit -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,E", [("default", 114), ("default", 192), ("default", 256), ("wideA", 31), ("wideA", 48),
                                    ("wideB", 39)])
def test_beyond_the_old_limit(lib, name, E):
    case = lc.case(name, E)
    assert bc.plan(case.cfg, case.B, E)[0] is None
    p = lc.plan(case.cfg, case.B, E)[0]
    print("large plan %s: %s" % (case.name, p))
    assert p["spill"] >= 1 and p["TS"] == max(32, 1 << (E - 1).bit_length())
    lc.check(lib, case, DEV)


@pytest.mark.parametrize("level", [1, 2, 3, 4])
def test_the_smallest_size_of_each_level(lib, level):
    """wideB: the smallest E at which the plan reports each level."""
    E = lc.first_E_of_each_level("wideB")[level]
    case = lc.case("wideB", E)
    p = lc.plan(case.cfg, case.B, E)[0]
    print("large plan %s: %s" % (case.name, p))
    assert p["spill"] == level and lc.plan(case.cfg, case.B, E - 1)[0]["spill"] == level - 1
    lc.check(lib, case, DEV)


# ---- the wrapper --------------------------------------------------------------------------------------------------

def test_wrapper_beyond_the_old_limit(lib):
    """GraphEncoder.backward / backward_compact / backward_step at wideA, E = 48: the ctypes call's bytes, and
    gradients(); with embed=True the EmbedConv range is embed_backward's."""
    import torch
    import recurrent_model as rcm
    case = lc.case("wideA", 48, aggr="node")
    srcs = case.sources(DEV)
    want = lc.call(lib, case.cfg, case.blob, case.x, srcs["reference"], case.agent_id, case.dout)
    enc = gnn.GraphEncoder(case.cfg, case.blob, DEV)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    x, dout, aid, full = t(case.x), t(case.dout), t(case.agent_id), t(case.full)
    out = enc.backward(x, full, dout, aid, dh0=True, check=True)
    np.testing.assert_array_equal(bits(out["dweights"]), want["dweights"].view(np.int32))
    np.testing.assert_array_equal(bits(out["dh0"]), want["dh0"].view(np.int32))
    grads, got = enc.gradients(), bc.split(case.cfg, want["dweights"])
    assert set(grads) == {"gnn." + n for n in got}
    for n, g in got.items():
        np.testing.assert_array_equal(bits(grads["gnn." + n]), g.view(np.int32))
    table, bts, N = case._found["compact"]
    masks = t(rcm.pack_bits(bts).view(np.int64))
    for o in (enc.backward_compact(x, t(table), masks, N, dout, aid, dh0=True),
              enc.backward_step(x.reshape(-1, N, case.E, case.cfg.F), t(table), masks.reshape(-1, N, 1), N, dout,
                                aid.reshape(-1, N), dh0=True)):
        np.testing.assert_array_equal(bits(o["dweights"]), want["dweights"].view(np.int32))
        np.testing.assert_array_equal(bits(o["dh0"]), want["dh0"].view(np.int32))
    # embed=True: the conv range unchanged, the EmbedConv range embed_backward's on this call's dh0
    n0 = bc.conv0(case.cfg)
    dembed = enc.embed_backward(x, full, out["dh0"].clone())["dembed"].clone()
    both = enc.backward(x, full, dout, aid, embed=True)
    np.testing.assert_array_equal(bits(both["dweights"])[n0:], want["dweights"].view(np.int32)[n0:])
    np.testing.assert_array_equal(bits(both["dweights"])[:n0], bits(dembed))
    assert np.abs(dembed.cpu().numpy()).max() > 0
    # a size the forward refuses still raises
    with pytest.raises(gnn.GnnError, match="lsm_gnn_forward refuses"):
        enc.backward(torch.zeros((1, 65, case.cfg.F), device=DEV), torch.zeros((1, 65, 65), device=DEV),
                     dout[:1], aid[:1])


def test_wrapper_below_the_limit_is_unchanged(lib):
    import torch
    case = bc.shape_case(24, 1)
    want = bc.call(lib, case.cfg, case.blob, case.x, case.sources(DEV)["reference"], case.agent_id, case.dout)
    enc = gnn.GraphEncoder(case.cfg, case.blob, DEV)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=DEV)
    out = enc.backward(t(case.x), t(case.full), t(case.dout), t(case.agent_id), dh0=True)
    np.testing.assert_array_equal(bits(out["dweights"]), want["dweights"].view(np.int32))
    np.testing.assert_array_equal(bits(out["dh0"]), want["dh0"].view(np.int32))
    # the cached workspace is sized by the entry point that is used: lsm_gnn_backward's here
    ws = enc._bwd_outputs(case.B, case.E)
    assert ws["large"] is False and ws["workspace"].numel() * 8 == bc.ws_bytes(case.cfg, case.B, case.E)
    big = lc.case("wideA", 48)
    ws = gnn.GraphEncoder(big.cfg, big.blob, DEV)._bwd_outputs(2, 48)
    assert ws["large"] is True and ws["workspace"].numel() * 8 >= lc.ws_bytes(big.cfg, 2, 48) > bc.ws_bytes(big.cfg, 2, 48)


# ---- training where it was refused --------------------------------------------------------------------------------

T, L = 4, 2


def wide_env(layout="reference"):
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    env = GpuGraphVecEnv(EnvArgs(num_agents=16, seed=1), num_envs=2, device=DEV, return_numpy=False, build_infos=False,
                         adj_layout=layout)
    assert env.E == 48 and env.N == 16
    return env


def wide_policy(env, seed=1):
    """dp.heads with wideA encoders and 64-wide encoder outputs at the heads; the critic's first block is obs when
    share_obs would exceed the heads' 256-wide input."""
    N, OBS, F = env.N, env.OBS, env.F
    acfg = dataclasses.replace(lc.WIDE_A, F=F, aggr="node")
    ccfg = dataclasses.replace(lc.WIDE_A, F=F, aggr="global_mean")
    ah = policy.HeadConfig(kind="actor", in0=OBS, in1=64, num_actions=25, recurrent_N=1)
    ch = policy.HeadConfig(kind="critic", in0=N * OBS if N * OBS + 64 <= 256 else OBS, in1=64, recurrent_N=1)
    asd, csd = pm.random_head_weights(ah, 11 + seed), pm.random_head_weights(ch, 12 + seed)
    return policy.DevicePolicy(gnn.GraphEncoder(acfg, gm.default_weights(acfg, 5)[1], DEV),
                               policy.PolicyHead(ah, policy.pack_head_weights(asd, ah), DEV),
                               gnn.GraphEncoder(ccfg, gm.default_weights(ccfg, 6)[1], DEV),
                               policy.PolicyHead(ch, policy.pack_head_weights(csd, ch), DEV))


def test_encoders_backward_at_16_agents_with_wide_encoders(lib):
    """ppo_loss, heads_backward(dx=True), encoders_backward(embed=True) on a collected minibatch: both encoders'
    gradients are the direct ctypes calls' on the same minibatch and dx1."""
    import device_policy_cases as dp
    from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss
    env = wide_env()
    pol = wide_policy(env)
    buf = dp.collect(env, pol, T)
    vn = DeviceValueNorm(DEV)
    next_value = pol.get_values(env, buf.rnn_states_critic[-1], buf.masks[-1], buffer=buf, row=-1)
    buf.compute_returns(next_value, vn, gamma=0.99, gae_lambda=0.95)
    adv, _ = buf.advantages(vn)
    mb = next(iter(buf.recurrent_generator(adv, 2, L)))
    loss = PPOLoss(LossConfig(num_actions=25), DEV)
    out = pol.ppo_loss(mb, loss, vn, data_chunk_length=L)
    heads = pol.heads_backward(mb, out, data_chunk_length=L, dx=True)
    got = pol.encoders_backward(mb, heads, dh0=True, embed=True)
    np_ = lambda x: x.detach().cpu().numpy()
    x, full, aid = np_(mb["node_obs"]), np_(mb["adj"]), np_(mb["agent_id"]).reshape(-1)
    assert x.shape == (64, 48, env.F)
    src = ga.dense_sources(full, DEV)["reference"]
    for who, enc in (("actor", pol.actor_encoder), ("critic", pol.critic_encoder)):
        assert bc.plan(enc.cfg, 64, 48)[0] is None and lc.plan(enc.cfg, 64, 48)[0]["spill"] >= 1
        blob = np_(enc.weights)
        want = lc.call(lib, enc.cfg, blob, x, src, aid if enc.cfg.aggr == "node" else None, np_(heads[who]["dx1"]))
        n0 = bc.conv0(enc.cfg)
        dw = np_(got[who]["dweights"])
        np.testing.assert_array_equal(dw.view(np.int32)[n0:], want["dweights"].view(np.int32)[n0:], who)
        np.testing.assert_array_equal(np_(got[who]["dh0"]).view(np.int32), want["dh0"].view(np.int32), who)
        emb = ec.call(lib, enc.cfg, blob, x, src, want["dh0"])
        np.testing.assert_array_equal(dw.view(np.int32)[:n0], emb["dembed"].view(np.int32), who)
        assert np.isfinite(dw).all() and np.abs(dw[:n0]).max() > 0 and np.abs(dw[n0:]).max() > 0
    buf.detach()
    env.close()


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_train_at_16_agents_with_wide_encoders(lib, layout):
    """One DeviceTrainer.train of one epoch of two minibatches against the loop by hand, as test_gpu_trainer.py
    compares them: every blob, both Adam moments, the optimiser and normaliser state, and train_info."""
    import torch
    import device_policy_cases as dp
    import test_gpu_trainer as tt
    from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss
    from lsm.trainer import DeviceTrainer, TrainConfig

    class Side(tt.Side):
        def __init__(self, env):
            self.pol = wide_policy(env)
            self.vn = DeviceValueNorm(DEV)
            self.loss = PPOLoss(LossConfig(num_actions=25), DEV)
            self.aopt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [self.pol.actor_encoder, self.pol.actor_head], DEV)
            self.copt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [self.pol.critic_encoder, self.pol.critic_head], DEV)

    cfg = TrainConfig(ppo_epoch=1, num_mini_batch=2, data_chunk_length=L)
    env = wide_env(layout)
    A, B = Side(env), Side(env)
    tt.same_tensors(A.snapshot(), B.snapshot(), "A and B start alike")
    buf = dp.collect(env, A.pol, T)
    tr = A.trainer(cfg)
    tr.compute(env, buf, **tt.RETURNS)
    start = A.snapshot()
    g = torch.Generator().manual_seed(3)
    P = [torch.randperm(T * 2 * 16 // L, generator=g).to(DEV)]
    res = tr.train(buf, permutations=P)
    want = tt.by_hand(B, buf, cfg, permutations=P)
    now = A.snapshot()
    tt.same_tensors(now, B.snapshot(), layout + ": trainer against the loop by hand")
    assert all((now[k] != start[k]).any() for k in now), "every blob, moment and state moved"
    tt.check_result(res, want, layout, updates=2)
    assert int(res["updates"]) == 2 and int(res["first_nonfinite"]) == -1
    assert np.isfinite(want["train_info"]).all() and (want["counts"][:6] == 2).all()
    buf.detach()
    env.close()
