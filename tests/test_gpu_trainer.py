"""GPU tests of GR_MAPPO.train on the device (csrc/lsm_train_info.hip through include/lsm_train_info.h, and
lsm/trainer.py): the accumulator's kernels bit-equal to the host entry points on tests/train_info_model.py's cases,
then DeviceTrainer.train against the same loop written by hand on the pieces it orders -- advantages, the
generators, DevicePolicy.ppo_update -- with the scalars of every minibatch read back and averaged on the host in
float64: weights, moments, optimiser and normaliser state bit-equal, train_info the bits of float32(mean64). The
yardstick is the existing, already tested pieces; the code under test only orders them. Sizes: 4 envs x 3 agents,
T = 6, chunks of 3, two epochs of two minibatches (24 chunks, 12 per minibatch, four updates)."""
import types

import numpy as np
import pytest

import device_policy_cases as dp
import train_info_model as tm
from lsm import capi, optim, policy
from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss
from lsm.trainer import COUNT_KEYS, REFERENCE_KEYS, DeviceTrainer, TrainConfig, TrainerError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T, L, EPOCHS, MINIBATCHES = 6, 3, 2, 2
UPDATES = EPOCHS * MINIBATCHES
RETURNS = dict(gamma=0.99, gae_lambda=0.95)
CFG = TrainConfig(ppo_epoch=EPOCHS, num_mini_batch=MINIBATCHES, data_chunk_length=L)
CFG_FF = TrainConfig(ppo_epoch=EPOCHS, num_mini_batch=MINIBATCHES, data_chunk_length=L, use_recurrent_policy=False)


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


def np_(t):
    return t.detach().cpu().numpy()


def bits_of(t):
    return tm.bits(np_(t))


# ---- the kernels ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_kernels_equal_the_host_entry_points(lib, name):
    seq, num, garbage = tm.CASES[name]
    dev, host = tm.run(lib, seq, num, dev=DEV, garbage=garbage), tm.run(lib, seq, num, garbage=garbage)
    tm.same(dev, host, name + ": device against host")
    tm.same(dev, tm.model(seq, num), name + ": device against the model")


def test_kernels_on_a_second_stream_and_twice(lib):
    import torch
    seq, num, garbage = tm.CASES["seven_updates"]
    once = tm.run(lib, seq, num, dev=DEV, garbage=garbage)
    tm.same(tm.run(lib, seq, num, dev=DEV, garbage=garbage), once, "the same sequence twice")
    tm.same(tm.run(lib, seq, num, dev=DEV, stream=torch.cuda.Stream(DEV), garbage=garbage), once, "a second stream")


# ---- the closed loop --------------------------------------------------------------------------------------------

class Side:
    """One learner: a policy, its optimisers, value normaliser and loss, built from dp.heads' state dicts (the
    same for every Side of one seed and recurrent_N)."""

    def __init__(self, env, recurrent_N=1):
        self.pol, _, _ = dp.heads(env, recurrent_N=recurrent_N, seed=1)
        self.vn = DeviceValueNorm(DEV)
        self.loss = PPOLoss(LossConfig(num_actions=25), DEV)
        self.aopt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [self.pol.actor_encoder, self.pol.actor_head], DEV)
        self.copt = optim.DeviceAdam(optim.AdamConfig(lr=7e-4), [self.pol.critic_encoder, self.pol.critic_head], DEV)

    def trainer(self, cfg=CFG):
        return DeviceTrainer(self.pol, self.loss, self.vn, self.aopt, self.copt, cfg)

    def actor(self):
        return {"actor_encoder": self.pol.actor_encoder.weights, "actor_head": self.pol.actor_head.weights,
                "actor state": self.aopt.state,
                **{"actor exp_avg %d" % i: t for i, t in enumerate(self.aopt.exp_avg)},
                **{"actor exp_avg_sq %d" % i: t for i, t in enumerate(self.aopt.exp_avg_sq)}}

    def tensors(self):
        return {**self.actor(),
                "critic_encoder": self.pol.critic_encoder.weights, "critic_head": self.pol.critic_head.weights,
                "critic state": self.copt.state,
                **{"critic exp_avg %d" % i: t for i, t in enumerate(self.copt.exp_avg)},
                **{"critic exp_avg_sq %d" % i: t for i, t in enumerate(self.copt.exp_avg_sq)},
                "value norm state": self.vn.state, "value norm denorm": self.vn.denorm}

    def snapshot(self):
        return {k: bits_of(t).copy() for k, t in self.tensors().items()}


def same_tensors(a, b, what):
    assert set(a) == set(b)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], "%s: %s" % (what, k))


def by_hand(side, buf, cfg=CFG, permutations=None, generator=None, update_actor=True):
    """GR_MAPPO.train written on the pieces, with the reference's reads after every minibatch (the six scalars
    and the two skip flags) and its float64 sums on the host. ratio is the loss's stats entry (the row
    policy_loss is a view of; ppo_update hands out imp_weights, whose mean it is to float32 rounding)."""
    adv, stats = buf.advantages(side.vn)
    sums, counts = np.zeros(tm.SLOTS, np.float64), np.zeros(tm.SLOTS, np.int64)
    flat = buf.T * buf.env.num_envs * buf.env.N
    for e in range(cfg.ppo_epoch):
        perm = None if permutations is None else permutations[e]
        if cfg.use_recurrent_policy:
            batches, Lc = buf.recurrent_generator(adv, cfg.num_mini_batch, cfg.data_chunk_length, chunks=perm,
                                                  generator=generator), cfg.data_chunk_length
        else:
            batches, Lc = buf.feed_forward_generator(adv, cfg.num_mini_batch, indices=perm, generator=generator), None
        for mb in batches:
            if Lc is None:
                mb = dict(mb, actions=buf.actions.reshape(flat, -1)[mb["indices"]],
                          action_log_probs=buf.action_log_probs.reshape(flat, -1)[mb["indices"]])
            res = side.pol.ppo_update(mb, side.loss, side.vn, side.aopt, side.copt, data_chunk_length=Lc,
                                      update_actor=update_actor)
            ratio = None
            if update_actor:
                ratio = res["policy_loss"]._base[3]
                mean = float(res["imp_weights"].double().mean())
                assert abs(float(ratio) - mean) <= 1e-5 * abs(mean), "stats[3] is imp_weights.mean()"
            vals = (res["value_loss"], res["policy_loss"], res["dist_entropy"], res["actor_grad_norm"],
                    res["critic_grad_norm"], ratio, res["skipped"]["actor"], res["skipped"]["critic"])
            for k, v in enumerate(vals):
                if v is not None:
                    sums[k] += np.float64(np_(v).astype(np.float32))    # the read the trainer does not make
                    counts[k] += 1
    out = np.empty(tm.SLOTS, np.float32)
    out[:tm.MEANS] = (sums[:tm.MEANS] / np.float64(cfg.num_updates)).astype(np.float32)
    out[tm.MEANS:] = sums[tm.MEANS:].astype(np.float32)
    return dict(train_info=out, counts=counts, advantage_stats=np_(stats))


def check_result(res, want, what, updates=UPDATES):
    np.testing.assert_array_equal(bits_of(res["train_info"]), tm.bits(want["train_info"]), what + ": train_info")
    np.testing.assert_array_equal(np_(res["counts"]), want["counts"], what + ": counts")
    np.testing.assert_array_equal(bits_of(res["advantage_stats"]), tm.bits(want["advantage_stats"]), what)
    assert int(res["updates"]) == updates and int(res["first_nonfinite"]) == -1
    for k, name in enumerate(capi.TRAIN_INFO_SLOTS):
        assert res[name].dim() == 0 and res[name].data_ptr() == res["train_info"].data_ptr() + 4 * k


def permutations(n, seed=3):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(n, generator=g).to(DEV) for _ in range(EPOCHS)]


def prepared(layout="reference", recurrent_N=1):
    """(env, A, B, the buffer A collected with returns computed): A and B are bit-identical learners."""
    env = dp.env(layout)
    A, B = Side(env, recurrent_N), Side(env, recurrent_N)
    same_tensors(A.snapshot(), B.snapshot(), "A and B start alike")
    buf = dp.collect(env, A.pol, T)
    return env, A, B, buf


@pytest.mark.parametrize("layout", ["reference", "compact"])
def test_train_equals_the_loop_by_hand(lib, layout):
    """Also update_actor=False, and a second train() after after_update and a fresh collect, on the same two
    learners: the state restarts through `first`, no stale sum survives."""
    env, A, B, buf = prepared(layout)
    tr = A.trainer()
    tr.compute(env, buf, **RETURNS)
    start = A.snapshot()
    P = permutations(T * 4 * 3 // L)
    res = tr.train(buf, permutations=P)
    want = by_hand(B, buf, permutations=P)
    now = A.snapshot()
    same_tensors(now, B.snapshot(), layout + ": trainer against the loop by hand")
    assert all((now[k] != start[k]).any() for k in now), "every blob, moment and state moved"
    check_result(res, want, layout)
    assert (want["counts"] == UPDATES).all() and float(A.aopt.state[0]) == UPDATES
    host = tr.train_info_host()
    assert list(host) == list(REFERENCE_KEYS + COUNT_KEYS)
    assert all(np.float32(host[k]) == want["train_info"][i] for i, k in enumerate(REFERENCE_KEYS))
    assert host["actor_skipped"] == 0 and host["critic_skipped"] == 0 and all(np.isfinite(want["train_info"]))
    assert want["train_info"][3] > 0 and want["train_info"][4] > 0 and want["train_info"][2] > 0

    # the critic alone
    held = {k: bits_of(t).copy() for k, t in A.actor().items()}
    res = tr.train(buf, update_actor=False, permutations=P)
    want = by_hand(B, buf, permutations=P, update_actor=False)
    same_tensors({k: bits_of(t) for k, t in A.actor().items()}, held, "update_actor=False touched the actor")
    same_tensors(A.snapshot(), B.snapshot(), layout + ": update_actor=False")
    check_result(res, want, layout + ": update_actor=False")
    info, counts = np_(res["train_info"]), np_(res["counts"])
    assert all(info[k] == 0 and counts[k] == 0 for k in tm.ACTOR) and all(counts[k] == UPDATES for k in tm.CRITIC)
    assert info[0] > 0 and info[4] > 0

    # a second iteration: after_update, a fresh collect by the updated policy, compute, train
    buf.after_update()
    import torch
    g = torch.Generator(device=DEV).manual_seed(9)
    for t in range(T):
        out = A.pol.get_actions(env, buf.rnn_states[t], buf.rnn_states_critic[t], buf.masks[t], generator=g, buffer=buf)
        buf.insert_step(out["actions_env"], 0, value_preds=out["values"],
                        policy={k: out[k] for k in ("actions", "action_log_probs", "rnn_states", "rnn_states_critic")})
    tr.compute(env, buf, **RETURNS)
    P2 = permutations(T * 4 * 3 // L, seed=4)
    res = tr.train(buf, permutations=P2)
    want = by_hand(B, buf, permutations=P2)
    same_tensors(A.snapshot(), B.snapshot(), layout + ": the second train()")
    check_result(res, want, layout + ": the second train()")
    assert (np_(res["counts"]) == UPDATES).all()
    buf.detach()
    env.close()


def test_feed_forward_minibatches(lib):
    env, A, B, buf = prepared(recurrent_N=0)
    tr = A.trainer(CFG_FF)
    tr.compute(env, buf, **RETURNS)
    P = permutations(T * 4 * 3)
    res = tr.train(buf, permutations=P)
    want = by_hand(B, buf, CFG_FF, permutations=P)
    same_tensors(A.snapshot(), B.snapshot(), "feed-forward: trainer against the loop by hand")
    check_result(res, want, "feed-forward")
    assert float(A.aopt.state[0]) == UPDATES and float(A.copt.state[0]) == UPDATES
    buf.detach()
    env.close()


def test_default_permutation_draws_one_randperm_per_epoch(lib):
    import torch
    env, A, B, buf = prepared()
    tr = A.trainer()
    tr.compute(env, buf, **RETURNS)
    ga, gb = torch.Generator(device=DEV).manual_seed(21), torch.Generator(device=DEV).manual_seed(21)
    res = tr.train(buf, generator=ga)
    want = by_hand(B, buf, generator=gb)
    same_tensors(A.snapshot(), B.snapshot(), "seeded generator")
    check_result(res, want, "seeded generator")
    assert torch.equal(ga.get_state(), gb.get_state()), "train() drew more or less than the loop by hand"
    buf.detach()
    env.close()


def test_compute_equals_get_values_and_compute_returns(lib):
    import torch
    env, A, _, buf = prepared()
    next_value = A.pol.get_values(env, buf.rnn_states_critic[-1], buf.masks[-1], buffer=buf, row=-1)
    buf.compute_returns(next_value, A.vn, **RETURNS)
    want = [bits_of(buf.returns).copy(), bits_of(buf.value_preds).copy(), bits_of(next_value).copy()]
    assert np_(buf.returns).any()
    buf.returns.zero_()
    buf.value_preds[-1].zero_()
    got = A.trainer().compute(env, buf, **RETURNS)
    for a, b, what in zip((buf.returns, buf.value_preds, got), want, ("returns", "value_preds", "next_value")):
        np.testing.assert_array_equal(bits_of(a), b, what)
    buf.detach()
    env.close()


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(lib):
    from lsm.buffer import DeviceGraphBuffer
    env, A, B, buf = prepared()
    start = A.snapshot()
    with pytest.raises(policy.PolicyError, match="actor_opt must be"):
        DeviceTrainer(A.pol, A.loss, A.vn, B.aopt, B.copt, CFG)
    with pytest.raises(policy.PolicyError, match="critic_opt must be"):
        DeviceTrainer(A.pol, A.loss, A.vn, A.aopt, B.copt, CFG)
    args = types.SimpleNamespace(ppo_epoch=EPOCHS, num_mini_batch=MINIBATCHES, data_chunk_length=L,
                                 use_recurrent_policy=True, use_naive_recurrent_policy=True)
    with pytest.raises(TrainerError, match="naive_recurrent_generator raises"):
        TrainConfig.from_args(args)
    args.use_naive_recurrent_policy = False
    assert TrainConfig.from_args(args) == CFG
    with pytest.raises(TrainerError, match="the heads have an RNN"):
        A.trainer(CFG_FF)
    tr = A.trainer()
    with pytest.raises(TrainerError, match="train_info_host follows"):
        tr.train_info_host()
    tr.compute(env, buf, **RETURNS)
    with pytest.raises(TrainerError, match="permutations must hold ppo_epoch = 2"):
        tr.train(buf, permutations=permutations(T * 4 * 3 // L)[:1])
    buf.detach()
    bare = DeviceGraphBuffer(env, episode_length=T)
    with pytest.raises(TrainerError, match="no policy_rows"):
        tr.train(bare)
    same_tensors(A.snapshot(), start, "a refusal launched something")
    assert tr.last is None
    bare.detach()
    env.close()


# ---- no host read -----------------------------------------------------------------------------------------------

def test_train_makes_no_host_read(lib):
    """torch's sync debug mode raises on every synchronising torch call; it does not see ctypes calls, whose
    freedom from synchronisation rests on the units' own texts and tests."""
    import torch
    env, A, _, buf = prepared()
    tr = A.trainer()
    tr.compute(env, buf, **RETURNS)
    probe = torch.ones(1, device=DEV)
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            res = tr.train(buf, generator=torch.Generator(device=DEV).manual_seed(2))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not honour set_sync_debug_mode('error')")
    assert int(res["updates"]) == UPDATES and np.isfinite(np_(res["train_info"])).all()
    buf.detach()
    env.close()
