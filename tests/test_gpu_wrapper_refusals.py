"""GPU tests of what GraphEncoder, PolicyHead and PPOLoss do before and around their launches: the refusal of a
CPU tensor, a float64 tensor, a tensor one element short and a tensor on another device, each in the wrapper's
own error class and words; the output cache's policy seen from outside (eight row counts are kept, the ninth
empties it); and a non-contiguous input giving the bytes of its contiguous copy. M = 3 rows throughout."""
import numpy as np
import pytest

import gnn_model as gm
import policy_model as pm
from lsm import capi, gnn, policy
from lsm.loss import DeviceValueNorm, LossConfig, LossError, PPOLoss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, E, F = 3, 4, 7


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


class Wrappers:
    """The three wrappers and, per row count, a valid call of each: call[name](m, **replaced) passes the
    wrapper its inputs for m rows with the named ones replaced."""

    def __init__(self):
        import torch
        gcfg = gnn.GnnConfig(F=F)
        hcfg = policy.HeadConfig(kind="actor", in0=6, in1=16, hidden=64, num_actions=25, recurrent_N=1)
        self.encoder = gnn.GraphEncoder(gcfg, gm.default_weights(gcfg, 5)[1], DEV)
        self.head = policy.PolicyHead(hcfg, policy.pack_head_weights(pm.random_head_weights(hcfg, 11), hcfg), DEV)
        self.loss = PPOLoss(LossConfig(num_actions=25), DEV)
        self.vn = DeviceValueNorm(DEV)
        self.g = torch.Generator(device=DEV).manual_seed(3)
        self.call = {"encoder": self.encode, "forward": self.forward, "evaluate": self.evaluate, "loss": self.ppo}

    def rand(self, *shape):
        import torch
        return torch.rand(shape, generator=self.g, device=DEV)

    def encoder_inputs(self, m):
        import torch
        node = self.rand(m, E, F)
        node[:, :, F - 1] = torch.arange(E, device=DEV) % 4   # entity types
        return dict(node_obs=node, adj=self.rand(m, E, E) * (self.rand(m, E, E) < 0.5),
                    agent_id=torch.zeros(m, dtype=torch.int64, device=DEV))

    def head_inputs(self, m):
        import torch
        return dict(x0=self.rand(m, 6), x1=self.rand(m, 16), rnn_states=self.rand(m, 1, 64),
                    masks=torch.ones((m, 1), device=DEV))

    def loss_inputs(self, m):
        import torch
        return dict(logits=self.rand(m, 25), values=self.rand(m, 1),
                    actions=torch.arange(m, device=DEV).float().view(m, 1) % 25, old_log_probs=-self.rand(m, 1) - 2.0,
                    advantages=self.rand(m, 1) - 0.5, value_preds=self.rand(m, 1), returns=self.rand(m, 1),
                    active_masks=torch.ones((m, 1), device=DEV))

    def encode(self, m, **over):
        return self.encoder.forward(**{**self.encoder_inputs(m), **over})

    def forward(self, m, **over):
        return self.head.forward(**{**self.head_inputs(m), "u": self.rand(m), **over})

    def evaluate(self, m, **over):
        import torch
        acts = torch.arange(m, device=DEV).float().view(m, 1) % 25
        return self.head.evaluate(**{**self.head_inputs(m), "T": 1, "actions": acts, **over})

    def ppo(self, m, **over):
        return self.loss.forward(**{**self.loss_inputs(m), "value_norm": self.vn, **over})


@pytest.fixture(scope="module")
def w(lib):
    return Wrappers()


def _valid(w, name, arg):
    inputs = {"encoder": w.encoder_inputs, "loss": w.loss_inputs}.get(name, w.head_inputs)(M)
    return dict(inputs, actions=inputs.get("actions", w.rand(M, 1)))[arg]


# (the call, the argument replaced, its valid shape, the wrapper's noun, whether the size is named as a shape)
ARGS = [("encoder", "adj", (M, E, E), "encoder", True),
        ("forward", "x0", (M, 6), "head", False), ("forward", "rnn_states", (M, 1, 64), "head", False),
        ("evaluate", "x0", (M, 6), "head", False), ("evaluate", "actions", (M, 1), "head", False),
        ("loss", "advantages", (M, 1), "loss", False), ("loss", "value_preds", (M, 1), "loss", False)]
ERRORS = {"encoder": gnn.GnnError, "forward": policy.PolicyError, "evaluate": policy.PolicyError, "loss": LossError}
IDS = ["%s-%s" % a[:2] for a in ARGS]


def _refused(w, name, arg, tensor, text):
    with pytest.raises(ERRORS[name]) as e:
        w.call[name](M, **{arg: tensor})
    assert type(e.value) is ERRORS[name] and str(e.value) == text


@pytest.mark.parametrize("name, arg, shape, noun, shaped", ARGS, ids=IDS)
def test_a_cpu_tensor_is_refused(w, name, arg, shape, noun, shaped):
    _refused(w, name, arg, _valid(w, name, arg).cpu(), "%s must be a CUDA (HIP) tensor; there is no CPU fallback" % arg)


@pytest.mark.parametrize("name, arg, shape, noun, shaped", ARGS, ids=IDS)
def test_a_float64_tensor_is_refused(w, name, arg, shape, noun, shaped):
    n = int(np.prod(shape))
    text = ("%s must be torch.float32 %s, got torch.float64 %s" % (arg, shape, shape) if shaped else
            "%s must hold %d float32 values, got torch.float64 %s" % (arg, n, shape))
    _refused(w, name, arg, _valid(w, name, arg).double(), text)


@pytest.mark.parametrize("name, arg, shape, noun, shaped", ARGS, ids=IDS)
def test_a_tensor_one_element_short_is_refused(w, name, arg, shape, noun, shaped):
    n = int(np.prod(shape))
    text = ("%s must be torch.float32 %s, got torch.float32 (%d,)" % (arg, shape, n - 1) if shaped else
            "%s must hold %d float32 values, got torch.float32 (%d,)" % (arg, n, n - 1))
    _refused(w, name, arg, _valid(w, name, arg).reshape(-1)[:n - 1], text)


@pytest.mark.parametrize("name, arg, shape, noun, shaped", ARGS, ids=IDS)
def test_a_tensor_on_another_device_is_refused(w, name, arg, shape, noun, shaped):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device only")
    _refused(w, name, arg, _valid(w, name, arg).to("cuda:1"), "%s is on cuda:1, the %s on cuda:0" % (arg, noun))


def test_the_literal_words_of_one_refusal_per_wrapper(w):
    """The texts above are put together from the argument's name and shape; these five are spelled out."""
    _refused(w, "encoder", "adj", w.rand(M, E, E).double(),
             "adj must be torch.float32 (3, 4, 4), got torch.float64 (3, 4, 4)")
    _refused(w, "encoder", "node_obs", w.rand(M, E, F).cpu(),
             "node_obs must be a CUDA (HIP) tensor; there is no CPU fallback")
    _refused(w, "forward", "x0", w.rand(17), "x0 must hold 18 float32 values, got torch.float32 (17,)")
    _refused(w, "evaluate", "masks", w.rand(M, 1).cpu(), "masks must be a CUDA (HIP) tensor; there is no CPU fallback")
    _refused(w, "loss", "logits", w.rand(M, 25).double(),
             "logits must hold 75 float32 values, got torch.float64 (3, 25)")


@pytest.mark.parametrize("name, key", [("encoder", None), ("forward", "features"), ("evaluate", "features"),
                                       ("loss", "dlogits")])
def test_eight_row_counts_are_cached_and_the_ninth_empties_the_cache(lib, name, key):
    """Row counts 1 .. 9 on one stream: after eight the first call's output is still the cached object, after
    the ninth it is not, and the ninth's is."""
    call = Wrappers().call[name]   # fresh wrappers: nothing is cached yet
    pick = (lambda out: out) if key is None else (lambda out: out[key])
    outs = [pick(call(m)) for m in range(1, 9)]
    for m in (8, 1):
        assert pick(call(m)) is outs[m - 1]
    ninth = pick(call(9))
    assert tuple(ninth.shape)[0] == 9
    assert pick(call(9)) is ninth
    again = pick(call(1))
    assert again is not outs[0] and tuple(again.shape) == tuple(outs[0].shape)
    assert pick(call(9)) is ninth and pick(call(1)) is again


def test_a_non_contiguous_input_gives_the_bytes_of_its_contiguous_copy(w):
    import torch
    x1 = w.rand(M, 32)[:, ::2]
    adj = (w.rand(M, E, 2 * E) * (w.rand(M, E, 2 * E) < 0.5))[:, :, ::2]
    logits = w.rand(M, 50)[:, ::2]
    assert not (x1.is_contiguous() or adj.is_contiguous() or logits.is_contiguous())
    u = w.rand(M)
    hin, ein, lin = w.head_inputs(M), w.encoder_inputs(M), w.loss_inputs(M)
    acts = torch.tensor([[4.0], [0.0], [24.0]], device=DEV)
    state0 = w.vn.state.clone()

    def ppo(lg):
        w.vn.state.copy_(state0)
        return w.loss.forward(**dict(lin, logits=lg, value_norm=w.vn))

    calls = {"forward": lambda t: w.head.forward(**dict(hin, x1=t, u=u)),
             "evaluate": lambda t: w.head.evaluate(**dict(hin, x1=t, T=1, actions=acts)),
             "encoder": lambda t: {"out": w.encoder.forward(**dict(ein, adj=t))}, "loss": ppo}
    for name, t in (("forward", x1), ("evaluate", x1), ("encoder", adj), ("loss", logits)):
        got = {k: v.clone() for k, v in calls[name](t).items() if not k.startswith("_")}
        want = calls[name](t.contiguous())
        assert sorted(got) == sorted(k for k in want if not k.startswith("_"))
        for k, v in got.items():
            assert v.shape == want[k].shape and v.dtype == want[k].dtype
            assert v.cpu().numpy().tobytes() == want[k].cpu().numpy().tobytes(), (name, k)
