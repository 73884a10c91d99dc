"""CPU tests of the policy-head ABI (include/lsm_policy.h): the header and its exports, the weight blob's
packing, the float64 model pinned against torch.nn modules in double, lsm_host_head_forward -- the per-row
text the kernel runs -- against tests/policy_model.py within the tolerance measured per case and output
tensor (4 * e32 + 4 * 2^-23 * s), the sampler's discrete outputs (tests/policy_cases.py: exact on decidable
rows), bad uniforms, and the argument refusals (which return before any launch or write, so they need no
device)."""
import dataclasses
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

import policy_abi as pa
import policy_cases as pc
import policy_model as pm
from lsm import capi, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_policy.h")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    from lsm import build
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_POLICY) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN):
        assert not declared & set(other)
    assert "lsm_policy.hip" in build.UNITS
    body = hdr[hdr.index("typedef struct lsm_head_config"):hdr.index("} lsm_head_config")]
    assert re.findall(r"int32_t\s+(\w+);", body) == [f for f, _ in capi.LsmHeadConfig._fields_]
    body = hdr[hdr.index("typedef struct lsm_head_io"):hdr.index("} lsm_head_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmHeadIo._fields_]


def test_build_id_is_unchanged_by_the_unit(lib):
    """The rollout's build id covers the step kernels, the host ABI and lsm_rollout.h only."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert "lsm_policy.hip" not in deps and "lsm_policy.h" not in deps
    assert lib.lsm_build_id().decode() == build.build_id()
    src = open(os.path.join(build.CSRC, "lsm_policy.hip")).read()
    assert "lsm_rollout.h" not in src and "lsm_policy.h" in src


# ---- the yardstick itself -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["actor", "critic", "option recurrent_N 2", "option tanh", "option no feature norm",
                                  "option critic x0 null", "avail"])
def test_model64_agrees_with_torch_modules_in_double(name):
    """model64 is written out from the header's formulas; the same network from nn.Linear / nn.LayerNorm /
    nn.GRU / log_softmax cast to double agrees to about 1e-12 relative, so the yardstick does not depend
    on the code under test."""
    case = (pc.shape_case(name, 65) if name in ("actor", "critic") else pc.avail_case() if name == "avail"
            else pc.option_case(name[len("option "):]))
    ref = pm.model64_torch(case.cfg, case.sd, case.inp)
    for k, v in ref.items():
        mine = case.w64[k]
        sel = pm.finite_logits(mine) if k in ("logits", "logp") else np.ones(mine.shape, bool)
        scale = max(1.0, float(np.abs(mine[sel]).max()))
        err = float(np.abs(v - mine)[sel].max())
        print("pin %s %s: %.3e" % (name, k, err / scale))
        assert err <= 1e-11 * scale, (name, k, err)
    if "logits" in ref:
        np.testing.assert_array_equal(ref["logits"][~case.fin], case.w64["logits"][~case.fin])


# ---- the weight blob ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["actor", "critic"] + sorted(pc.OPTIONS))
def test_pack_unpack_round_trip(lib, name):
    cfg = pc.ACTOR if name == "actor" else pc.CRITIC if name == "critic" else pc.option_case(name).cfg
    sd = pm.random_head_weights(cfg, 4)
    assert "base.mlp.fc_h.0.weight" in sd                     # the unused template: ignored
    sd["gnn_base.gnn1.lin_key.weight"] = np.zeros((2, 2), np.float32)
    blob = policy.pack_head_weights(sd, cfg)
    assert blob.dtype == np.float32 and blob.shape == (int(lib.lsm_head_weights_floats(cfg.struct())),)
    assert blob.size == sum(int(np.prod(s)) for _, s in policy.head_weight_entries(cfg))
    back = policy.unpack_head_weights(blob, cfg)
    names = dict(policy.head_weight_entries(cfg))
    want = {k: v for k, v in sd.items() if k in names}
    assert set(back) == set(want)
    for k in want:
        np.testing.assert_array_equal(back[k], want[k], err_msg=k)
    # the documented order: the feature norm first (1 / 0 when it is off), the output bias last
    n = cfg.in0 + cfg.in1
    if cfg.feature_norm:
        np.testing.assert_array_equal(blob[:n], sd["base.feature_norm.weight"])
    else:
        assert (blob[:n] == 1).all() and (blob[n:2 * n] == 0).all()
    last = "act.action_out.linear.bias" if cfg.kind == "actor" else "v_out.bias"
    np.testing.assert_array_equal(blob[-cfg.out_rows:], sd[last])
    # torch tensors and a prefix
    import torch
    tsd = {"actor." + k: torch.from_numpy(v) for k, v in want.items()}
    np.testing.assert_array_equal(policy.pack_head_weights(tsd, cfg, prefix="actor."), blob)


def test_pack_refuses_missing_and_misshaped_by_name(lib):
    cfg = pc.ACTOR
    sd = pm.random_head_weights(cfg, 4)
    for key in ("rnn.rnn.bias_hh_l0", "base.feature_norm.bias", "base.mlp.fc2.0.2.weight", "act.action_out.linear.weight"):
        short = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(policy.PolicyError, match=re.escape(key)):
            policy.pack_head_weights(short, cfg)
    for key in ("base.mlp.fc1.0.weight", "rnn.rnn.weight_ih_l0", "rnn.norm.bias"):
        wrong = dict(sd)
        wrong[key] = np.zeros(tuple(s + 1 for s in sd[key].shape), np.float32)
        with pytest.raises(policy.PolicyError, match=re.escape(key)):
            policy.pack_head_weights(wrong, cfg)
    with pytest.raises(policy.PolicyError, match=re.escape("v_out.weight")):
        policy.pack_head_weights(sd, dataclasses.replace(pc.CRITIC, in0=pc.OBS))
    with pytest.raises(policy.PolicyError, match=re.escape("base.feature_norm.weight")):
        policy.pack_head_weights(sd, dataclasses.replace(cfg, in0=7))
    with pytest.raises(policy.PolicyError):
        policy.unpack_head_weights(np.zeros(7, np.float32), cfg)


def test_from_args_reads_the_reference_names():
    a = types.SimpleNamespace(hidden_size=64, layer_N=1, use_ReLU=True, use_feature_normalization=True, recurrent_N=1,
                              use_recurrent_policy=True, use_naive_recurrent_policy=False)
    assert policy.HeadConfig.from_args(a, "actor", 6, 16, num_actions=25) == pc.ACTOR
    assert policy.HeadConfig.from_args(a, "critic", 48, 16) == pc.CRITIC
    a.use_recurrent_policy = False
    assert policy.HeadConfig.from_args(a, "critic", 48, 16).recurrent_N == 0
    a.use_naive_recurrent_policy = True
    assert policy.HeadConfig.from_args(a, "critic", 48, 16).recurrent_N == 1
    with pytest.raises(ValueError):
        dataclasses.replace(pc.ACTOR, kind="both").struct()
    with pytest.raises(ValueError):
        dataclasses.replace(pc.ACTOR, num_actions=None).struct()


def test_weights_floats_is_zero_for_a_refused_config(lib):
    assert lib.lsm_head_weights_floats(dataclasses.replace(pc.ACTOR, hidden=129).struct()) == 0
    assert lib.lsm_policy_last_error().decode().startswith("head: ")
    with pytest.raises(policy.PolicyError, match="head: "):
        policy.head_weights_floats(dataclasses.replace(pc.CRITIC, layer_N=5))


# ---- parity of the host entry point -----------------------------------------------------------------------

@pytest.mark.parametrize("M", pc.SHAPE_M)
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_host_shapes(lib, kind, M):
    pc.check(lib, pc.shape_case(kind, M))


@pytest.mark.parametrize("name", sorted(pc.OPTIONS))
def test_host_options(lib, name):
    pc.check(lib, pc.option_case(name))


@pytest.mark.parametrize("name", sorted(pc.PLAN_OPTIONS))
def test_host_plan_cases(lib, name):
    """The forward's largest tile (in 256, hidden 128) and its narrowest input row (in0 + in1 = 1)."""
    pc.check(lib, pc.plan_case(name))


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_host_masked_state_does_not_leak(lib, kind):
    pc.masks_checks(lib, kind, None)


def test_host_available_actions(lib):
    pc.avail_checks(lib, None)


def test_host_stratified_sampler(lib):
    pc.stratified_checks(lib, None)


def test_host_same_call_twice_and_null_outputs(lib):
    pc.twice_and_null_checks(lib, None)


def test_host_bad_uniforms(lib):
    pc.bad_u_checks(lib, None)


def test_empty_batch_is_legal(lib):
    for cfg in (pc.ACTOR, pc.CRITIC):
        case = pc.shape_case(cfg.kind, 1)
        inp = {k: (v[:0] if v is not None else None) for k, v in case.inp.items()}
        got, bad = pa.run(lib, cfg, case.blob, inp)
        assert got == {} and bad == 0


# ---- argument refusals: nonzero and a text, before any launch or write -------------------------------------

REFUSALS = {
    "null weights": dict(over=dict(weights=None)),
    "null io": dict(over=dict(io=None)),
    "null x0": dict(over=dict(x0=None)),
    "null x1": dict(over=dict(x1=None)),
    "misaligned x1": dict(add=dict(x1=2)),
    "misaligned weights": dict(add=dict(weights=1)),
    "misaligned features": dict(add=dict(features=2)),
    "misaligned bad": dict(add=dict(bad=4)),
    "M < 0": dict(over=dict(M=-1)),
    "M = 2^31": dict(over=dict(M=2 ** 31)),
    "in0 < 0": dict(cfg=dict(in0=-1)),
    "in1 < 0": dict(cfg=dict(in1=-1, in0=40)),
    "in = 0": dict(cfg=dict(in0=0, in1=0)),
    "in = 257": dict(cfg=dict(in0=241)),
    "hidden = 0": dict(cfg=dict(hidden=0)),
    "hidden = 129": dict(cfg=dict(hidden=129)),
    "layer_N = -1": dict(cfg=dict(layer_N=-1)),
    "layer_N = 5": dict(cfg=dict(layer_N=5)),
    "recurrent_N = -1": dict(cfg=dict(recurrent_N=-1)),
    "recurrent_N = 3": dict(cfg=dict(recurrent_N=3)),
    "num_actions = 0": dict(cfg=dict(num_actions=0)),
    "num_actions = 65": dict(cfg=dict(num_actions=65)),
    "unknown kind": dict(struct=dict(kind=2)),
    "rnn_out overlaps rnn_states": dict(alias=("rnn_out", "rnn_states", 0)),
    "rnn_out overlaps the end of rnn_states": dict(alias=("rnn_out", "rnn_states", 4 * (5 * 64 - 1))),
    "recurrent without rnn_states": dict(over=dict(rnn_states=None)),
    "recurrent without masks": dict(over=dict(masks=None)),
    "actor with neither action output": dict(over=dict(actions_i32=None, actions_f32=None)),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(lib, what):
    spec = REFUSALS[what]
    case = pc.shape_case("actor", 5)
    cfg = dataclasses.replace(case.cfg, **spec.get("cfg", {}))
    over = dict(spec.get("over", {}))
    if "struct" in spec:
        st = cfg.struct()
        for k, v in spec["struct"].items():
            setattr(st, k, v)
        over["cfg"] = st
    blob = np.zeros(80000, np.float32)
    pa.run(lib, cfg, blob, case.inp, expect_rc=1, bad_init=3, over=over, add=spec.get("add"), alias=spec.get("alias"))


def test_refusal_shape_case_is_accepted_unchanged(lib):
    """The refusal tests' call succeeds without its one change (so each refusal is due to that change)."""
    case = pc.shape_case("actor", 5)
    pa.run(lib, case.cfg, np.zeros(80000, np.float32), case.inp)
    pc.check(lib, case)


def test_fields_of_the_other_kind_are_not_checked(lib):
    """A critic ignores the actor's fields of lsm_head_io (and an actor `values`): misaligned garbage there
    is neither refused nor touched, and the outputs are the same bytes."""
    for kind, junk in (("critic", dict(u=2, available_actions=6, actions_i32=1, actions_f32=3, log_probs=5, logits=7)),
                       ("actor", dict(values=2))):
        case = pc.shape_case(kind, 5)
        clean, _ = pa.run(lib, case.cfg, case.blob, case.inp)
        got, bad = pa.run(lib, case.cfg, case.blob, case.inp, over=junk)
        assert bad == 0 and set(got) == set(clean)
        for k in clean:
            np.testing.assert_array_equal(got[k].view(np.int32), clean[k].view(np.int32), err_msg=k)
    # without an RNN the state fields are ignored too
    case = pc.option_case("critic recurrent_N 0")
    pa.run(lib, case.cfg, case.blob, case.inp, over=dict(rnn_states=2, masks=2, rnn_out=2))
