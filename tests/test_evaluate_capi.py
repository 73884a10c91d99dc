"""CPU tests of the heads' sequence form (include/lsm_evaluate.h): the header and its exports, the float64
model pinned against torch.nn modules in double and against fixtures recorded from the reference's own
MLPBase / RNNLayer / ACTLayer (tests/golden/evaluate/), lsm_host_head_evaluate -- the per-chunk text the
kernel runs -- against tests/evaluate_model.py within the tolerance measured per case and output tensor
(4 * e32 + 4 * 2^-23 * s), masks, availability, active masks, NaN features, bad actions, T = 1 against
lsm_head_forward, and the argument refusals (which return before any launch or write, so they need no
device)."""
import dataclasses
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import evaluate_cases as ec
import evaluate_model as em
import policy_model as pm
from lsm import capi, policy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_evaluate.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "evaluate")


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
    assert declared == set(capi.EXPORTED_EVALUATE) and len(declared) == 3
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY):
        assert not declared & set(other)
    assert "lsm_evaluate.hip" in build.UNITS and "lsm_head_tile.h" in build.UNITS["lsm_policy.hip"]
    body = hdr[hdr.index("typedef struct lsm_eval_io"):hdr.index("} lsm_eval_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmEvalIo._fields_]


def test_the_two_kernels_share_one_text(lib):
    """The per-row pieces live in csrc/lsm_head_tile.h alone; the rollout's build id does not cover them."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_evaluate.hip", "lsm_evaluate.h", "lsm_head_tile.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    shared = open(os.path.join(build.CSRC, "lsm_head_tile.h")).read()
    for unit in ("lsm_policy.hip", "lsm_evaluate.hip", "lsm_backward.hip"):
        src = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "lsm_head_tile.h"' in src and "lsm_rollout.h" not in src
        for piece in ("void dot4(", "void linear(", "void layer_norm(", "void gru_layer(", "void masked_softmax(",
                      "void save_rows(", "void load_rows(", "void mlp(", "Tile block_tile("):
            assert piece in shared and piece not in src, (unit, piece)
        # every unit runs the shared MLP, GRU cell and kernel entry, and none writes its own again
        for call in ("mlp(n, w, ", "gru_layer(n, w, ", "block_tile(n.", "load_inputs(n, "):
            assert call in src, (unit, call)
        for text in ("gru_layer_save", "sigmoid_(", "readfirstlane"):
            assert text not in src, (unit, text)
    # the one-step kernel and the backward's stage 1 copy their rows through the shared loops; eval_tile and
    # bwd_tile's gradient stores keep their own (eval_kernel and bwd_kernel are kept byte-identical)
    for unit in ("lsm_policy.hip", "lsm_backward.hip"):
        src = open(os.path.join(build.CSRC, unit)).read()
        assert "load_rows(" in src and "save_rows(" in src, unit


def test_scratch_bytes(lib):
    f = lib.lsm_head_evaluate_scratch_bytes
    assert f(-1, 1) == 0 and f(1, 0) == 0
    assert f(0, 1) == 16 and f(1, 5) == 16 and f(64, 1) == 16 and f(65, 1) == 32 and f(129, 2) == 48


# ---- the yardstick itself -----------------------------------------------------------------------------------

def _pin_case(name):
    if name.startswith("option "):
        return ec.option_case(name[len("option "):])
    return {"actor": lambda: ec.shape_case("actor", 65, 10), "critic": lambda: ec.shape_case("critic", 65, 10),
            "masks actor": lambda: ec.masks_case("actor"), "masks critic": lambda: ec.masks_case("critic"),
            "avail": lambda: ec.avail_case("some"), "nan": ec.nan_case}[name]()


@pytest.mark.parametrize("name", ["actor", "critic", "masks actor", "masks critic", "avail", "nan",
                                  "option recurrent_N 0", "option tanh", "option no feature norm",
                                  "option critic x0 null"])
def test_model64_agrees_with_torch_modules_in_double(name):
    """model64 is written out from the header's formulas; the same network from nn.Linear / nn.LayerNorm /
    nn.GRU (one step per call, h * masks[l] before each) and Categorical.log_prob / .entropy() cast to double
    agrees to about 1e-12 relative, so the yardstick does not depend on the code under test. Categorical is
    compared on rows with at least one available action."""
    case = _pin_case(name)
    ref = em.model64_torch(case.cfg, case.sd, case.inp, case.C, case.T)
    for k, v in ref.items():
        mine = case.w64[k]
        sel = np.ones(mine.shape, bool)
        if k == "logits":
            sel = case.fin
        elif k == "log_probs":
            sel = case.some & ~case.unavail
        elif k == "entropy":
            sel = case.some
        scale = max(1.0, float(np.abs(mine[sel]).max()))
        err = float(np.abs(v - mine)[sel].max())
        print("pin %s %s: %.3e" % (name, k, err / scale))
        assert err <= 1e-11 * scale, (name, k, err)
    if case.cfg.kind == "actor":
        want = em.dist_entropy(np.where(case.some, ref["entropy"], case.w64["entropy"]), case.inp.get("active"))
        assert abs(want - case.w64["dist_entropy"]) <= 1e-11


def _fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def test_the_reference_fixtures_are_there():
    assert _fixtures() == ["t4_c3_rn1", "t4_c3_rn2"]


@pytest.mark.parametrize("name", ["t4_c3_rn1", "t4_c3_rn2"])
def test_model64_reproduces_the_reference(name):
    """The reference's own MLPBase, RNNLayer (T x N branch) and ACTLayer.evaluate_actions in float64
    (tests/golden/make_evaluate_golden.py): model64 agrees to 1e-12 on the features (NaN zeroed), the final
    states, the log-probabilities and dist_entropy."""
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    cfg = policy.HeadConfig(kind="actor", in0=int(z["in0"]), in1=int(z["in1"]), hidden=int(z["hidden"]),
                            layer_N=int(z["layer_N"]), relu=bool(z["relu"]), feature_norm=bool(z["feature_norm"]),
                            recurrent_N=int(z["recurrent_N"]), num_actions=int(z["num_actions"]))
    Cn, T = int(z["C"]), int(z["T"])
    sd = {k[2:]: v for k, v in z.items() if k.startswith("w_")}
    assert set(sd) == {n for n, _ in policy.head_weight_entries(cfg)}
    inp = {k: z[k] for k in ("x0", "x1", "states", "masks", "actions", "avail", "active")}
    mk = inp["masks"].reshape(T, Cn)
    assert (mk[0] == 0).any() and (mk[1:] == 0).any() and (inp["avail"] == 0).any() and (inp["active"] == 0).any()
    assert np.isnan(inp["x1"]).sum() == 1 and cfg.recurrent_N == (2 if name.endswith("rn2") else 1)
    got = em.model64(cfg, sd, inp, Cn, T)
    assert not np.isnan(z["features"]).any() and (z["features"][(T - 1) * Cn + 1] == 0).all()
    for k in ("features", "rnn_out", "log_probs"):
        assert got[k].shape == z[k].shape, k
        np.testing.assert_allclose(got[k], z[k], rtol=0, atol=1e-12, equal_nan=True, err_msg=k)
    assert np.isnan(z["rnn_out"][1]).all() and not np.isnan(z["rnn_out"][[0, 2]]).any()
    assert abs(got["dist_entropy"] - float(z["dist_entropy"])) <= 1e-12


# ---- parity of the host entry point -----------------------------------------------------------------------

@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "C%d-T%d" % s)
@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_host_shapes(lib, kind, shape):
    ec.check(lib, ec.shape_case(kind, *shape))


@pytest.mark.parametrize("name", sorted(ec.OPTIONS))
def test_host_options(lib, name):
    ec.check(lib, ec.option_case(name))


@pytest.mark.parametrize("name", sorted(ec.PLAN_OPTIONS))
def test_host_plan_cases(lib, name):
    """One case per size limit and width class (evaluate_cases.PLAN_OPTIONS, the limits found through
    lsm_head_plan); past an LDS limit the call is refused and writes nothing."""
    ec.plan_checks(lib, name, None)


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_host_masked_state_does_not_leak(lib, kind):
    ec.masks_checks(lib, kind, None)


def test_host_available_actions_and_active_masks(lib):
    ec.avail_checks(lib, None)


def test_host_nan_features_are_read_as_zero(lib):
    ec.nan_checks(lib, None)


def test_host_bad_actions(lib):
    ec.bad_action_checks(lib, None)


def test_host_single_step_agrees_with_the_forward(lib):
    ec.t1_checks(lib, None)


def test_host_same_call_twice_and_null_outputs(lib):
    ec.twice_and_null_checks(lib, None)


def test_empty_minibatch_is_legal(lib):
    for kind in ("actor", "critic"):
        case = ec.shape_case(kind, 1, 3)
        inp = {k: (v[:0] if v is not None else None) for k, v in case.inp.items()}
        got, bad = ec.run(lib, case.cfg, case.blob, inp, 0, 3)
        assert got == {} and bad == 0


# ---- argument refusals: nonzero and a text, before any launch or write -------------------------------------

REFUSALS = {
    "null weights": dict(over=dict(weights=None)),
    "null io": dict(over=dict(io=None)),
    "null x0": dict(over=dict(x0=None)),
    "null x1": dict(over=dict(x1=None)),
    "null actions": dict(over=dict(actions=None)),
    "misaligned x1": dict(add=dict(x1=2)),
    "misaligned weights": dict(add=dict(weights=1)),
    "misaligned actions": dict(add=dict(actions=2)),
    "misaligned entropy": dict(add=dict(entropy=2)),
    "misaligned bad": dict(add=dict(bad=4)),
    "misaligned scratch": dict(add=dict(scratch=4)),
    "dist_entropy without scratch": dict(over=dict(scratch=None)),
    "T = 0": dict(over=dict(T=0)),
    "T < 0": dict(over=dict(T=-2)),
    "C < 0": dict(over=dict(C=-1)),
    "T * C = 2^31": dict(over=dict(C=2 ** 30, T=2)),
    "in0 < 0": dict(cfg=dict(in0=-1)),
    "in = 0": dict(cfg=dict(in0=0, in1=0)),
    "in = 257": dict(cfg=dict(in0=241)),
    "hidden = 0": dict(cfg=dict(hidden=0)),
    "hidden = 129": dict(cfg=dict(hidden=129)),
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
    "actor with every output null": dict(over={k: None for k in ec.ACTOR_OUT}),
    "LDS: hidden 128, recurrent_N 2, in 250": dict(cfg=dict(hidden=128, recurrent_N=2, in0=234), match="LDS"),
}


def _refusal_case():
    return ec.shape_case("actor", 5, 2)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(lib, what):
    spec = REFUSALS[what]
    case = _refusal_case()
    cfg = dataclasses.replace(case.cfg, **spec.get("cfg", {}))
    over = dict(spec.get("over", {}))
    if "struct" in spec:
        st = cfg.struct()
        for k, v in spec["struct"].items():
            setattr(st, k, v)
        over["cfg"] = st
    blob = np.zeros(300000, np.float32)
    ec.run(lib, cfg, blob, case.inp, case.C, case.T, expect_rc=1, bad_init=3, over=over, add=spec.get("add"),
           alias=spec.get("alias"))
    if "match" in spec:
        assert spec["match"] in lib.lsm_policy_last_error().decode()


def test_refusal_case_is_accepted_unchanged(lib):
    """The refusal tests' call succeeds without its one change (so each refusal is due to that change)."""
    case = _refusal_case()
    ec.run(lib, case.cfg, np.zeros(300000, np.float32), case.inp, case.C, case.T)
    ec.check(lib, case)


def test_the_lds_refusal_names_the_need_and_spares_the_defaults(lib):
    """hidden 128, recurrent_N 2, in 250 needs 200704 bytes for a 64-chunk tile and is refused with that
    figure; the reference's hidden 64, recurrent_N 1 fits at the widest input, 256, and runs."""
    wide = dataclasses.replace(ec.ACTOR, hidden=128, recurrent_N=2, in0=234)
    case = _refusal_case()
    ec.run(lib, wide, np.zeros(300000, np.float32), case.inp, case.C, case.T, expect_rc=1)
    err = lib.lsm_policy_last_error().decode()
    assert "200704" in err and "163840" in err, err
    assert policy.head_weights_floats(wide) > 0            # lsm_head_forward still takes this config
    cfg = dataclasses.replace(ec.ACTOR, in0=240)
    assert cfg.in0 + cfg.in1 == 256 and cfg.hidden == 64 and cfg.recurrent_N == 1
    ec.check(lib, ec.Case("in 256", cfg, 3, 2, seed=2))


def test_fields_of_the_other_kind_are_not_checked(lib):
    """A critic ignores the actor's fields of lsm_eval_io (and an actor `values`): misaligned garbage there
    is neither refused nor touched, and the outputs are the same bytes; without an RNN the state fields are
    ignored too."""
    junk = dict(actions=2, available_actions=6, active_masks=2, log_probs=5, entropy=3, dist_entropy=1, logits=7,
                scratch=2)
    for kind, over in (("critic", junk), ("actor", dict(values=2))):
        case = ec.shape_case(kind, 5, 2) if kind == "actor" else ec.shape_case(kind, 1, 3)
        clean, _ = ec.run(lib, case.cfg, case.blob, case.inp, case.C, case.T)
        got, bad = ec.run(lib, case.cfg, case.blob, case.inp, case.C, case.T, over=over)
        assert bad == 0
        ec.same_bytes(got, clean, kind)
    case = ec.option_case("critic recurrent_N 0")
    ec.run(lib, case.cfg, case.blob, case.inp, case.C, case.T, over=dict(rnn_states=2, masks=2, rnn_out=2))
