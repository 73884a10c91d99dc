"""CPU tests of the graph-encoder ABI (include/lsm_gnn.h): the header and its exports, the weight blob's
packing, lsm_host_gnn_forward -- the per-graph text the kernel runs -- against tests/gnn_model.py within
the tolerance measured per case (4 * e32 + 4 * 2^-23 * s, see gnn_model), bad inputs, and the argument
refusals (which return before any launch or write, so they need no device)."""
import ctypes as C
import dataclasses
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gnn_abi as ga
import gnn_cases as gc
import gnn_model as gm
from lsm import capi, gnn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_gnn.h")


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
    assert declared == set(capi.EXPORTED_GNN) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES):
        assert not declared & set(other)
    assert "lsm_gnn.hip" in build.UNITS
    body = hdr[hdr.index("typedef struct lsm_gnn_config"):hdr.index("} lsm_gnn_config")]
    for field, _ in capi.LsmGnnConfig._fields_:
        assert re.search(r"\b%s\b" % field, body), field
    assert len(re.findall(r"int32_t\s+\w+;", body)) == len(capi.LsmGnnConfig._fields_)


def test_build_id_is_unchanged_by_the_unit(lib):
    """The rollout's build id covers the step kernels, the host ABI and lsm_rollout.h only."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert "lsm_gnn.hip" not in deps and "lsm_gnn.h" not in deps
    assert lib.lsm_build_id().decode() == build.build_id()
    src = open(os.path.join(build.CSRC, "lsm_gnn.hip")).read()
    assert "lsm_rollout.h" not in src and "lsm_gnn.h" in src


# ---- the weight blob ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["default"] + sorted(gc.OPTIONS))
def test_pack_unpack_round_trip(lib, name):
    cfg = dataclasses.replace(gc.DEFAULT, **gc.OPTIONS.get(name, {}))
    sd = gm.random_weights(cfg, 4)
    sd["gnn.embed_layer.layers.2.weight"] = np.zeros(3, np.float32)    # the shared layer norm's aliases: ignored
    sd["actor.fc.weight"] = np.zeros((2, 2), np.float32)
    blob = gnn.pack_weights(sd, cfg)
    assert blob.dtype == np.float32 and blob.shape == (int(lib.lsm_gnn_weights_floats(cfg.struct())),)
    back = gnn.unpack_weights(blob, cfg)
    want = {k: v for k, v in sd.items() if k[4:] in dict(gnn.weight_entries(cfg)) and k.startswith("gnn.")}
    assert set(back) == set(want)
    for k in want:
        np.testing.assert_array_equal(back[k], want[k], err_msg=k)
    # the documented order: the embedding table first, the last conv's skip bias last
    np.testing.assert_array_equal(blob[:cfg.num_embeddings * cfg.embedding_size],
                                  sd["gnn.embed_layer.entity_embed.weight"].reshape(-1))
    last = "gnn1" if cfg.layer_N == 0 else "gnn2.%d" % (cfg.layer_N - 1)
    np.testing.assert_array_equal(blob[-cfg.out_dim:], sd["gnn.%s.lin_skip.bias" % last])
    # torch tensors and another prefix
    import torch
    tsd = {"enc." + k[4:]: torch.from_numpy(v) for k, v in want.items()}
    np.testing.assert_array_equal(gnn.pack_weights(tsd, cfg, prefix="enc."), blob)


def test_pack_refuses_missing_and_misshaped_by_name(lib):
    cfg = gc.DEFAULT
    sd = gm.random_weights(cfg, 4)
    for key in ("gnn.gnn2.1.lin_edge.weight", "gnn.embed_layer.layer_norm.bias", "gnn.embed_layer.layers.0.weight"):
        short = {k: v for k, v in sd.items() if k != key}
        with pytest.raises(gnn.GnnError, match=re.escape(key)):
            gnn.pack_weights(short, cfg)
    for key in ("gnn.gnn1.lin_query.weight", "gnn.embed_layer.lin1.weight", "gnn.gnn2.0.lin_skip.bias"):
        wrong = dict(sd)
        wrong[key] = np.zeros(tuple(s + 1 for s in sd[key].shape), np.float32)
        with pytest.raises(gnn.GnnError, match=re.escape(key)):
            gnn.pack_weights(wrong, cfg)
    # a config with other sizes refuses the same state dict by the first entry that differs
    with pytest.raises(gnn.GnnError, match="lin1.weight"):
        gnn.pack_weights(sd, dataclasses.replace(cfg, F=10))
    with pytest.raises(gnn.GnnError):
        gnn.unpack_weights(np.zeros(7, np.float32), cfg)


def test_from_args_reads_the_reference_names():
    import types
    a = types.SimpleNamespace(num_embeddings=4, embedding_size=2, embed_hidden_size=16, embed_layer_N=1,
                              embed_use_ReLU=True, use_feature_normalization=True, gnn_hidden_size=16, gnn_num_heads=3,
                              gnn_concat_heads=False, gnn_layer_N=2, gnn_use_ReLU=True, global_aggr_type="mean",
                              embed_add_self_loop=True)
    assert gnn.GnnConfig.from_args(a, 11, "node") == gc.DEFAULT
    assert gnn.GnnConfig.from_args(a, 11, "global") == dataclasses.replace(gc.DEFAULT, aggr="global_mean")
    with pytest.raises(ValueError):
        gnn.GnnConfig.from_args(a, 11, "edge")


# ---- parity of the host entry point -----------------------------------------------------------------------

@pytest.mark.parametrize("B", gc.SHAPE_B)
@pytest.mark.parametrize("E", gc.SHAPE_E)
def test_host_shapes(lib, E, B):
    gc.check(lib, gc.shape_case(E, B))


def test_host_structure(lib):
    case = gc.structure_case()
    outs = gc.check(lib, case)
    node = outs[("reference", "node")]
    np.testing.assert_array_equal(outs[("compact", "node")].view(np.int32), node.view(np.int32))
    # -0.0 entries are not edges: the same bytes as with +0.0 in their place
    plus = np.where(case.full == 0, np.float32(0), case.full)
    assert plus.view(np.int32).tolist() != case.full.view(np.int32).tolist()
    again, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, ga.dense_sources(plus)["reference"], case.agent_id)
    np.testing.assert_array_equal(again.view(np.int32), node.view(np.int32))
    # the direction: the asymmetric graph's transpose is another graph (and the model agrees with each)
    flipped = case.full.transpose(0, 2, 1).copy()
    out_t, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, ga.dense_sources(flipped)["reference"], case.agent_id)
    assert np.abs(out_t[3] - node[3]).max() > 1e-3


def test_structure_expectation_covers_its_cases(lib):
    """The expectation itself: the no-edge graph's nodes are act(lin_skip) of a zero embed sum, and the
    single-edge target's attention output is v_r + ee (alpha = 1)."""
    case = gc.structure_case()
    cfg = dataclasses.replace(case.cfg, layer_N=0)
    sd = gm.random_weights(cfg, 0)
    n = gm.nodes64(cfg, sd, case.x[:2], case.full[:2])
    b = sd["gnn.gnn1.lin_skip.bias"].astype(np.float64)
    np.testing.assert_allclose(n[0], np.broadcast_to(np.maximum(b, 0), n[0].shape), rtol=0, atol=1e-12)
    assert (case.full[1][:, 7] != 0).sum() == 1 and not case.full[1][:, 5].any()


@pytest.mark.parametrize("name", sorted(gc.OPTIONS))
def test_host_options(lib, name):
    gc.check(lib, gc.option_case(name))


@pytest.mark.parametrize("name", sorted(gc.PLAN_CASES))
def test_host_plan_cases(lib, name):
    """One case per launch plan (gnn_cases.PLAN_CASES, sized from lsm_gnn_plan); a case at the largest accepted
    E also shows E + 1 refused with nothing written."""
    gc.check(lib, gc.plan_case(name))
    if gc.PLAN_CASES[name][1] == "max":
        gc.refused_beyond(lib, name)


def test_host_ego_only_is_the_same_output(lib):
    case = gc.shape_case(24, 5)
    src = case.sources()["reference"]
    blob = case.weights()[1]
    full, _ = ga.run(lib, case.cfg, blob, case.x, src, case.agent_id)
    ego, _ = ga.run(lib, dataclasses.replace(case.cfg, ego_only=True), blob, case.x, src, case.agent_id)
    np.testing.assert_array_equal(ego.view(np.int32), full.view(np.int32))


# ---- bad inputs --------------------------------------------------------------------------------------------

def test_host_bad_inputs(lib):
    gc.bad_input_checks(lib, None)


# ---- argument refusals: nonzero and a text, before any launch or write -------------------------------------

REFUSALS = {
    "null weights": dict(over=dict(weights=None)),
    "null node_obs": dict(over=dict(node_obs=None)),
    "null adj": dict(over=dict(adj=None)),
    "null out": dict(over=dict(out=None)),
    "node aggregation, null agent_id": dict(over=dict(agent_id=None)),
    "E = 0": dict(over=dict(E=0)),
    "E = 257": dict(over=dict(E=257)),
    "compact N = 0": dict(over=dict(N=0)),
    "compact B % N": dict(over=dict(N=3)),
    "B < 0": dict(over=dict(B=-1)),
    "B = 2^31": dict(over=dict(B=2 ** 31)),
    "F = 1": dict(cfg=dict(F=1)),
    "F = 65": dict(cfg=dict(F=65)),
    "num_embeddings = 0": dict(cfg=dict(num_embeddings=0)),
    "embedding_size = 0": dict(cfg=dict(embedding_size=0)),
    "embed_hidden = 0": dict(cfg=dict(embed_hidden=0)),
    "embed_hidden = 65": dict(cfg=dict(embed_hidden=65)),
    "C = 0": dict(cfg=dict(C=0)),
    "C = 65": dict(cfg=dict(C=65)),
    "H = 0": dict(cfg=dict(H=0)),
    "H = 5": dict(cfg=dict(H=5)),
    "embed_layer_N = 5": dict(cfg=dict(embed_layer_N=5)),
    "embed_layer_N = -1": dict(cfg=dict(embed_layer_N=-1)),
    "layer_N = 5": dict(cfg=dict(layer_N=5)),
    "unknown aggregation": dict(struct=dict(aggr=4)),
    "LDS: E = 256 with H * C = 256": dict(cfg=dict(C=64, H=4, concat=True), over=dict(E=256)),
}


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(lib, what):
    spec = REFUSALS[what]
    case = gc.shape_case(24, 5)
    cfg = dataclasses.replace(case.cfg, **spec.get("cfg", {}))
    if "struct" in spec:
        st = cfg.struct()
        for k, v in spec["struct"].items():
            setattr(st, k, v)
        over = dict(spec.get("over", {}), cfg=st)
    else:
        over = spec.get("over", {})
    blob = np.zeros(20000, np.float32)
    ga.run(lib, cfg, blob, case.x, case.sources()["compact"], case.agent_id, bad_init=3, expect_rc=1, over=over)


def test_weights_floats_is_zero_for_a_refused_config(lib):
    assert lib.lsm_gnn_weights_floats(dataclasses.replace(gc.DEFAULT, H=5).struct()) == 0
    assert lib.lsm_gnn_last_error().decode().startswith("gnn: ")
    cfg = gc.DEFAULT
    assert lib.lsm_gnn_weights_floats(cfg.struct()) == sum(int(np.prod(s)) for _, s in gnn.weight_entries(cfg))


def test_empty_batch_is_legal(lib):
    case = gc.shape_case(24, 5)
    for layout in ga.LAYOUTS:
        out, bad = ga.run(lib, case.cfg, case.weights()[1], case.x[:0], case.sources()[layout], case.agent_id[:0])
        assert out.shape == (0, 16) and bad == 0
