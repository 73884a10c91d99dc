"""GPU tests of the fused graph-encoder forward (csrc/lsm_gnn.hip through include/lsm_gnn.h and
lsm/gnn.py): the kernel against tests/gnn_model.py's float64 model within the tolerance measured per case
(4 * e32 + 4 * 2^-23 * s, e32 the float32 torch model's own error: see gnn_model), in both adjacency
layouts, on tests/gnn_cases.py's cases -- each a few small graphs -- with canaries behind the output."""
import dataclasses

import numpy as np
import pytest

import gnn_abi as ga
import gnn_cases as gc
import gnn_model as gm
from lsm import capi, gnn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.mark.parametrize("B", gc.SHAPE_B)
@pytest.mark.parametrize("E", gc.SHAPE_E)
def test_shapes(lib, E, B):
    gc.check(lib, gc.shape_case(E, B), DEV)


def test_structure(lib):
    case = gc.structure_case()
    outs = gc.check(lib, case, DEV)
    node = outs[("reference", "node")]
    np.testing.assert_array_equal(outs[("compact", "node")].view(np.int32), node.view(np.int32))
    # -0.0 entries are not edges: the same bytes as with +0.0 in their place
    plus = np.where(case.full == 0, np.float32(0), case.full)
    again, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, ga.dense_sources(plus, DEV)["reference"], case.agent_id)
    np.testing.assert_array_equal(again.view(np.int32), node.view(np.int32))
    # the direction: the asymmetric graph's transpose is another graph
    flipped = case.full.transpose(0, 2, 1).copy()
    out_t, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, ga.dense_sources(flipped, DEV)["reference"],
                      case.agent_id)
    assert np.abs(out_t[3] - node[3]).max() > 1e-3


@pytest.mark.parametrize("name", sorted(gc.OPTIONS))
def test_options(lib, name):
    gc.check(lib, gc.option_case(name), DEV)


@pytest.mark.parametrize("name", sorted(gc.PLAN_CASES))
def test_plan_cases(lib, name):
    """One case per launch plan (gnn_cases.PLAN_CASES, sized from lsm_gnn_plan): every team size, a graph count
    the LDS cut (to 3 and to 1), both sides of the adjacency's move out of LDS in both instances, the largest
    graphs and the widest config at its largest accepted E, with E + 1 refused and nothing written."""
    gc.check(lib, gc.plan_case(name), DEV)
    if gc.PLAN_CASES[name][1] == "max":
        gc.refused_beyond(lib, name, DEV)


def test_ego_row(lib):
    """agent_id differing per graph, 0 and E - 1 among them: each row is that node's, not another's."""
    case = gc.shape_case(24, 5)
    ids = case.agent_id
    assert ids[0] == 0 and ids[-1] == 23 and len(set(ids.tolist())) == 5
    src = case.sources(DEV)["reference"]
    out, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, src, ids)
    w64, tol, e32 = case.ref.want(case.cfg, ids)
    gm.assert_close(out, w64, tol, e32, "ego row")
    other, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, src, (ids + 1) % 24)
    assert (np.abs(other - out).max(axis=1) > 10 * tol).all()
    # the timing knob computes the same row
    ego, _ = ga.run(lib, dataclasses.replace(case.cfg, ego_only=True), case.weights()[1], case.x, src, ids)
    np.testing.assert_array_equal(ego.view(np.int32), out.view(np.int32))


def test_bad_inputs_and_nan_edge(lib):
    gc.bad_input_checks(lib, DEV)


@pytest.mark.parametrize("E,B", [(24, 67), (192, 5)])
def test_same_call_twice_gives_identical_bytes(lib, E, B):
    case = gc.shape_case(E, B)
    for layout in ga.LAYOUTS:
        src = case.sources(DEV)[layout]
        a, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, src, case.agent_id)
        b, _ = ga.run(lib, case.cfg, case.weights()[1], case.x, src, case.agent_id)
        np.testing.assert_array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("which", ["shape 24 67", "shape 65 5", "shape 192 1", "option C12 hidden20", "option tanh"])
def test_device_matches_host(lib, which):
    """The kernel and lsm_host_gnn_forward run one per-graph text; exp / tanh / rsqrt and the FMA
    contraction differ, so the comparison uses the case's tolerance, not bit equality."""
    kind, rest = which.split(" ", 1)
    case = gc.shape_case(*map(int, rest.split())) if kind == "shape" else gc.option_case(rest)
    for aggr in case.aggrs:
        cfg = case.with_aggr(aggr)
        blob = case.weights(aggr)[1]
        host, _ = ga.run(lib, cfg, blob, case.x, case.sources(None)["compact"], case.agent_id)
        dev, _ = ga.run(lib, cfg, blob, case.x, case.sources(DEV)["compact"], case.agent_id)
        _, tol, e32 = case.ref.want(cfg, case.agent_id)
        err = float(np.abs(dev.astype(np.float64) - host).max())
        print("gnn device vs host %s %s: %.3e (tol %.3e)" % (which, aggr, err, tol))
        assert err <= tol, (which, aggr, err, tol)


@pytest.mark.parametrize("layout", ga.LAYOUTS)
def test_public_surface(lib, layout):
    """GraphEncoder.forward / forward_compact and GpuGraphVecEnv.gnn_features on a 4-env, N = 3 env after
    one step, against model64 on the expanded adjacency; load() changes the output; non-CUDA is refused."""
    import torch
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    env = GpuGraphVecEnv(EnvArgs(num_agents=3, seed=1), num_envs=4, device=DEV, return_numpy=False, build_infos=False,
                         adj_layout=layout)
    env.reset(0)
    env.step(torch.full((4, 3), 7, dtype=torch.int32, device=DEV), 0)
    B, E, F = 12, env.E, env.F
    x = env.t_node.view(B, E, F).cpu().numpy()
    adj = env.reference_adj().reshape(B, E, E).cpu().numpy()
    ids = env.agent_id.view(B).cpu().numpy()
    assert (adj != 0).any() and set(ids.tolist()) == {0, 1, 2}
    for aggr in ("node", "global_mean"):
        cfg = gnn.GnnConfig(F=F, aggr=aggr)
        sd, blob = gm.default_weights(cfg, 5)
        enc = gnn.GraphEncoder(cfg, blob, DEV)
        ref = gm.Reference(cfg, sd, x, adj)
        w64, tol, e32 = ref.want(cfg, ids)
        got = env.gnn_features(enc, check=True).clone()
        assert got.shape == (B, 16) and got.is_cuda
        gm.assert_close(got.cpu().numpy(), w64, tol, e32, "gnn_features %s %s" % (layout, aggr))
        # the two entry points of the encoder on the same step agree to the byte
        dense = enc.forward(env.t_node.view(B, E, F), env.reference_adj().reshape(B, E, E).contiguous(),
                            env.agent_id.view(B, 1)).clone()
        np.testing.assert_array_equal(dense.cpu().numpy().view(np.int32), got.cpu().numpy().view(np.int32))
        if layout == "compact":
            cmp_ = enc.forward_compact(env.t_node.view(B, E, F), env.t_adj, env.t_adj_mask, 3, env.agent_id).clone()
            np.testing.assert_array_equal(cmp_.cpu().numpy().view(np.int32), dense.cpu().numpy().view(np.int32))
        # load(): new weights, new output, the new model's
        sd2 = gm.random_weights(cfg, 6)
        enc.load(sd2)
        got2 = env.gnn_features(enc).cpu().numpy()
        ref2 = gm.Reference(cfg, sd2, x, adj)
        gm.assert_close(got2, *ref2.want(cfg, ids), "after load %s %s" % (layout, aggr))
        assert np.abs(got2 - dense.cpu().numpy()).max() > 1e-3
        # a non-CUDA tensor is refused
        with pytest.raises(gnn.GnnError):
            enc.forward(env.t_node.view(B, E, F).cpu(), env.reference_adj().reshape(B, E, E), env.agent_id)
        with pytest.raises(gnn.GnnError):
            enc.forward(env.t_node.view(B, E, F), env.reference_adj().reshape(B, E, E).cpu(), env.agent_id)
    with pytest.raises(gnn.GnnError):
        gnn.GraphEncoder(cfg, blob, "cpu")
    # check=True raises on an out-of-range agent id and clears the word
    cfg = gnn.GnnConfig(F=F)
    enc = gnn.GraphEncoder(cfg, gm.default_weights(cfg, 5)[1], DEV)
    bad_ids = torch.full((B, 1), E, dtype=torch.int64, device=DEV)
    dense_adj = env.reference_adj().reshape(B, E, E).contiguous()
    with pytest.raises(gnn.GnnError):
        enc.forward(env.t_node.view(B, E, F), dense_adj, bad_ids, check=True)
    assert int(enc.bad.item()) == 0
    assert not enc.forward(env.t_node.view(B, E, F), dense_adj, bad_ids).cpu().numpy().any()
    env.close()
