"""GPU tests of the minibatch edge lists (csrc/lsm_mb_edges.hip, lsm.edges.minibatch_edges and the
generators' edges=True) against oracle/process_adj.py on the adjacency the reference's recurrent_generator
yielded (tests/golden/recurrent/) and on numpy-built dense matrices (tests/mb_edges_abi.py). Every
comparison is of bytes."""
import numpy as np
import pytest

import mb_edges_abi as mb
import recurrent_abi as ra
import recurrent_model as rcm
from lsm import capi
from oracle.process_adj import process_adj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ("reference", "compact")


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


@pytest.fixture(scope="module")
def synthetic():
    return {E: mb.synthetic(E, DEV) for E in mb.SYN_E}


def _check(lib, src, ids, chunks, want, what, **kw):
    want_ei, want_ea, want_off = want
    ei, ea, off, bad = mb.run_device(lib, src, ids, chunks, **kw)   # checks the canaries behind every output
    np.testing.assert_array_equal(off, want_off, err_msg=str(what))
    mb.assert_edges(ei, ea, want_ei, want_ea, what)
    return bad


# ---- count + emit -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ra.fixtures())
def test_gpu_fixture_minibatches(lib, name):
    z = ra.load_fixture(name)
    T, M, L, mbs = z["T"], z["M"], z["L"], z["mb"]
    srcs = mb.fixture_sources(z, DEV)
    full = srcs["reference"].full
    perm = np.random.default_rng(T * M).permutation(T * M)
    for i in range(z["num_mini_batch"]):
        chunks = z["perm"][i * mbs:(i + 1) * mbs]
        want = mb.expected(full, chunks, (L, T, M))
        ref_ei, ref_ea = process_adj(z["b%d_adj" % i])   # what the reference's generator yielded
        mb.assert_edges(want[0], want[1], ref_ei, ref_ea, (name, i, "model"))
        ids = perm[i::z["num_mini_batch"]]
        want_idx = mb.expected(full, ids, None)
        for layout in LAYOUTS:
            assert _check(lib, srcs[layout], chunks, (L, T, M), want, (name, i, layout, "chunks")) == 0
            assert _check(lib, srcs[layout], ids, None, want_idx, (name, i, layout, "indices")) == 0


@pytest.mark.parametrize("E", mb.SYN_E)
def test_gpu_synthetic(lib, synthetic, E):
    srcs = synthetic[E]
    for case in sorted(mb.SYN_CASES):
        ids, chunks = mb.syn_case(case)
        want = mb.expected(srcs["reference"].full, ids, chunks)
        for layout in LAYOUTS:
            assert _check(lib, srcs[layout], ids, chunks, want, (E, case, layout)) == 0


def test_gpu_unaligned_adjacency_takes_the_4_byte_path(lib):
    """An even E whose matrices start 4 bytes off a 16-byte boundary: no 16-B loads from them."""
    full = mb.synthetic(24)["reference"].full
    src = mb.Source(full, device=DEV)
    src.adj = ra.Placed(full.view(np.int32), 1, DEV)
    ids, chunks = mb.syn_case("idx9")
    assert _check(lib, src, ids, chunks, mb.expected(full, ids, chunks), "off by 4") == 0


def test_gpu_empty_minibatch(lib, synthetic):
    for chunks in (None, (3, mb.SYN_T, 4)):
        ei, ea, off, bad = mb.run_device(lib, synthetic[24]["compact"], [], chunks)
        assert off.tolist() == [0] and ei.shape == (2, 0) and bad == 0


# ---- nnz read on the device ---------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_device_side_nnz(lib, synthetic, layout):
    for E, case in ((24, "idx9"), (66, "chunk9"), (5, "chunk5")):
        src = synthetic[E][layout]
        ids, chunks = mb.syn_case(case)
        want = mb.expected(src.full, ids, chunks)
        nnz = want[1].shape[0]
        assert nnz > 1
        for cap in (nnz, nnz + 7):
            _check(lib, src, ids, chunks, want, (E, case, cap), dev_nnz=True, cap=cap)
        # one edge too few: nothing is written (run_device checks every output word) and offsets[G] reports nnz
        ei, ea, off, bad = mb.run_device(lib, src, ids, chunks, dev_nnz=True, cap=nnz - 1)
        assert ei.shape == (2, 0) and ea.shape == (0, 1) and off[-1] == nnz
        np.testing.assert_array_equal(off, want[2])


# ---- bad ids --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_bad_ids(lib, synthetic, layout):
    E, rows = 24, 12
    src = synthetic[E][layout]
    for chunks, limit in ((None, rows), ((3, mb.SYN_T, 4), rows // 3)):
        ids = np.array([2, -1, 1, limit, 2 ** 40, limit - 1, 2, -2 ** 40, 0], dtype=np.int64)
        steps = chunks[0] if chunks else 1
        want = mb.expected(src.full, ids, chunks)
        ei, ea, off, bad = mb.run_device(lib, src, ids, chunks)
        assert bad == 1
        np.testing.assert_array_equal(off, want[2])
        mb.assert_edges(ei, ea, want[0], want[1], (layout, chunks))
        per = np.diff(off).reshape(steps, len(ids))
        assert (per[:, [1, 3, 4, 7]] == 0).all() and per[:, [0, 5, 6]].any()
        assert set(np.unique(ei[0] // E)) == {g for g in range(steps * len(ids)) if per.reshape(-1)[g]}
        assert mb.run_device(lib, src, ids[[0, 2, 5, 6, 8]], chunks)[3] == 0


# ---- end to end: two buffers, reference and compact layout ------------------------------------------

POLICY = dict(hidden_size=4, recurrent_N=2, num_actions=25)
FF_KEYS = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "value_preds", "returns", "masks",
           "active_masks", "advantages", "indices")


def test_gpu_generators_yield_edges():
    import torch
    from lsm import edges as lsm_edges
    from lsm import hj_tables
    from lsm.buffer import DeviceGraphBuffer
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    T, n, N = 6, 12, 8
    M = n * N
    args = EnvArgs(num_agents=N, episode_length=4, num_env_steps=T * 4, use_safety_filter=True, seed=11)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    envs = [GpuGraphVecEnv(args, num_envs=n, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                           adj_layout=layout) for layout in LAYOUTS]
    bufs = [DeviceGraphBuffer(e, episode_length=T, policy_rows=POLICY) for e in envs]
    assert bufs[0].adj_mask is None and bufs[1].adj_mask is not None
    E = envs[0].E
    for b in bufs:
        b.warmup(4)
    g = torch.Generator(device=DEV).manual_seed(5)
    for t in range(T):
        a = torch.randint(0, 25, (n, N), generator=g, device=DEV, dtype=torch.int32)
        vp = torch.randn((n, N), generator=g, device=DEV)
        pol = dict(actions=a.to(torch.float32).reshape(n, N, 1), action_log_probs=torch.randn((n, N, 1), generator=g, device=DEV),
                   rnn_states=torch.randn((n, N, 2, 4), generator=g, device=DEV),
                   rnn_states_critic=torch.randn((n, N, 2, 4), generator=g, device=DEV))
        for b in bufs:
            b.insert_step(a, 4, value_preds=vp, policy=pol)
    next_value = torch.randn((n, N, 1), generator=g, device=DEV)
    advs = []
    for b in bufs:
        b.compute_returns(next_value, None, gamma=0.99, gae_lambda=0.95)
        advs.append(b.advantages(None)[0])
    host = lambda t: t.cpu().numpy()
    ref_adj = host(bufs[0].adj[:T]).reshape(T * M, E, E)

    def collect(gen):
        return [{k: (v.clone() if v is not None else None) for k, v in mbatch.items()} for mbatch in gen]

    def compare(plain, edged, keys, idkey, chunks):
        assert len(plain) == len(edged) == 2 and len(plain[0]) == len(edged[0]) > 1
        for layout in range(2):
            for p, e in zip(plain[layout], edged[layout]):
                assert tuple(p) == keys                                   # a default generator: today's keys
                assert tuple(e) == keys + ("edge_index", "edge_attr")
                assert e["adj"] is None and p["adj"].shape[1:] == (E, E)
                for k in keys:                                            # every other field is unchanged
                    if k != "adj" and p[k] is not None:
                        assert torch.equal(p[k], e[k]), k
                    else:
                        assert k == "adj" or e[k] is None
                want_ei, want_ea = lsm_edges.process_adj(p["adj"])
                assert e["edge_index"].dtype == torch.int64 and e["edge_attr"].dtype == torch.float32
                assert e["edge_index"].shape == want_ei.shape and e["edge_attr"].shape == want_ea.shape
                assert torch.equal(e["edge_index"], want_ei) and torch.equal(e["edge_attr"], want_ea)
                assert want_ea.shape[0] > 0 and e["edge_index"].is_contiguous() and e["edge_attr"].is_contiguous()
                # and the oracle on the numpy statement of the minibatch
                ora_ei, ora_ea, _ = mb.expected(ref_adj, host(e[idkey]), chunks)
                mb.assert_edges(host(e["edge_index"]), host(e["edge_attr"]), ora_ei, ora_ea, idkey)
        for r, c in zip(edged[0], edged[1]):                              # the two layouts agree
            assert torch.equal(r["edge_index"], c["edge_index"]) and torch.equal(r["edge_attr"], c["edge_attr"])

    # feed_forward_generator
    perm = torch.randperm(T * M, generator=torch.Generator().manual_seed(3)).to(DEV)
    plain = [collect(b.feed_forward_generator(adv, num_mini_batch=3, indices=perm)) for b, adv in zip(bufs, advs)]
    edged = [collect(b.feed_forward_generator(adv, num_mini_batch=3, indices=perm, edges=True))
             for b, adv in zip(bufs, advs)]
    compare(plain, edged, FF_KEYS, "indices", None)

    # recurrent_generator: L = 4 does not divide T = 6, so chunks straddle two series
    for L, k_mb in ((4, 3), (3, 4)):
        nch = T * M // L
        cperm = torch.randperm(nch, generator=torch.Generator().manual_seed(3)).to(DEV)
        if L == 4:
            assert ((host(cperm) * L) % T + L > T).any()
        plain = [collect(b.recurrent_generator(adv, k_mb, L, chunks=cperm)) for b, adv in zip(bufs, advs)]
        edged = [collect(b.recurrent_generator(adv, k_mb, L, chunks=cperm, edges=True)) for b, adv in zip(bufs, advs)]
        compare(plain, edged, rcm.NAMES + ("chunks",), "chunks", (L, T, M))

    # the count-first path (outputs sized exactly) gives the same tensors as the bounded one
    bounded = edged[1]
    keep = lsm_edges.BOUNDED_OUTPUT_BYTES
    lsm_edges.BOUNDED_OUTPUT_BYTES = 0
    try:
        exact = collect(bufs[1].recurrent_generator(advs[1], 4, 3, chunks=cperm, edges=True))
    finally:
        lsm_edges.BOUNDED_OUTPUT_BYTES = keep
    for x, y in zip(exact, bounded):
        assert torch.equal(x["edge_index"], y["edge_index"]) and torch.equal(x["edge_attr"], y["edge_attr"])

    # minibatch_edges itself: an id outside the buffer raises, and the next call is clean again
    ids = torch.tensor([3, T * M, 5], dtype=torch.int64, device=DEV)
    with pytest.raises(lsm_edges.EdgeError):
        lsm_edges.minibatch_edges(bufs[0].adj[:T], None, N, ids)
    ei, ea = lsm_edges.minibatch_edges(bufs[0].adj[:T], None, N, ids[[0, 2, 0]])
    ora_ei, ora_ea, _ = mb.expected(ref_adj, np.array([3, 5, 3]), None)
    mb.assert_edges(host(ei), host(ea), ora_ei, ora_ea, "after a bad id")
    for e in envs:
        e.close()
