"""GPU tests of the recurrent hand-off (csrc/lsm_chunks.hip, DeviceGraphBuffer's policy rows and
recurrent_generator) against the minibatches recorded from the reference's recurrent_generator
(tests/golden/recurrent/) and the numpy model (tests/recurrent_model.py). Every comparison is of bytes:
the code under test only copies, selects and zero-fills."""
import numpy as np
import pytest

import recurrent_abi as ra
import recurrent_model as rcm
from lsm import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


# ---- lsm_buffer_gather_chunks -----------------------------------------------------------------------

@pytest.mark.parametrize("name", ra.fixtures())
def test_gpu_gather_chunks_matches_fixture(lib, name):
    z = ra.load_fixture(name)
    T, M, L, mb = z["T"], z["M"], z["L"], z["mb"]
    specs, names = ra.fixture_specs(z)
    for i in range(z["num_mini_batch"]):
        chunks = z["perm"][i * mb:(i + 1) * mb]
        got, bad = ra.run_fixture(lib, specs, chunks, L, T, M, device=DEV)
        assert bad == 0
        for g, nm, s in zip(got, names, specs):
            np.testing.assert_array_equal(g, ra.fixture_batch(z, i, nm), err_msg="%s (%s) batch %d" % (nm, s["kind"], i))


T_SYN, M_SYN, L_SYN = 7, 40, 4          # 280 samples, a multiple of every N below; L does not divide T
ROW_WORDS = [1, 6, 4, 12, 576]          # 4, 24, 16, 48 and 2304 B
COMPACT = [(10, 5), (16, 8)]            # E % 4 != 0 (4-B units) and E % 4 == 0 (16-B units)
COMPACT_WIDE = [(70, 2), (72, 2)]       # two mask words


def _synthetic(compact):
    rng = np.random.default_rng(7)
    rows = T_SYN * M_SYN
    specs = [dict(kind="rows", src=rng.integers(-2 ** 31, 2 ** 31, (rows, w)).astype(np.int32)) for w in ROW_WORDS]
    # 16-B rows that sit 4 bytes off a 16-byte boundary (src and dst): the 4-B path
    specs.append(dict(kind="rows", off=1, src=rng.integers(-2 ** 31, 2 ** 31, (rows, 4)).astype(np.int32)))
    for w in (8, 3):   # the recurrent states: 16-B and 4-B units
        specs.append(dict(kind="first", src=rng.integers(-2 ** 31, 2 ** 31, (rows, w)).astype(np.int32)))
    for E, N in compact:
        A = rng.normal(0, 1, (rows // N, E, E)).astype(np.float32)
        A[A == 0] = 1.0   # non-zero under every set bit: a product with the mask would differ from the select
        A[0, 0, 0] = np.inf
        bits = rng.random((rows, E)) < 0.2
        bits[0, 0] = bits[0, E - 1] = bits[1, 1] = True
        bits[2] = False
        specs.append(dict(kind="compact", A=A, masks=rcm.pack_bits(bits), N=N))
    return specs


@pytest.fixture(scope="module")
def sources():
    return {"lean": ra.ChunkSources(_synthetic(COMPACT), DEV),
            "wide": ra.ChunkSources(_synthetic(COMPACT + COMPACT_WIDE), DEV)}


# 1000 chunks of 4 steps: 576 000 units in the 2304-byte field, more than one grid of 2048 x 256 threads
@pytest.mark.parametrize("Cn,which", [(1, "wide"), (37, "wide"), (70, "lean"), (1000, "lean")])
def test_gpu_gather_chunks_matches_numpy(lib, sources, Cn, which):
    src = sources[which]
    nch = rcm.data_chunks(L_SYN, T_SYN, M_SYN)
    assert nch == 70 and (np.arange(nch) * L_SYN % T_SYN + L_SYN > T_SYN).any()   # some chunks straddle
    rng = np.random.default_rng(Cn)
    if Cn == 1:
        cases = [[0], [nch - 1], [1]]   # chunk 1 covers samples 4..7: it runs from column 0 into column 1
    elif Cn == nch:
        cases = [rng.permutation(nch)]
    else:
        c = rng.integers(0, nch, Cn)     # duplicates are allowed at the ABI level
        c[[0, 1, 2, 3, Cn - 1]] = [0, nch - 1, 5, 5, 0]
        cases = [c]
    for chunks in cases:
        got, bad = src.run(lib, chunks, L_SYN, T_SYN, M_SYN)   # run() checks the canaries
        assert bad == 0
        for g, w, s in zip(got, src.model(chunks, L_SYN, T_SYN, M_SYN), src.specs):
            np.testing.assert_array_equal(g, w, err_msg=str((s["kind"], g.shape)))


def test_gpu_gather_chunks_bad_ids(lib, sources):
    src = sources["wide"]
    nch = rcm.data_chunks(L_SYN, T_SYN, M_SYN)
    chunks = np.random.default_rng(1).integers(0, nch, 37)
    bad_at = [3, 5, 7, 36]
    chunks[bad_at] = [nch, -1, 2 ** 40, -2 ** 40]
    got, bad = src.run(lib, chunks, L_SYN, T_SYN, M_SYN)
    assert bad == 1
    for g, w, s in zip(got, src.model(chunks, L_SYN, T_SYN, M_SYN), src.specs):
        steps = 1 if s["kind"] == "first" else L_SYN
        assert (g.reshape(steps, 37, -1)[:, bad_at] == 0).all(), s["kind"]
        np.testing.assert_array_equal(g, w, err_msg=s["kind"])


# ---- lsm_buffer_copy_rows ---------------------------------------------------------------------------

@pytest.mark.parametrize("M", [100, 1000])
@pytest.mark.parametrize("dones", ["none", "all", "third", "null"])
def test_gpu_copy_rows(lib, M, dones):
    rng = np.random.default_rng(M)
    widths = [1, 1, 4, 4, 6, 8, 4]   # 4-B rows, 16-B rows, 24-B rows (4-B units), 32-B rows, 16-B rows off by 4
    offs = [0, 0, 0, 0, 0, 0, 1]
    flags = [1, 0, 1, 0, 1, 1, 1]
    srcs = [rng.integers(1, 2 ** 31, (M, w)).astype(np.int32) for w in widths]   # no zero words
    d = {"none": np.zeros(M, np.uint8), "all": np.ones(M, np.uint8),
         "third": (np.arange(M) % 3 == 0).astype(np.uint8), "null": None}[dones]
    if d is None:
        flags = [0] * len(widths)
    got = ra.copy_rows(lib, srcs, d, flags, M, DEV, offs)   # checks the neighbouring rows' canaries
    for g, s, fl in zip(got, srcs, flags):
        np.testing.assert_array_equal(g, rcm.copy_rows(s, d, fl))
        if fl:
            np.testing.assert_array_equal((g == 0).all(axis=1), d != 0)   # zero exactly where done
        else:
            np.testing.assert_array_equal(g, s)


# ---- end to end: two buffers, reference and compact layout ------------------------------------------

POLICY = dict(hidden_size=4, recurrent_N=2, num_actions=25)


def test_gpu_buffer_recurrent_hand_off():
    import torch
    from lsm import hj_tables
    from lsm.buffer import BufferError, DeviceGraphBuffer, chunk_rows
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv
    T, n, N = 6, 12, 8
    M = n * N
    # episodes of 4 steps in a buffer of 6: every env is done, and resets, at buffer row 4
    args = EnvArgs(num_agents=N, episode_length=4, num_env_steps=T * 4, use_safety_filter=True, seed=11)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    envs = [GpuGraphVecEnv(args, num_envs=n, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                           adj_layout=layout) for layout in ("reference", "compact")]
    bufs = [DeviceGraphBuffer(e, episode_length=T, policy_rows=POLICY) for e in envs]
    assert bufs[0].adj_mask is None and bufs[1].adj_mask is not None
    host = lambda t: t.cpu().numpy()
    E = envs[0].E
    for b in bufs:
        assert b.rnn_states.shape == (T + 1, n, N, 2, 4) and b.rnn_states_critic.shape == (T + 1, n, N, 2, 4)
        assert b.actions.shape == (T, n, N, 1) and b.action_log_probs.shape == (T, n, N, 1)
        assert b.available_actions.shape == (T + 1, n, N, 25)
        assert not b.rnn_states.any() and not b.actions.any() and bool((b.available_actions == 1).all())
        b.warmup(4)
    g = torch.Generator(device=DEV).manual_seed(5)
    rand = lambda *s: torch.rand(s, generator=g, device=DEV) + 0.5   # never zero
    for t in range(T):
        a = torch.randint(0, 25, (n, N), generator=g, device=DEV, dtype=torch.int32)
        vp = torch.randn((n, N), generator=g, device=DEV)
        pol = dict(actions=a.to(torch.float32).reshape(n, N, 1), action_log_probs=-rand(n, N, 1),
                   rnn_states=rand(n, N, 2, 4), rnn_states_critic=rand(n, N, 2, 4),
                   available_actions=(rand(n, N, 25) > 0.8).to(torch.float32))
        for b in bufs:
            dones, _ = b.insert_step(a, 4, value_preds=vp, policy=pol)
            done = host(b.masks[t + 1, ..., 0]) == 0
            np.testing.assert_array_equal(done, host(dones) != 0)
            for k in ("rnn_states", "rnn_states_critic"):
                got = host(getattr(b, k)[t + 1])
                np.testing.assert_array_equal((got == 0).all(axis=(2, 3)), done, err_msg=k)   # zero exactly where done
                np.testing.assert_array_equal(got[~done], host(pol[k])[~done], err_msg=k)
            assert torch.equal(b.actions[t], pol["actions"]) and torch.equal(b.action_log_probs[t], pol["action_log_probs"])
            assert torch.equal(b.available_actions[t + 1], pol["available_actions"])
            assert torch.equal(b.value_preds[t, ..., 0], vp)
    masks = host(bufs[0].masks)
    whole = (masks[1:, :, :, 0] == 0).all(axis=2)
    assert whole.any() and not whole.all()   # whole-env dones occurred, inside the gathered rows too
    assert (masks[1:T] == 0).any()

    next_value = torch.randn((n, N, 1), generator=g, device=DEV)
    advs = []
    for b in bufs:
        b.compute_returns(next_value, None, gamma=0.99, gae_lambda=0.95)
        advs.append(b.advantages(None)[0])
    assert host(advs[0]).tobytes() == host(advs[1]).tobytes()

    ref = bufs[0]
    views = {k: host(getattr(ref, k))[:T] for k in rcm.NAMES if k != "advantages"}
    views["advantages"] = host(advs[0])
    views = {k: v.reshape((T * M,) + v.shape[3:]) for k, v in views.items()}
    for L, k_mb in ((4, 3), (3, 4)):
        nch = T * M // L
        assert nch == {4: 144, 3: 192}[L]
        perm = torch.randperm(nch, generator=torch.Generator().manual_seed(3)).to(DEV)
        p = host(perm)
        if L == 4:
            assert ((p * L) % T + L > T).any()   # straddling chunks
        got = []
        for b, adv in zip(bufs, advs):
            out = []
            for mb in b.recurrent_generator(adv, k_mb, L, chunks=perm):
                assert tuple(mb) == rcm.NAMES + ("chunks",)   # the reference's names, in its yield order
                out.append({f: host(v).copy() for f, v in mb.items()})
            got.append(out)
        assert len(got[0]) == k_mb and len(got[1]) == k_mb
        C = nch // k_mb
        for i, (r, c) in enumerate(zip(got[0], got[1])):
            ch = p[i * C:(i + 1) * C]
            np.testing.assert_array_equal(r["chunks"], ch)
            np.testing.assert_array_equal(host(chunk_rows(perm[i * C:(i + 1) * C], L, T, M)),
                                          rcm.chunk_rows(ch, L, T, M))
            for f in rcm.NAMES + ("chunks",):
                assert r[f].dtype == c[f].dtype and r[f].shape == c[f].shape, f
                assert r[f].tobytes() == c[f].tobytes(), f   # the two layouts give the same bytes
            for f in rcm.NAMES:
                want = (rcm.gather_first if f in rcm.FIRST else rcm.gather_rows)(views[f], ch, L, T, M)
                assert r[f].shape == want.shape and r[f].dtype == want.dtype, f
                assert r[f].tobytes() == want.tobytes(), f
            assert r["adj"].shape == (L * C, E, E) and r["rnn_states"].shape == (C, 2, 4)

    # the default permutation: a device randperm, num_mini_batch batches of distinct chunks
    gen = torch.Generator(device=DEV).manual_seed(9)
    ids = [host(mb["chunks"]).copy() for mb in ref.recurrent_generator(advs[0], 5, 4, generator=gen)]
    assert len(ids) == 5 and all(len(x) == 144 // 5 for x in ids)
    allc = np.concatenate(ids)
    assert len(np.unique(allc)) == len(allc) and allc.min() >= 0 and allc.max() < 144
    with pytest.raises(BufferError):
        next(ref.recurrent_generator(advs[0], 2, 4, chunks=torch.zeros(144, dtype=torch.int64, device=DEV)))

    # after_update carries row T of the three new fields to row 0
    for b in bufs:
        last = {k: host(getattr(b, k)[-1]).copy() for k in ("rnn_states", "rnn_states_critic", "available_actions")}
        assert any((last[k] != host(getattr(b, k)[0])).any() for k in last)
        b.after_update()
        for k in last:
            np.testing.assert_array_equal(host(getattr(b, k)[0]), last[k], err_msg=k)

    # a buffer without policy_rows: no policy fields, and policy= is refused
    for e in envs:
        e.close()
    env = GpuGraphVecEnv(args, num_envs=n, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                         adj_layout="compact")
    plain = DeviceGraphBuffer(env, episode_length=T)
    assert plain.rnn_states is None and plain.actions is None and plain.available_actions is None
    plain.warmup(4)
    a = torch.zeros((n, N), device=DEV, dtype=torch.int32)
    with pytest.raises(BufferError):
        plain.insert_step(a, 4, policy=dict(actions=a, action_log_probs=a, rnn_states=a, rnn_states_critic=a))
    assert plain.step == 0
    for t in range(T):
        plain.insert_step(a, 4, value_preds=torch.randn((n, N), generator=g, device=DEV))
    adv = torch.randn((T, n, N, 1), generator=g, device=DEV)
    perm = torch.randperm(144, generator=torch.Generator().manual_seed(4)).to(DEV)
    names = tuple(k for k in rcm.NAMES if k not in rcm.POLICY)
    pviews = {k: host(getattr(plain, k))[:T] for k in names if k not in ("advantages", "adj")}
    pviews["advantages"] = host(adv)
    for i, mb in enumerate(plain.recurrent_generator(adv, 2, 4, chunks=perm)):
        assert tuple(mb) == names + ("chunks",)
        ch = host(perm)[i * 72:(i + 1) * 72]
        for f, v in pviews.items():
            want = rcm.gather_rows(v.reshape((T * M,) + v.shape[3:]), ch, 4, T, M)
            assert host(mb[f]).tobytes() == want.tobytes(), f
    env.close()
