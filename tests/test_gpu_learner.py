"""GPU tests of the learner hand-off (csrc/lsm_returns.hip, csrc/lsm_gather.hip, DeviceGraphBuffer's
compute_returns / advantages / feed_forward_generator) against the fixtures recorded from the reference
(tests/golden/returns/), lsm_host_compute_returns and the numpy model (tests/returns_model.py).

Tolerances: returns and every gathered byte are bit-equal. The advantage statistics are float64 sums of
at most 2.2e6 float32 values, each thread adding at most 34 of them before the tree of partial sums
(error below 1e-13) in a one-pass variance on inputs with |mean| <= 2 std: rtol 1e-9 against
np.nanmean / np.nanstd of the float64-cast values. The normalised advantages are compared with the reference's float32 expression at the project's float32 output tolerance, 1e-5 (the
float32-versus-float64 statistics differ by 4.8e-7 at most on the CPU)."""
import ctypes as C

import numpy as np
import pytest

import learner_abi as la
import returns_model as rm
from lsm import capi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BRANCHES = [(g, p, d) for g in (False, True) for p in (False, True) for d in (False, True)]
DEN = np.array([2.8504124, 2.038297], dtype=np.float32)


@pytest.fixture(scope="module")
def lib():
    return capi.load_library()


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _tp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- lsm_buffer_compute_returns ---------------------------------------------------------------------

@pytest.mark.parametrize("name", la.fixtures())
def test_gpu_compute_returns_matches_fixture(lib, name):
    z = la.load_fixture(name)
    T, M, gae = z["T"], z["M"], bool(z["use_gae"])
    ret, v = la.compute_returns(lib, z["rewards"], z["value_preds_in"], z["masks"], z["bad_masks"], z["next_value"],
                                z["den"], z["gamma"], z["gae_lambda"], gae, bool(z["use_proper_time_limits"]),
                                device=DEV)
    rows = la.written_rows(T, gae)
    np.testing.assert_array_equal(la.bits(ret[rows]), la.bits(z["returns"].reshape(T + 1, M)[rows]))
    np.testing.assert_array_equal(la.bits(v), la.bits(z["value_preds_out"].reshape(T + 1, M)))
    if gae:
        assert (ret[T] == la.SENTINEL).all()


@pytest.mark.parametrize("T,M", [(1, 1), (6, 15), (6, 296), (25, 1000)])
def test_gpu_compute_returns_matches_host(lib, T, M):
    rng = np.random.default_rng(100 * T + M)
    f32 = np.float32
    rewards = rng.normal(0, 2, (T, M)).astype(f32)
    values = rng.normal(0.5, 1.5, (T + 1, M)).astype(f32)
    masks = (rng.random((T + 1, M)) >= 0.3).astype(f32)
    bad = (rng.random((T + 1, M)) >= 0.3).astype(f32)
    nv = rng.normal(0.5, 1.5, M).astype(f32)
    for gae, proper, den in BRANCHES:
        args = (rewards, values, masks, bad if proper else None, nv, DEN if den else None, 0.99, 0.95, gae, proper)
        h_ret, h_v = la.compute_returns(lib, *args)
        d_ret, d_v = la.compute_returns(lib, *args, device=DEV)
        # all rows: the one the branch does not write holds the sentinel on both sides
        np.testing.assert_array_equal(la.bits(d_ret), la.bits(h_ret), err_msg=str((gae, proper, den)))
        np.testing.assert_array_equal(la.bits(d_v), la.bits(h_v), err_msg=str((gae, proper, den)))


# ---- lsm_buffer_advantages --------------------------------------------------------------------------

def _advantages(lib, returns, values, active, den):
    import torch
    count = returns.size
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32).reshape(-1),
                                                         device=DEV)
    tr, tv, ta, td = t(returns), t(values), t(active), t(den)
    nbytes = lib.lsm_buffer_advantages_workspace_bytes(count)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    adv = torch.full((count + 8,), float(la.SENTINEL), dtype=torch.float32, device=DEV)   # 8 canaries
    stats = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    rc = lib.lsm_buffer_advantages(_tp(tr), _tp(tv), _tp(ta), _tp(td), count, _tp(adv), _tp(stats), _tp(ws), nbytes,
                                   _stream())
    assert rc == 0, lib.lsm_returns_last_error()
    torch.cuda.synchronize()
    a = adv.cpu().numpy()
    assert (a[count:] == la.SENTINEL).all()
    return a[:count], stats.cpu().numpy()


def _advantage_case(count, den):
    if count == 90:   # the fixture's shape: T * n * N = 6 * 3 * 5
        z = la.load_fixture("t6_gae1_ptl0_vn%d" % (den is not None))
        ret, val, act = z["returns"][:-1], z["value_preds_out"][:-1], z["active_masks"][:-1]
        raw = ret - rm.dn(val, den)
        np.testing.assert_array_equal(la.bits(raw), la.bits(z["adv_raw"]))
        return ret.reshape(-1), val.reshape(-1), act.reshape(-1), raw.reshape(-1), z["adv_norm"].reshape(-1)
    rng = np.random.default_rng(count)
    ret = rng.normal(0.5, 2.0, count).astype(np.float32)
    val = rng.normal(0.0, 1.0, count).astype(np.float32)
    act = (rng.random(count) >= 0.2).astype(np.float32)
    act[0] = 1.0
    raw = ret - rm.dn(val, den)
    return ret, val, act, raw, rm.reference_advantages(raw, act)


# 300001: the partial kernel strides its grid (256 workgroups x 1024 elements per round) into a ragged
# tail; 2200003: the finishing launch is at its 2048-workgroup cap
@pytest.mark.parametrize("count", [3, 90, 12800, 300001, 2200003])
@pytest.mark.parametrize("den", [None, DEN], ids=["plain", "denorm"])
def test_gpu_advantages(lib, count, den):
    ret, val, act, raw, want = _advantage_case(count, den)
    x = raw.astype(np.float64)[act != 0]
    assert abs(x.mean()) <= 2 * x.std()   # the one-pass variance keeps its digits
    adv, stats = _advantages(lib, ret, val, act, den)
    print("count", count, "stats", stats, "numpy", x.mean(), x.std(), "max |adv - reference|", np.abs(adv - want).max())
    np.testing.assert_allclose(stats[:2], [x.mean(), x.std()], rtol=1e-9)
    assert stats[2] == x.size
    np.testing.assert_allclose(adv, want, rtol=1e-5, atol=1e-5)
    adv2, stats2 = _advantages(lib, ret, val, act, den)
    assert stats.tobytes() == stats2.tobytes() and adv.tobytes() == adv2.tobytes()


@pytest.mark.parametrize("count", [3, 12800])
def test_gpu_advantages_all_inactive(lib, count):
    ret, val, act, raw, _ = _advantage_case(count, None)
    adv, stats = _advantages(lib, ret, val, np.zeros_like(act), None)
    assert np.isnan(stats[0]) and np.isnan(stats[1]) and stats[2] == 0
    assert np.isnan(adv).all()


# ---- lsm_buffer_gather on synthetic arrays ----------------------------------------------------------

ROWS = 80                      # a multiple of every N below
ROW_BYTES = [4, 12, 16, 28, 140, 400, 2304]
COMPACT = [(10, 5), (16, 8), (70, 2), (72, 2)]   # 70: two mask words, 4-B units; 72: two words, 16-B units
CANARY = np.int32(-559038737)  # 0xDEADBEEF
TAIL = 8


class _Gather:
    """The synthetic source arrays on the device (built once) and one launch over all of them."""

    def __init__(self):
        import torch
        rng = np.random.default_rng(7)
        self.src_np, self.src_t, self.spec = [], [], []
        for rb in ROW_BYTES + [16]:   # the last one sits 4 bytes off a 16-byte boundary (src and dst)
            off = 1 if len(self.src_np) == len(ROW_BYTES) else 0
            a = rng.integers(-2 ** 31, 2 ** 31, (ROWS, rb // 4), dtype=np.int64).astype(np.int32)
            t = torch.zeros(off + a.size, dtype=torch.int32, device=DEV)
            t[off:] = torch.as_tensor(a.reshape(-1), device=DEV)
            self.src_np.append(a)
            self.src_t.append(t)
            self.spec.append(("rows", rb, off))
        self.compact = []
        for E, N in COMPACT:
            W = (E + 63) // 64
            A = rng.normal(0, 1, (ROWS // N, E, E)).astype(np.float32)
            A[A == 0] = 1.0   # non-zero under every set bit: a product with the mask would differ from the select
            A[0, 0, 0] = np.inf
            b = rng.random((ROWS, E)) < 0.2
            b[0, 0] = b[0, E - 1] = b[1, 1] = True
            b[2] = False
            m = np.zeros((ROWS, W), dtype=np.uint64)
            for e in range(E):
                m[:, e // 64] |= b[:, e].astype(np.uint64) << np.uint64(e % 64)
            np.testing.assert_array_equal(rm.mask_bits(m, E), b)
            self.compact.append((A, m, torch.as_tensor(A, device=DEV), torch.as_tensor(m.view(np.int64), device=DEV)))
            self.spec.append(("compact", E, N))

    def run(self, lib, indices):
        import torch
        B = len(indices)
        idx = torch.as_tensor(np.asarray(indices, dtype=np.int64), device=DEV)
        bad = torch.zeros(1, dtype=torch.int64, device=DEV)
        fields = (capi.LsmGatherField * len(self.spec))()
        dsts, want = [], []
        for k, (kind, x, y) in enumerate(self.spec):
            f = fields[k]
            if kind == "rows":
                words, off = x // 4, y
                src = self.src_t[k]
                f.kind, f.row_bytes = capi.LSM_GATHER_ROWS, x
                f.src = src.data_ptr() + 4 * off
                want.append(rm.gather_rows(self.src_np[k], indices))
            else:
                A, m, tA, tm = self.compact[k - len(self.src_np)]
                words, off = x * x, 0
                f.kind, f.E, f.N = capi.LSM_GATHER_COMPACT_ADJ, x, y
                f.src, f.masks = tA.data_ptr(), tm.data_ptr()
                want.append(rm.gather_compact_adj(A, m, indices, y).view(np.int32).reshape(B, -1))
            d = torch.full((off + B * words + TAIL,), int(CANARY), dtype=torch.int32, device=DEV)
            f.dst = d.data_ptr() + 4 * off
            dsts.append((d, off, words))
        rc = lib.lsm_buffer_gather(fields, len(self.spec), _tp(idx), B, ROWS, _tp(bad), _stream())
        assert rc == 0, lib.lsm_gather_last_error()
        torch.cuda.synchronize()
        got = []
        for (d, off, words), spec in zip(dsts, self.spec):
            a = d.cpu().numpy()
            assert (a[:off] == CANARY).all() and (a[off + B * words:] == CANARY).all(), spec
            got.append(a[off:off + B * words].reshape(B, words))
        return got, want, int(bad.cpu().numpy()[0])


@pytest.fixture(scope="module")
def gather():
    return _Gather()


# 4000: 576 000 units in the 2304-byte field, more than one grid of 2048 x 256 threads
@pytest.mark.parametrize("B", [1, 37, 300, 4000])
def test_gpu_gather_matches_numpy(lib, gather, B):
    rng = np.random.default_rng(B)
    if B == 1:
        cases = [[0], [ROWS - 1]]
    else:
        idx = rng.integers(0, ROWS, B)
        idx[[0, 1, 2, 3, B - 1]] = [0, ROWS - 1, 5, 5, 0]   # both ends, duplicates
        cases = [idx]
    for A, m, _, _ in gather.compact:   # sample 0: an inf under a set bit (a product would give NaN)
        assert np.isinf(A[0, 0, 0]) and rm.mask_bits(m[0], A.shape[-1])[0]
    for idx in cases:
        got, want, bad = gather.run(lib, idx)
        assert bad == 0
        for g, w, spec in zip(got, want, gather.spec):
            np.testing.assert_array_equal(g, w, err_msg=str(spec))


def test_gpu_gather_out_of_range_index(lib, gather):
    B = 37
    idx = np.random.default_rng(1).integers(0, ROWS, B)
    idx[3], idx[5], idx[7], idx[B - 1] = ROWS, -1, 2 ** 40, -2 ** 40
    got, want, bad = gather.run(lib, idx)
    assert bad == 1
    for g, w, spec in zip(got, want, gather.spec):
        assert (g[[3, 5, 7, B - 1]] == 0).all(), spec
        np.testing.assert_array_equal(g, w, err_msg=str(spec))


# ---- end to end: two buffers, reference and compact layout ------------------------------------------

class _Norm:
    """A value normaliser as compute_returns sees one: running_mean_var() -> 1-element tensors."""

    def running_mean_var(self):
        import torch
        return torch.tensor([2.038297]), torch.tensor([8.124851])


FIELDS = ("share_obs", "obs", "node_obs", "adj", "agent_id", "share_agent_id", "value_preds", "returns", "masks",
          "active_masks", "advantages")


@pytest.mark.parametrize("gae,proper,norm", [(True, False, "object"), (False, True, "pair"), (True, True, None)])
def test_gpu_buffer_learner_hand_off(gae, proper, norm):
    import torch
    from lsm import hj_tables
    from lsm.buffer import DeviceGraphBuffer
    from lsm.config import EnvArgs
    from lsm.vec_env import GpuGraphVecEnv, expand_compact_adj
    T, n, N = 6, 12, 8
    args = EnvArgs(num_agents=N, episode_length=T, num_env_steps=T * 4, use_safety_filter=True, seed=11)
    vt, _ = hj_tables.default_tables("double_integrator", small=True)
    envs = [GpuGraphVecEnv(args, num_envs=n, device=DEV, value_table=vt, return_numpy=False, build_infos=False,
                           adj_layout=layout) for layout in ("reference", "compact")]
    bufs = [DeviceGraphBuffer(e, episode_length=T) for e in envs]
    assert bufs[0].adj_mask is None and bufs[1].adj_mask is not None
    g = torch.Generator(device=DEV).manual_seed(5)
    for b in bufs:
        assert b.value_preds.shape == (T + 1, n, N, 1) and b.returns.shape == (T + 1, n, N, 1)
        assert not b.value_preds.any() and not b.returns.any()
        b.warmup(4)
    for t in range(T):
        a = torch.randint(0, 25, (n, N), generator=g, device=DEV, dtype=torch.int32)
        vp = torch.randn((n, N), generator=g, device=DEV)
        for b in bufs:
            b.insert_step(a, 4, value_preds=vp)
        assert torch.equal(bufs[0].value_preds[t, ..., 0], vp)
    next_value = torch.randn((n, N, 1), generator=g, device=DEV)
    vn = {"object": _Norm(), "pair": (2.5, -0.75), None: None}[norm]
    if norm == "object":
        mean, var = vn.running_mean_var()
        den = np.array([torch.sqrt(var).numpy()[0], mean.numpy()[0]], dtype=np.float32)
    else:
        den = np.array(vn, dtype=np.float32) if vn else None
    E = envs[0].E
    for b in bufs:
        b.bad_masks[2, 3, 1] = 0.0
        b.bad_masks[T, 0, 0] = 0.0
        b.active_masks[1, 2, 3] = 0.0
        b.returns[T] = float(la.SENTINEL)

    host = lambda t: t.cpu().numpy()
    ref = bufs[0]
    want_v = host(ref.value_preds).copy()
    want_r = host(ref.returns).copy()
    rm.compute_returns(host(ref.rewards), want_v, host(ref.masks), host(ref.bad_masks), host(next_value), den, want_r,
                       0.99, 0.95, gae, proper)
    raw = rm.raw_advantages(want_r, want_v, den)
    want_stats = rm.advantage_stats(raw, host(ref.active_masks)[:-1])
    want_adv = rm.normalised_advantages(raw, want_stats)
    advs = []
    for b in bufs:
        b.compute_returns(next_value, vn, gamma=0.99, gae_lambda=0.95, use_gae=gae, use_proper_time_limits=proper)
        np.testing.assert_array_equal(la.bits(host(b.returns)), la.bits(want_r))
        np.testing.assert_array_equal(la.bits(host(b.value_preds)), la.bits(want_v))
        adv, stats = b.advantages(vn)
        assert adv.shape == (T, n, N, 1) and adv.dtype == torch.float32 and stats.dtype == torch.float64
        np.testing.assert_allclose(host(stats), want_stats, rtol=1e-9)
        np.testing.assert_allclose(host(adv), want_adv, rtol=1e-5, atol=1e-5)
        advs.append(adv)
    assert host(advs[0]).tobytes() == host(advs[1]).tobytes()

    # minibatches: the same explicit permutation through both buffers
    batch = T * n * N
    perm = torch.randperm(batch, generator=torch.Generator().manual_seed(3)).to(DEV)
    k = 4
    views = {f: host(getattr(ref, f))[:-1] for f in FIELDS if f != "advantages"}
    views["advantages"] = host(advs[0])
    views = {f: v.reshape((batch,) + v.shape[3:]) for f, v in views.items()}
    got = []
    for b, adv in zip(bufs, advs):
        out = []
        for mb in b.feed_forward_generator(adv, num_mini_batch=k, indices=perm):
            assert set(mb) == set(FIELDS) | {"indices"}
            out.append({f: host(v).copy() for f, v in mb.items()})
        got.append(out)
    assert len(got[0]) == k and len(got[1]) == k
    p = host(perm)
    for i, (r, c) in enumerate(zip(got[0], got[1])):
        idx = p[i * (batch // k):(i + 1) * (batch // k)]
        np.testing.assert_array_equal(r["indices"], idx)
        for f in FIELDS + ("indices",):
            assert r[f].dtype == c[f].dtype and r[f].shape == c[f].shape, f
            assert r[f].tobytes() == c[f].tobytes(), f
        for f in FIELDS:
            assert r[f].shape == (len(idx),) + views[f].shape[1:], f
            assert r[f].tobytes() == views[f][idx].tobytes(), f
        assert r["adj"].shape == (len(idx), E, E)
    for b in bufs:
        np.testing.assert_array_equal(np.concatenate([m["indices"] for m in got[bufs.index(b)]]), p)
    # the compact buffer's expansion is the reference-layout adjacency
    full = expand_compact_adj(bufs[1].adj[:-1].reshape(T * n, E, E), bufs[1].adj_mask[:-1].reshape(T * n, N, -1), E)
    assert host(full).reshape(batch, E, E).tobytes() == views["adj"].tobytes()

    # the default permutation: a device randperm, num_mini_batch batches that cover every sample once
    for b, adv in zip(bufs, advs):
        gen = torch.Generator(device=DEV).manual_seed(9)
        idx = [host(mb["indices"]).copy() for mb in b.feed_forward_generator(adv, num_mini_batch=3, generator=gen)]
        assert len(idx) == 3
        np.testing.assert_array_equal(np.sort(np.concatenate(idx)), np.arange(batch))
    with pytest.raises(AssertionError):
        next(ref.feed_forward_generator(advs[0], num_mini_batch=batch + 1))
    for e in envs:
        e.close()
