"""include/lsm_train_info.h restated in numpy float64, and its cases, shared by tests/test_train_info_capi.py
(lsm_host_train_info_add / _mean on host memory) and tests/test_gpu_trainer.py (the kernels): `run` lays a sequence
of updates out with the state and `out` between canaries, calls the library and returns what it left; `model` is
what the header says it must be. The arithmetic is one float64 addition per slot and call, in call order, and one
division, so the comparison is bit for bit; where a sum is NaN its place is compared, not the NaN's sign and
payload (they depend on how each side propagates a NaN operand, as in include/lsm_optim.h)."""
import ctypes as C

import numpy as np

from lsm import capi

SLOTS, MEANS, WORDS = capi.LSM_TRAIN_INFO_SLOTS, capi.LSM_TRAIN_INFO_MEANS, capi.LSM_TRAIN_INFO_STATE_WORDS
ACTOR = (1, 2, 3, 5, 6)    # the slots that are null with update_actor=False
CRITIC = (0, 4, 7)
CANARY64 = np.int64(0x5A5A5A5A5A5A5A5A)
CANARY32 = np.float32(-7.25)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def value_bits(a):
    """a's bits with every NaN mapped to one pattern."""
    a = np.ascontiguousarray(a)
    b = bits(a).copy()
    if a.dtype.kind == "f":
        b[np.isnan(a)] = bits(np.array([np.nan], a.dtype))[0]
    return b


def model(seq, num_updates, acc=np.float64):
    """The header: seq is a list of updates, each a list of SLOTS values (np.float32 or None); the first update
    starts the state. acc=np.float32: the accumulator the header does not use, for the contrast."""
    s, n = np.zeros(SLOTS, acc), np.zeros(SLOTS, np.int64)
    updates, first_nonfinite = 0, -1
    with np.errstate(all="ignore"):
        for upd in seq:
            bad = False
            for k, x in enumerate(upd):
                if x is None:
                    continue
                x = np.float32(x)
                s[k] = s[k] + acc(x)
                n[k] += 1
                bad = bad or not np.isfinite(x)
            if first_nonfinite == -1 and bad:
                first_nonfinite = updates
            updates += 1
        out = np.empty(SLOTS, np.float32)
        out[:MEANS] = (s[:MEANS].astype(np.float64) / np.float64(num_updates)).astype(np.float32)
        out[MEANS:] = s[MEANS:].astype(np.float32)
    return dict(sum=s.astype(np.float64), n=n, updates=np.int64(updates), first_nonfinite=np.int64(first_nonfinite),
                out=out)


def _src(ptrs):
    src = capi.LsmTrainInfoSrc()
    for k, p in enumerate(ptrs):
        src.value[k] = p
    return src


def run(lib, seq, num_updates, dev=None, stream=None, garbage=None):
    """The sequence through the library: every update's values in one float32 array (a canary between any two),
    the state and out between canaries. garbage: the int64 words the state holds before the first call (default:
    a NaN bit pattern in every word). dev None: the host entry points. Returns model()'s dict."""
    vals = np.full((len(seq), 2 * SLOTS + 1), CANARY32, np.float32)    # value k of update u at [u, 2 * k + 1]
    for u, upd in enumerate(seq):
        for k, x in enumerate(upd):
            if x is not None:
                vals[u, 2 * k + 1] = np.float32(x)
    state = np.full(WORDS + 2, CANARY64, np.int64)
    state[1:-1] = np.int64(0x7FF8DEADBEEF0001) if garbage is None else garbage
    out = np.full(SLOTS + 2, CANARY32, np.float32)
    vals0 = vals.copy()
    if dev is None:
        held = (vals, state, out)
        addr = lambda a: a.ctypes.data
    else:
        import torch
        held = tuple(torch.from_numpy(a).to(dev) for a in (vals, state, out))
        addr = lambda t: t.data_ptr()
    sp, op = C.c_void_p(addr(held[1]) + 8), C.c_void_p(addr(held[2]) + 4)
    srcs = [_src([addr(held[0]) + 4 * (u * vals.shape[1] + 2 * k + 1) if x is not None else None
                  for k, x in enumerate(upd)]) for u, upd in enumerate(seq)]
    err = lambda: lib.lsm_train_info_last_error().decode()
    if dev is None:
        for u, src in enumerate(srcs):
            assert lib.lsm_host_train_info_add(sp, src, int(u == 0)) == 0, err()
        assert lib.lsm_host_train_info_mean(sp, num_updates, op) == 0, err()
    else:
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
            sh = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for u, src in enumerate(srcs):
                assert lib.lsm_train_info_add(sp, src, int(u == 0), sh) == 0, err()
            assert lib.lsm_train_info_mean(sp, num_updates, op, sh) == 0, err()
        torch.cuda.synchronize(dev)
        vals, state, out = (t.cpu().numpy() for t in held)
    assert state[0] == CANARY64 and state[-1] == CANARY64, "the state's neighbours were written"
    assert out[0] == CANARY32 and out[-1] == CANARY32, "out's neighbours were written"
    np.testing.assert_array_equal(bits(vals), bits(vals0), "the sources were written")
    w = state[1:-1]
    return dict(sum=w[:SLOTS].view(np.float64).copy(), n=w[SLOTS:2 * SLOTS].copy(), updates=w[2 * SLOTS],
                first_nonfinite=w[2 * SLOTS + 1], out=out[1:-1].copy())


def same(got, want, what):
    for k in ("sum", "n", "updates", "first_nonfinite", "out"):
        np.testing.assert_array_equal(value_bits(np.asarray(got[k])), value_bits(np.asarray(want[k])),
                                      "%s: %s" % (what, k))


def randoms(updates, seed, pattern=None):
    """updates x SLOTS random scalars of a train_info's magnitudes; pattern(u): the non-null slots of update u."""
    rng = np.random.default_rng(seed)
    scale = np.array([1e-2, 1e-3, 3.2, 0.7, 11.0, 1.0, 1.0, 1.0], np.float64)
    seq = []
    for u in range(updates):
        x = (scale * rng.standard_normal(SLOTS)).astype(np.float32)
        x[MEANS:] = rng.integers(0, 2, 2)    # the skip flags are 0 or 1
        keep = range(SLOTS) if pattern is None else pattern(u)
        seq.append([x[k] if k in keep else None for k in range(SLOTS)])
    return seq


def cancel_case(values=(1e20, -1e20, 1.0)):
    """1e20, -1e20, 1 in every mean slot: the sum is 1 in any accumulator (the first two cancel exactly before
    the 1 arrives). absorb_case() is the order and the magnitude at which the accumulator's width shows."""
    return [[np.float32(v) if k < MEANS else np.float32(0) for k in range(SLOTS)] for v in values]


def absorb_case():
    """1e10, 1, -1e10: a float32 accumulator absorbs the 1 into 1e10 (its ulp there is 1024) and ends at 0;
    float64 (ulp 2e-6) keeps it. At 1e20 a float64 would absorb it too (ulp 16384)."""
    return cancel_case((1e10, 1.0, -1e10))


def nonfinite_case():
    """Five updates: a NaN in slot 1 of update 2 (0-based), an inf in slot 4 of update 3."""
    seq = randoms(5, 41)
    seq[2][1] = np.float32(np.nan)
    seq[3][4] = np.float32(np.inf)
    return seq


GARBAGE = np.array([0x7FF8000000000001, -1, 0x7FF0000000000000, 0xFFF8000000000000 - (1 << 64), 12345, -(1 << 62),
                    0x7FF8DEADBEEF0001, 1] * 3, np.int64)[:WORDS]

# name -> (the updates, num_updates, the state's words before the first call)
CASES = {
    "one_update": (randoms(1, 1), 1, None),
    "two_updates": (randoms(2, 2), 2, None),
    "seven_updates": (randoms(7, 3), 7, None),
    "critic_only": (randoms(3, 4, lambda u: CRITIC), 3, None),
    "actor_every_other_update": (randoms(4, 5, lambda u: range(SLOTS) if u % 2 == 0 else CRITIC), 4, None),
    "critic_only_first": (randoms(3, 6, lambda u: CRITIC if u == 0 else range(SLOTS)), 3, None),
    "one_slot_each": (randoms(8, 7, lambda u: (u,)), 8, None),
    "over_garbage": (randoms(3, 8, lambda u: CRITIC if u == 0 else range(SLOTS)), 3, GARBAGE),
    "over_zeros": (randoms(2, 9), 2, np.zeros(WORDS, np.int64)),
    "cancellation": (cancel_case(), 3, None),
    "absorption": (absorb_case(), 3, None),
    "nonfinite": (nonfinite_case(), 5, None),
    "more_updates_than_adds": (randoms(3, 10), 4, None),
    "fewer_updates_than_adds": (randoms(5, 11), 2, None),
}


def check_case(runner, name):
    seq, num, garbage = CASES[name]
    same(runner(seq, num, garbage=garbage), model(seq, num), name)
