"""What lsm/_device.py gives the encoder, head and loss wrappers, without a GPU: the output cache's policy, the
weight blob's pack / unpack on a small entry table, and each wrapper's refusal of a CPU device in its own error
class and words."""
import numpy as np
import pytest

from lsm import _device, gnn, loss, policy


class BlobError(RuntimeError):
    pass


def test_output_cache_keeps_eight_keys_and_empties_itself_for_the_ninth():
    cache = _device.OutputCache()
    made = []

    def make(k):
        made.append(k)
        return object()

    first = [cache.get(k, lambda k=k: make(k)) for k in range(8)]
    assert made == list(range(8))
    for k in range(8):   # all eight are held, the 8th too: nothing is made again
        assert cache.get(k, lambda k=k: make(k)) is first[k]
    assert made == list(range(8))
    ninth = cache.get(8, lambda: make(8))   # the 9th key empties the cache first: everything, not the oldest
    assert cache.get(8, lambda: make(8)) is ninth and made == list(range(9))
    for k in (7, 0):
        assert cache.get(k, lambda k=k: make(k)) is not first[k]
    assert made == list(range(9)) + [7, 0]


def test_output_cache_calls_make_once_per_key():
    cache = _device.OutputCache(limit=2)
    calls = []
    a = cache.get(("M", 1), lambda: calls.append(1) or [1])
    assert cache.get(("M", 1), lambda: calls.append(1) or [1]) is a and calls == [1]


ENTRIES = [("lin.weight", (2, 3)), ("norm.weight", (3,)), ("norm.bias", (3,))]


def _pack(sd, absent="norm.", floats=12, prefix="p."):
    return _device.pack_entries(sd, ENTRIES, prefix, absent, lambda: floats, BlobError, "pack_things")


def _unpack(blob, absent="norm.", floats=12, prefix="p."):
    return _device.unpack_entries(blob, ENTRIES, prefix, absent, lambda: floats, BlobError, "unpack_things")


def test_pack_and_unpack_round_trip_and_fill_the_absent_entries():
    rng = np.random.default_rng(0)
    full = {"p." + k: rng.normal(size=s).astype(np.float32) for k, s in ENTRIES}
    blob = _pack(full, absent=None)
    assert blob.dtype == np.float32 and blob.shape == (12,)
    assert blob.tobytes() == b"".join(full["p." + k].tobytes() for k, _ in ENTRIES)
    back = _unpack(blob, absent=None)
    assert list(back) == ["p." + k for k, _ in ENTRIES]
    assert all(back[k].shape == full[k].shape and back[k].tobytes() == full[k].tobytes() for k in full)
    assert _pack(back, absent=None).tobytes() == blob.tobytes()
    # the entries that may be absent: weight 1, bias 0 in the blob, and left out on the way back
    lin = {"p.lin.weight": full["p.lin.weight"]}
    blob = _pack(lin)
    assert blob.tobytes() == full["p.lin.weight"].tobytes() + np.array([1, 1, 1, 0, 0, 0], np.float32).tobytes()
    assert list(_unpack(blob)) == ["p.lin.weight"]
    assert _pack(_unpack(blob)).tobytes() == blob.tobytes()
    # present entries are packed even where they might be absent; torch tensors as well as arrays
    import torch
    assert _pack({k: torch.from_numpy(v) for k, v in full.items()}).tobytes() == _pack(full, absent=None).tobytes()


def test_pack_and_unpack_refuse_by_name_with_the_callers_function_name():
    full = {"p." + k: np.zeros(s, np.float32) for k, s in ENTRIES}
    with pytest.raises(BlobError) as e:
        _pack({k: v for k, v in full.items() if k != "p.lin.weight"})
    assert str(e.value) == "pack_things: p.lin.weight is missing from the state dict"
    with pytest.raises(BlobError) as e:   # nothing may be absent: the norm's entry is missed by name
        _pack({k: v for k, v in full.items() if k != "p.norm.bias"}, absent=None)
    assert str(e.value) == "pack_things: p.norm.bias is missing from the state dict"
    with pytest.raises(BlobError) as e:
        _pack(dict(full, **{"p.norm.weight": np.zeros((3, 1), np.float32)}))
    assert str(e.value) == "pack_things: p.norm.weight has shape (3, 1), the config needs (3,)"
    with pytest.raises(BlobError) as e:
        _pack(full, floats=13)
    assert str(e.value) == "pack_things: 12 floats packed, the library expects 13"
    with pytest.raises(BlobError) as e:
        _unpack(np.zeros(11, np.float32))
    assert str(e.value) == "unpack_things: blob of 11 floats, the config needs 12"


@pytest.mark.parametrize("make, error, text", [
    (lambda: gnn.GraphEncoder(gnn.GnnConfig(F=7), None, "cpu"), gnn.GnnError,
     "GraphEncoder needs a CUDA (HIP) device; there is no CPU fallback"),
    (lambda: policy.PolicyHead(policy.HeadConfig(kind="actor", in0=6, in1=16, num_actions=25), None, "cpu"),
     policy.PolicyError, "PolicyHead needs a CUDA (HIP) device; there is no CPU fallback"),
    (lambda: loss.PPOLoss(loss.LossConfig(num_actions=25), "cpu"), loss.LossError,
     "PPOLoss needs a CUDA (HIP) device; there is no CPU fallback"),
], ids=["GraphEncoder", "PolicyHead", "PPOLoss"])
def test_a_cpu_device_is_refused_in_the_wrappers_own_class_and_words(make, error, text):
    with pytest.raises(error) as e:
        make()
    assert type(e.value) is error and str(e.value) == text
    assert len({gnn.GnnError, policy.PolicyError, loss.LossError}) == 3
