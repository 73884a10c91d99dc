"""What the learner-side wrappers (``lsm.gnn.GraphEncoder``, ``lsm.policy.PolicyHead``, ``lsm.loss.PPOLoss``)
share: the lazy torch import, the checks of a call's device tensors, the per-(size, stream) output cache, a
call's epilogue, and the packed float32 weight blob of a state dict. Private to the package: the wrappers'
modules keep every public name.
"""
from __future__ import annotations

import numpy as np

from . import capi


def _torch():
    import torch
    return torch


def ptr(t):
    return t.data_ptr() if t is not None else None


class OutputCache:
    """Preallocated outputs by key, (size..., stream). At `limit` entries the next new key empties the cache
    first: everything, not the least recently used."""

    def __init__(self, limit: int = 8):
        self.limit = limit
        self._held = {}

    def get(self, key, make):
        out = self._held.get(key)
        if out is None:
            if len(self._held) >= self.limit:
                self._held.clear()
            out = self._held[key] = make()
        return out


def pack_entries(state_dict, entries, prefix, may_be_absent, expected_floats, error_class, fn_name):
    """The packed float32 blob of state_dict's entries [(name without prefix, shape)] (tensors or arrays), in
    their order. A missing or mis-shaped entry is refused by name as error_class("<fn_name>: ..."), except one
    whose name contains may_be_absent (None: none may be): its weight is filled with 1, its bias with 0.
    expected_floats() is the library's count, asked for after the entries were packed."""
    parts = []
    for name, shape in entries:
        key = prefix + name
        if key not in state_dict:
            if may_be_absent and may_be_absent in name:
                parts.append(np.full(shape, 1.0 if name.endswith("weight") else 0.0, np.float32).reshape(-1))
                continue
            raise error_class("%s: %s is missing from the state dict" % (fn_name, key))
        v = state_dict[key]
        a = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        if tuple(a.shape) != shape:
            raise error_class("%s: %s has shape %s, the config needs %s" % (fn_name, key, tuple(a.shape), shape))
        parts.append(np.ascontiguousarray(a, dtype=np.float32).reshape(-1))
    blob = np.concatenate(parts)
    if blob.size != expected_floats():
        raise error_class("%s: %d floats packed, the library expects %d" % (fn_name, blob.size, expected_floats()))
    return blob


def unpack_entries(blob, entries, prefix, left_out, expected_floats, error_class, fn_name):
    """The inverse of pack_entries: {prefix + name: float32 array}, without the entries whose name contains
    left_out (None: with all of them)."""
    blob = np.asarray(blob, dtype=np.float32).reshape(-1)
    if blob.size != expected_floats():
        raise error_class("%s: blob of %d floats, the config needs %d" % (fn_name, blob.size, expected_floats()))
    out, o = {}, 0
    for name, shape in entries:
        n = int(np.prod(shape))
        if not (left_out and left_out in name):
            out[prefix + name] = blob[o:o + n].reshape(shape).copy()
        o += n
    return out


class DeviceOp:
    """One wrapper's device side: ``lib``, ``device``, the bad-input word ``bad`` and, with _alloc_weights,
    the weight blob ``weights``. error_class is what every refusal raises, who the class's name in the
    constructor's refusal, noun what the wrapper calls itself in a device mismatch."""

    def __init__(self, device, error_class, who, noun):
        torch = self._torch = _torch()   # kept: _tensor and _stream run several times per call
        self.device = torch.device(device)
        self._error, self._noun = error_class, noun
        if self.device.type != "cuda":
            raise error_class("%s needs a CUDA (HIP) device; there is no CPU fallback" % who)
        self.lib = capi.load_library()
        self.bad = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _alloc_weights(self, n, blob):
        torch = _torch()
        self._n = n
        self.weights = torch.empty(n, dtype=torch.float32, device=self.device)
        self._set(blob)

    def _set(self, blob):
        torch = _torch()
        if isinstance(blob, torch.Tensor):
            src = blob.detach().reshape(-1).to(torch.float32)
        else:
            src = torch.from_numpy(np.ascontiguousarray(blob, dtype=np.float32).reshape(-1))
        if src.numel() != self._n:
            raise self._error("weight blob of %d floats, the config needs %d" % (src.numel(), self._n))
        self.weights.copy_(src, non_blocking=True)   # the one device copy, on the current stream

    def _stream(self):
        """The raw handle of the current stream on self.device."""
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _tensor(self, t, name, numel=None, dtype=None, shape=None, detach=False):
        """t, contiguous, after the checks: a CUDA tensor, on self.device, of dtype (None: float32) and
        either of `shape` or, shape None, of `numel` values."""
        torch = self._torch
        if dtype is None:
            dtype = torch.float32
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise self._error("%s must be a CUDA (HIP) tensor; there is no CPU fallback" % name)
        if t.device != self.device:
            raise self._error("%s is on %s, the %s on %s" % (name, t.device, self._noun, self.device))
        if shape is not None:
            if t.dtype != dtype or tuple(t.shape) != tuple(shape):
                raise self._error("%s must be %s %s, got %s %s" % (name, dtype, tuple(shape), t.dtype, tuple(t.shape)))
        elif t.dtype != dtype or t.numel() != numel:
            raise self._error("%s must hold %d float32 values, got %s %s" % (name, numel, t.dtype, tuple(t.shape)))
        if detach:
            t = t.detach()
        return t if t.is_contiguous() else t.contiguous()

    def _finish(self, rc, last_error, check, bad_text):
        """A call's epilogue: the library's refusal, then (check: one synchronisation) the bad-input word."""
        if rc != 0:
            raise self._error(last_error().decode())
        if check and int(self.bad.item()):
            self.bad.zero_()
            raise self._error(bad_text)
