"""ctypes helpers shared by the learner hand-off tests (include/lsm_learner.h): call the host or the
device entry points on numpy arrays and return numpy arrays, and load the reference fixtures."""
import ctypes as C
import glob
import os

import numpy as np

from lsm import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "returns")
SENTINEL = np.float32(-12345.5)


def fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    z["T"] = z["rewards"].shape[0]
    z["M"] = int(np.prod(z["rewards"].shape[1:]))
    z["den"] = z["denorm"] if int(z["use_valuenorm"]) else None
    return z


def written_rows(T, use_gae):
    """The returns rows a branch writes: 0..T-1, and T without GAE."""
    return slice(0, T) if use_gae else slice(0, T + 1)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _p(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def config(gamma, gae_lambda, use_gae, proper):
    return capi.LsmReturnsConfig(gamma=float(gamma), gae_lambda=float(gae_lambda), use_gae=int(use_gae),
                                 use_proper_time_limits=int(proper))


def compute_returns(lib, rewards, value_preds, masks, bad_masks, next_value, denorm, gamma, gae_lambda, use_gae,
                    proper, device=None):
    """Returns (returns [T+1][M] pre-filled with SENTINEL, value_preds after the call). device=None: the
    host entry point; else lsm_buffer_compute_returns on that torch device."""
    T = rewards.shape[0]
    f = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32).reshape(a.shape[0], -1).copy()
    r, v, m, b = f(rewards), f(value_preds), f(masks), f(bad_masks)
    M = r.shape[1]
    nv = np.ascontiguousarray(next_value, dtype=np.float32).reshape(M).copy()
    den = None if denorm is None else np.ascontiguousarray(denorm, dtype=np.float32).copy()
    ret = np.full((T + 1, M), SENTINEL, dtype=np.float32)
    cfg = config(gamma, gae_lambda, use_gae, proper)
    if device is None:
        rc = lib.lsm_host_compute_returns(_p(r), _p(v), _p(m), _p(b), _p(nv), _p(den), _p(ret), T, M, C.byref(cfg))
        assert rc == 0, lib.lsm_returns_last_error()
        return ret, v
    import torch
    t = lambda a: None if a is None else torch.as_tensor(a, device=device)
    tp = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    tr, tv, tm, tb, tnv, tden, tret = t(r), t(v), t(m), t(b), t(nv), t(den), t(ret)
    rc = lib.lsm_buffer_compute_returns(tp(tr), tp(tv), tp(tm), tp(tb), tp(tnv), tp(tden), tp(tret), T, M,
                                        C.byref(cfg), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.lsm_returns_last_error()
    torch.cuda.synchronize()
    return tret.cpu().numpy(), tv.cpu().numpy()
