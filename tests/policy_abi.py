"""ctypes helpers shared by the policy-head tests (include/lsm_policy.h): one call's inputs on the host or
on a torch device (tests/recurrent_abi.py's Placed), every requested output between canaries, and the two
entry points behind one call."""
import ctypes as C

import numpy as np

import recurrent_abi as ra
from lsm import capi

ACTOR_OUT = ("actions_i32", "actions_f32", "log_probs", "logits", "features", "rnn_out")
CRITIC_OUT = ("values", "features", "rnn_out")
INPUTS = {"x0": "x0", "x1": "x1", "states": "rnn_states", "masks": "masks", "u": "u", "avail": "available_actions"}


def out_shapes(cfg, M):
    return {"actions_i32": (M,), "actions_f32": (M,), "log_probs": (M,), "logits": (M, cfg.num_actions or 1),
            "values": (M,), "features": (M, cfg.hidden), "rnn_out": (M, cfg.recurrent_N, cfg.hidden)}


def default_outputs(cfg):
    names = ACTOR_OUT if cfg.kind == "actor" else CRITIC_OUT
    return tuple(n for n in names if n != "rnn_out" or cfg.recurrent_N)


def run(lib, cfg, blob, inp, device=None, outputs=None, mode=False, bad_init=0, expect_rc=0, over=None, add=None,
        alias=None):
    """lsm_host_head_forward (device None) or lsm_head_forward on `device`. inp: tests/policy_model.py's
    input dict; mode=True passes u = NULL. outputs: the names to request (the others are passed as NULL).
    Returns ({name: array}, bad). over: replace io fields (by their header name), or 'cfg' / 'weights' /
    'M' / 'io', for the refusal tests; add: {field or 'weights': bytes added to that pointer}; alias: (field,
    other field, bytes): the field points into the other's array. With expect_rc != 0 the outputs must
    hold their canaries."""
    M = int(inp["x1"].shape[0])
    outputs = default_outputs(cfg) if outputs is None else tuple(outputs)
    keep = [ra.Placed(np.ascontiguousarray(blob, dtype=np.float32), 0, device)]
    io = capi.LsmHeadIo()
    for key, field in INPUTS.items():
        a = inp.get(key)
        if a is None or (key == "u" and mode) or np.asarray(a).size == 0:
            continue
        p = ra.Placed(np.ascontiguousarray(a, dtype=np.float32), 0, device)
        keep.append(p)
        setattr(io, field, p.ptr)
    shapes = out_shapes(cfg, M)
    dsts = {}
    for name in outputs:
        d = ra.destination(max(int(np.prod(shapes[name])), 1), 0, device)
        dsts[name] = d
        setattr(io, name, d[0].ptr + 4 * ra.PRE)
    bad = ra.Placed(np.array([bad_init], np.int64), 0, device)
    io.bad = bad.ptr
    args = dict(cfg=cfg.struct() if hasattr(cfg, "struct") else cfg, weights=C.c_void_p(keep[0].ptr), io=C.byref(io), M=M)
    for k, v in (over or {}).items():
        if k in args:
            args[k] = v
        else:
            setattr(io, k, v)
    for k, v in (add or {}).items():
        if k == "weights":
            args["weights"] = C.c_void_p(keep[0].ptr + v)
        else:
            setattr(io, k, getattr(io, k) + v)
    if alias:
        setattr(io, alias[0], getattr(io, alias[1]) + alias[2])
    if device is None:
        rc = lib.lsm_host_head_forward(args["cfg"], args["weights"], args["io"], args["M"])
    else:
        import torch
        rc = lib.lsm_head_forward(args["cfg"], args["weights"], args["io"], args["M"],
                                  C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_policy_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    badv = int(bad.read().view(np.int64)[0])
    got = {}
    for name, d in dsts.items():
        words = ra.read_destination(d, "head " + name)
        n = int(np.prod(shapes[name]))
        if expect_rc or n == 0:
            assert (words == ra.CANARY).all(), "a refused or empty call wrote %s" % name
            continue
        got[name] = words[:n].view(np.int32 if name == "actions_i32" else np.float32).reshape(shapes[name]).copy()
    if expect_rc:
        assert err.startswith("head: ") and len(err) > len("head: "), err
        assert badv == bad_init, "a refused call wrote bad"
    return got, badv
