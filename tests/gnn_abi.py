"""ctypes helpers shared by the graph-encoder tests (include/lsm_gnn.h): one case's inputs in both
adjacency layouts (tests/mb_edges_abi.py's Source, on the host or on a torch device), a canaried output,
and the two entry points behind one call."""
import ctypes as C

import numpy as np

import mb_edges_abi as mb
import recurrent_abi as ra
import recurrent_model as rcm

LAYOUTS = ("reference", "compact")


def sources(table, bits, N, device=None):
    """{"reference", "compact"}: the compact statement (table [B / N, E, E], bits [B, E]) and the dense
    [B, E, E] matrices it stands for (Source.full, the oracle's expand_compact), placed on `device`."""
    cmp_ = mb.Source(table, rcm.pack_bits(bits), N, device)
    return {"reference": mb.Source(cmp_.full, device=device), "compact": cmp_}


def dense_sources(full, device=None):
    """Both layouts of given dense matrices [B, E, E]: the compact one has N = 1, a table equal to the
    matrix, and the disconnect bit of every node without any edge set, with inf in the table under it."""
    full = np.ascontiguousarray(full, dtype=np.float32)
    alone = ~((full != 0).any(axis=1) | (full != 0).any(axis=2))          # [B, E]
    under = alone[:, :, None] | alone[:, None, :]
    out = sources(np.where(under, np.float32(np.inf), full), alone, 1, device)
    np.testing.assert_array_equal(out["compact"].full, full)   # by value: a lone node's -0.0 comes back as +0.0
    return out


def _ptr(p):
    return C.c_void_p(p.ptr) if p is not None else None


def run(lib, cfg, blob, node_obs, src, agent_id=None, bad_init=0, expect_rc=0, over=None):
    """lsm_host_gnn_forward (src.device is None) or lsm_gnn_forward on src.device, with the output between
    canaries. Returns (out [B, out_dim] float32, bad). over: replace arguments (B, E, N, or a pointer
    name set to None) for the refusal tests; with expect_rc != 0 returns the raw output words."""
    dev = src.device
    node_obs = np.ascontiguousarray(node_obs, dtype=np.float32)
    B, E = node_obs.shape[0], src.E
    D = cfg.out_dim
    w = ra.Placed(np.ascontiguousarray(blob, dtype=np.float32).view(np.int32), 0, dev)
    x = ra.Placed(node_obs.view(np.int32), 0, dev) if node_obs.size else None
    aid = None
    if agent_id is not None:
        aid = ra.Placed(np.ascontiguousarray(agent_id, dtype=np.int64).reshape(-1).view(np.int32), 0, dev)
    dst = ra.destination(max(B * D, 1), 0, dev)
    bad = ra.Placed(np.array([bad_init], np.int64).view(np.int32), 0, dev)
    args = dict(cfg=cfg.struct(), weights=_ptr(w), node_obs=_ptr(x), adj=_ptr(src.adj), masks=_ptr(src.masks),
                B=B, E=E, N=src.N, agent_id=_ptr(aid), out=C.c_void_p(dst[0].ptr + 4 * ra.PRE), bad=_ptr(bad))
    args.update(over or {})
    order = ("cfg", "weights", "node_obs", "adj", "masks", "B", "E", "N", "agent_id", "out", "bad")
    if dev is None:
        rc = lib.lsm_host_gnn_forward(*[args[k] for k in order])
    else:
        import torch
        rc = lib.lsm_gnn_forward(*[args[k] for k in order], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_gnn_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    words = ra.read_destination(dst, "gnn out")
    badv = int(bad.read().view(np.int64)[0])
    if expect_rc:
        assert err.startswith("gnn: ") and len(err) > len("gnn: "), err
        assert (words == ra.CANARY).all() and badv == bad_init, "a refused call wrote"
        return words, badv
    if B * D == 0:
        assert (words == ra.CANARY).all()
    return words[:B * D].view(np.float32).reshape(B, D).copy(), badv
