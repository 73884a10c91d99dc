"""The heads' backward tests' cases and checks (shared by tests/test_heads_backward_capi.py on the host entry
point and tests/test_gpu_heads_backward.py on the kernels), with tests/heads_backward_model.py's two models
computed once per case, and the ctypes call: inputs on the host or on a torch device (tests/recurrent_abi.py's
Placed), every output and the workspace between canaries.

Tolerance: the project's rule per gradient tensor (each named weight entry, dx0, dx1),
max |out - truth64| <= 4 * e32 + 4 * 2^-23 * max |truth64| (policy_model.tensor_bound), from the two models
alone.

Which inputs make a case, decided from the float64 model alone (and the float32 torch model's signs), the
first seed that qualifies:
1. no row above evaluate_cases.MAX_AMP (that file's rule, for its stated reason);
2. no ReLU pre-activation within 2^-17 of 0, and the float32 torch model on the same side of 0 as the
   float64 model everywhere: the gradient jumps at 0, and one flipped unit is an O(1) change in a row's
   gradient, which no rounding bound covers.
No row is left out of any comparison."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import evaluate_cases as ec
import evaluate_model as em
import heads_backward_model as hm
import launch_plans as lp
import policy_cases as pc
import policy_model as pm
import recurrent_abi as ra
from lsm import capi, policy

ACTOR, CRITIC = pc.ACTOR, pc.CRITIC
SHAPES = ec.SHAPES
OPTION_C, OPTION_T = 65, 3
SLAB = capi.LSM_BWD_SLAB
NEAR = 2.0 ** -17
INPUTS = {"x0": "x0", "x1": "x1", "states": "rnn_states", "masks": "masks", "avail": "available_actions"}
SMALL = dict(hidden=8, in0=3, in1=4)     # the slab-boundary and structure cases: fast on the host


def seed_rows(cfg, R, seed):
    """The gradient at the head's output: N(0, 1) / R, [R, A] or [R]."""
    rng = np.random.default_rng(50000 + seed)
    shape = (R, cfg.num_actions) if cfg.kind == "actor" else (R,)
    return (rng.normal(size=shape) / R).astype(np.float32)


def run(lib, cfg, blob, inp, seed, Cn, T, device=None, dx=(True, True), expect_rc=0, over=None, add=None, alias=None,
        workspace=False):
    """lsm_host_head_backward (device None) or lsm_head_backward on `device`. Returns {dweights, dx0, dx1} (the
    requested ones). over: replace io fields (by their header name), or 'cfg' / 'weights' / 'C' / 'T' / 'io';
    add: {field or 'weights': bytes added to that pointer}; alias: (field, other field, bytes). With
    expect_rc != 0 every output and the workspace must hold their canaries and the text must start with
    "backward: "."""
    st = cfg.struct() if hasattr(cfg, "struct") else cfg
    keep = [ra.Placed(np.ascontiguousarray(blob, dtype=np.float32), 0, device)]
    io = capi.LsmBwdIo()
    for key, field in INPUTS.items():
        a = inp.get(key)
        if a is None or np.asarray(a).size == 0:
            continue
        p = ra.Placed(np.ascontiguousarray(a, dtype=np.float32), 0, device)
        keep.append(p)
        setattr(io, field, p.ptr)
    if seed is not None:
        p = ra.Placed(np.ascontiguousarray(seed, dtype=np.float32), 0, device)
        keep.append(p)
        setattr(io, "dlogits" if st.kind == capi.LSM_HEAD_ACTOR else "dvalues", p.ptr)
    R = max(Cn, 0) * max(T, 0)
    nw = int(lib.lsm_head_weights_floats(st))
    sizes = {"dweights": nw}
    if dx[0] and st.in0:
        sizes["dx0"] = R * st.in0
    if dx[1] and st.in1:
        sizes["dx1"] = R * st.in1
    wsb = int(lib.lsm_head_backward_workspace_bytes(st, max(Cn, 0), max(T, 1)))
    sizes["workspace"] = max(wsb, 8) // 4
    dsts = {}
    for name, n in sizes.items():
        if expect_rc:
            n = min(n, 64)        # a refused call writes nothing: a few words show it (T * C may be 2^31)
        d = ra.destination(max(n, 1), 0, device)
        dsts[name] = d
        setattr(io, name, d[0].ptr + 4 * ra.PRE)
    assert ra.PRE % 2 == 0      # the workspace is 8-byte aligned
    args = dict(cfg=st, weights=C.c_void_p(keep[0].ptr), io=C.byref(io), C=Cn, T=T)
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
        rc = lib.lsm_host_head_backward(args["cfg"], args["weights"], args["io"], args["C"], args["T"])
    else:
        import torch
        rc = lib.lsm_head_backward(args["cfg"], args["weights"], args["io"], args["C"], args["T"],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_policy_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    got = {}
    for name, d in dsts.items():
        words = ra.read_destination(d, "backward " + name)
        if expect_rc or Cn == 0:
            assert (words == ra.CANARY).all(), "a refused or empty call wrote %s" % name
            continue
        if name != "workspace" and sizes[name]:
            got[name] = words[:sizes[name]].view(np.float32).copy()
        if name == "workspace" and workspace:
            got[name] = words            # every word the call was given (workspace=True: the raw int32 words)
    if expect_rc:
        assert err.startswith("backward: ") and len(err) > len("backward: "), err
    else:
        if "dx0" in got:
            got["dx0"] = got["dx0"].reshape(R, st.in0)
        if "dx1" in got:
            got["dx1"] = got["dx1"].reshape(R, st.in1)
    return got


def same_side(pre64, pre32):
    """Rule 2 above."""
    for a, b in zip(pre64, pre32):
        if np.abs(a).min() < NEAR or ((a > 0) != (b > 0)).any():
            return False
    return True


class Case:
    def __init__(self, name, cfg, Cn, T, seed=0, **kw):
        self.name, self.cfg, self.C, self.T, self.R, self.seed = name, cfg, Cn, T, Cn * T, seed
        self.sd, self.blob = pc.weights(cfg, seed)
        self.inp = em.random_inputs(cfg, Cn, T, seed, **kw)
        self.dout = seed_rows(cfg, self.R, seed)
        self.g64 = hm.model64(cfg, self.sd, self.inp, self.dout, Cn, T)
        self.g32 = hm.model32(cfg, self.sd, self.inp, self.dout, Cn, T)
        self.names = [k for k in self.g64 if k not in ("out", "pre")]
        self.tol = {k: pm.tensor_bound(self.g64[k], self.g32[k]) for k in self.names}

    def admissible(self):
        amp = em.model64(self.cfg, self.sd, self.inp, self.C, self.T)["amp"].max()
        return amp <= ec.MAX_AMP and (not self.cfg.relu or same_side(self.g64["pre"], self.g32["pre"]))


def admitted(name, cfg, Cn, T, seed, **kw):
    for s in range(seed, seed + 50):
        case = Case(name, cfg, Cn, T, seed=s, **kw)
        if case.admissible():
            return case
    raise AssertionError("%s: no admissible seed" % name)


@functools.lru_cache(maxsize=None)
def shape_case(kind, Cn, T):
    return admitted("%s C%d T%d" % (kind, Cn, T), ACTOR if kind == "actor" else CRITIC, Cn, T, (Cn + T) % 7)


@functools.lru_cache(maxsize=None)
def option_case(name):
    base, over = ec.OPTIONS[name]
    return admitted("option " + name, dataclasses.replace(base, **over), OPTION_C, OPTION_T,
                    1 + sorted(ec.OPTIONS).index(name))


@functools.lru_cache(maxsize=None)
def plan_case(name):
    """evaluate_cases.PLAN_OPTIONS for the backward: a 'max' is the backward's own limit (lsm_head_plan)."""
    return admitted("plan " + name, ec.plan_cfg(name, "backward"), OPTION_C, ec.plan_T(name),
                    30 + sorted(ec.PLAN_OPTIONS).index(name))


def plan_of(name):
    return lp.head_plan(ec.plan_cfg(name, "backward"), "backward", OPTION_C, ec.plan_T(name))[0]


def plan_checks(lib, name, device):
    """The case against the model; a case at an LDS limit also shows the next size refused, nothing written."""
    case = plan_case(name)
    check(lib, case, device)
    past = ec.beyond(name, "backward") if name in ec.PLAN_LIMITS else None
    if past is not None:
        run(lib, past, np.zeros(400000, np.float32), em.random_inputs(past, 1, 1, 0), seed_rows(past, 1, 0), 1, 1,
            device, expect_rc=1)
        assert "bytes of LDS" in lib.lsm_policy_last_error().decode()


def forward_is_evaluates(lib, case, device):
    """Stage 1 of lsm_head_backward is lsm_head_evaluate's forward (the header's "the gradient is that of the
    function lsm_head_evaluate computes"): on the same inputs the features it saved, and the last GRU layer's
    h' at step T - 1, are evaluate's `features` and `rnn_out` to the byte. They are found in the workspace by
    the header's layout ([T*C][hidden] arrays) at the offsets lsm_head_plan reports; the words behind the
    documented size keep their canaries (run() checks the canaries around the buffer as well)."""
    cfg, Cn, T, R, Hd, RN = case.cfg, case.C, case.T, case.R, case.cfg.hidden, case.cfg.recurrent_N
    assert RN > 0
    ev, _ = ec.run(lib, cfg, case.blob, case.inp, Cn, T, device, outputs=("features", "rnn_out"), scratch=False)
    got = run(lib, cfg, case.blob, case.inp, case.dout, Cn, T, device, workspace=True)
    ws = got["workspace"]
    plan = lp.head_plan(cfg, "backward", Cn, T)[0]
    assert len(ws) - plan["ws_floats"] in (0, 1) and (ws[plan["ws_floats"]:] == ra.CANARY).all()
    assert not (ws[:plan["ws_floats"]] == ra.CANARY).all()
    feat = ws[plan["o_feat"]:plan["o_feat"] + R * Hd].reshape(R, Hd)
    np.testing.assert_array_equal(feat, ev["features"].view(np.int32), err_msg="the saved features")
    top = plan["o_ho"][RN - 1]
    last = ws[top:top + R * Hd].reshape(T, Cn, Hd)[T - 1]
    np.testing.assert_array_equal(last, ev["rnn_out"][:, RN - 1].view(np.int32), err_msg="h' at step T - 1")
    if RN == 2:
        low = ws[plan["o_ho"][0]:plan["o_ho"][0] + R * Hd].reshape(T, Cn, Hd)[T - 1]
        np.testing.assert_array_equal(low, ev["rnn_out"][:, 0].view(np.int32), err_msg="layer 0's h' at step T - 1")
    compare({k: v for k, v in got.items() if k != "workspace"}, case, "backward %s" % case.name)


def forward_cases():
    """An actor recurrent_N 2 with zero masks, and a critic recurrent_N 1."""
    return masks_case("actor"), shape_case("critic", 65, 10)


# nin = 64, 65 and 128: the bias column alone in a job's second tile, beside one weight column, and alone in
# its third (the accumulators a tile drops and the bias two-sum of the last tile, tied to the bytes)
TWICE_PLAN = ("hidden64 rn1 max in", "hidden65", "in128")


def plan_twice_checks(lib, name, device):
    case = plan_case(name)
    a = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
    b = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
    same_bytes(a, b, case.name)
    c = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device, dx=(False, False))
    np.testing.assert_array_equal(c["dweights"].view(np.int32), a["dweights"].view(np.int32))


@functools.lru_cache(maxsize=None)
def masks_case(kind):
    cfg = dataclasses.replace(ACTOR if kind == "actor" else CRITIC, recurrent_N=2)
    return admitted("masks " + kind, cfg, OPTION_C, OPTION_T, 3, mask_zeros=True)


@functools.lru_cache(maxsize=None)
def avail_case():
    return admitted("available_actions", ACTOR, OPTION_C, OPTION_T, 5, avail="some")


@functools.lru_cache(maxsize=None)
def slab_case(kind, R):
    """R rows of a small recurrent head in chunks of T = 2 (odd R: T = 1)."""
    T = 2 if R % 2 == 0 else 1
    cfg = dataclasses.replace(ACTOR if kind == "actor" else CRITIC, num_actions=5 if kind == "actor" else None, **SMALL)
    return admitted("slab %s R%d" % (kind, R), cfg, R // T, T, 2)


def entries(cfg, dweights):
    """{name: gradient} of a dweights blob; the feature-norm slots, left out without it, must be 0."""
    if not cfg.feature_norm:
        assert (dweights[:2 * (cfg.in0 + cfg.in1)] == 0).all(), "the unused feature-norm slots are not 0"
    return policy.unpack_head_weights(dweights, cfg)


def compare(got, case, what):
    out = dict(entries(case.cfg, got["dweights"]), **{k: got[k] for k in ("dx0", "dx1") if k in got})
    assert sorted(out) == sorted(case.names), (sorted(out), sorted(case.names))
    for k in case.names:
        pm.assert_close(out[k], case.g64[k], *case.tol[k], "%s %s" % (what, k))


def check(lib, case, device=None):
    """Parity of the entry point (host, or the kernels on `device`) with the float64 autograd within the
    measured tolerance, per gradient tensor. Returns the outputs."""
    got = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
    compare(got, case, "backward %s %s" % ("host" if device is None else "device", case.name))
    return got


def same_bytes(a, b, what=""):
    assert set(a) == set(b), what
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg="%s %s" % (what, k))


def avail_checks(lib, device):
    """Some actions unavailable: the model's gradients; 1e30 in dlogits at the unavailable entries gives the
    same bytes as zeros there."""
    case = avail_case()
    av = case.inp["avail"]
    assert (av == 0).sum() > case.R
    check(lib, case, device)
    zeros = np.where(av == 0, np.float32(0), case.dout)
    junk = np.where(av == 0, np.float32(1e30), case.dout)
    a = run(lib, case.cfg, case.blob, case.inp, zeros, case.C, case.T, device)
    b = run(lib, case.cfg, case.blob, case.inp, junk, case.C, case.T, device)
    same_bytes(a, b, "availability")


def twice_and_null_checks(lib, device):
    """The same call twice: identical bytes. Null dx0 / dx1 leave dweights the same bytes."""
    for case in (shape_case("actor", 129, 2), masks_case("critic")):
        a = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
        b = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
        same_bytes(a, b, case.name)
        for dx in ((False, False), (True, False), (False, True)):
            c = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device, dx=dx)
            assert set(c) == {"dweights"} | ({"dx0"} if dx[0] else set()) | ({"dx1"} if dx[1] else set())
            for k in c:
                np.testing.assert_array_equal(c[k].view(np.int32), a[k].view(np.int32), err_msg=k)


def structure_checks(lib, device):
    """Exact zeros, no model. A recurrent_N 2 head, C = 67 (two tiles), T = 4, a zero mask at step 2 of chunk 5."""
    cfg = dataclasses.replace(ACTOR, recurrent_N=2, num_actions=5, **SMALL)
    _, blob = pc.weights(cfg, 1)
    Cn, T = 67, 4
    R = Cn * T
    inp = em.random_inputs(cfg, Cn, T, seed=1)
    mk = np.ones((T, Cn), np.float32)
    mk[2, 5] = 0
    inp["masks"] = mk.reshape(R, 1)
    go = lambda s, i=inp, c=cfg, b=blob: run(lib, c, b, i, s, Cn, T, device)
    dx = lambda g: np.concatenate([g["dx0"], g["dx1"]], axis=1).reshape(T, Cn, -1)

    zero = go(np.zeros((R, 5), np.float32))
    for k, v in zero.items():
        assert (v == 0).all(), "zero seeds: %s is not exactly 0" % k

    def one(l, b):
        s = np.zeros((T, Cn, 5), np.float32)
        s[l, b] = [0.3, -0.2, 0.1, 0.25, -0.45]
        return s.reshape(R, 5)

    # a seed at step 3 of chunk 9 alone: every other chunk, and nothing later (there is nothing later), is 0;
    # all of chunk 9's earlier steps are reached through the state
    d = dx(go(one(3, 9)))
    others = np.arange(Cn) != 9
    assert (d[:, others] == 0).all() and (np.abs(d[:, 9]).max(axis=1) > 0).all()
    # a seed at step 1 of chunk 64 (the second tile's first chunk): later steps of the chunk are exactly 0
    d = dx(go(one(1, 64)))
    assert (d[:, np.arange(Cn) != 64] == 0).all() and (d[2:, 64] == 0).all()
    assert (np.abs(d[:2, 64]).max(axis=1) > 0).all()
    # behind the zero mask at step 2 of chunk 5: a seed at step 3 (or 2) leaves steps 0 and 1 exactly 0
    for l in (3, 2):
        d = dx(go(one(l, 5)))
        assert (d[:2, 5] == 0).all() and (np.abs(d[2:l + 1, 5]).max(axis=1) > 0).all(), l
    # dweights of two disjoint seed sets add up to that of their union within the tolerance: the union case's
    # own per-tensor bound (the gradient is linear in the seed)
    case = slab_case("actor", 2 * SLAB)
    half = np.arange(case.R)[:, None] % 3 == 0
    ga = run(lib, case.cfg, case.blob, case.inp, np.where(half, case.dout, np.float32(0)), case.C, case.T, device)
    gb = run(lib, case.cfg, case.blob, case.inp, np.where(half, np.float32(0), case.dout), case.C, case.T, device)
    gu = run(lib, case.cfg, case.blob, case.inp, case.dout, case.C, case.T, device)
    ea, eb, eu = (entries(case.cfg, g["dweights"]) for g in (ga, gb, gu))
    for k in eu:
        tol = case.tol[k][0]
        err = float(np.abs(ea[k].astype(np.float64) + eb[k] - eu[k]).max())
        print("disjoint seeds %s: err %.3e tol %.3e" % (k, err, tol))
        assert err <= tol, (k, err, tol)

    # recurrent_N 0: dx row m depends on seed row m only
    cfg0 = dataclasses.replace(cfg, recurrent_N=0)
    _, blob0 = pc.weights(cfg0, 1)
    inp0 = em.random_inputs(cfg0, R, 1, seed=1)
    s = np.zeros((R, 5), np.float32)
    s[70] = [0.3, -0.2, 0.1, 0.25, -0.45]
    g = run(lib, cfg0, blob0, inp0, s, R, 1, device)
    d = np.concatenate([g["dx0"], g["dx1"]], axis=1)
    assert (d[np.arange(R) != 70] == 0).all() and np.abs(d[70]).max() > 0


def refusal_checks(lib, device=None):
    """Every refusal starts with "backward: " and writes nothing (run() asserts both)."""
    case = shape_case("actor", 1, 3)
    crit = shape_case("critic", 1, 3)
    bad = lambda c=case, **kw: run(lib, kw.pop("cfg", c.cfg), c.blob, c.inp, c.dout, kw.pop("C", c.C), kw.pop("T", c.T),
                                   device, expect_rc=1, **kw)
    for field in ("x0", "x1", "rnn_states", "masks", "dlogits", "dweights", "workspace"):
        bad(over={field: None})
    bad(crit, over={"dvalues": None})
    bad(over={"weights": None})
    bad(over={"io": None})
    for field in ("x0", "x1", "rnn_states", "masks", "available_actions", "dlogits", "dweights", "dx0", "dx1"):
        if field == "available_actions":
            c = avail_case()
            run(lib, c.cfg, c.blob, c.inp, c.dout, c.C, c.T, device, expect_rc=1, add={field: 2})
        else:
            bad(add={field: 2})
    bad(crit, add={"dvalues": 2})
    bad(add={"weights": 2})
    bad(add={"workspace": 4})
    bad(T=0)
    bad(C=-1)
    bad(C=2 ** 30, T=2)
    for out, other in (("dx0", "x0"), ("dx1", "x1"), ("dx1", "dlogits"), ("dweights", "masks"), ("dx1", "dx0"),
                       ("dx0", "dweights"), ("dweights", "workspace"), ("dx1", "workspace")):
        bad(alias=(out, other, 0))
    bad(alias=("dx1", "x1", 4))
    st = case.cfg.struct()
    big = dataclasses.replace(ACTOR, hidden=128, in0=200, in1=40)
    bad(cfg=big)
    text = lib.lsm_policy_last_error().decode()
    assert "bytes of LDS" in text and "163840" in text, text
    for k, v in (("hidden", 0), ("hidden", 129), ("layer_N", 5), ("recurrent_N", 3), ("kind", 2), ("num_actions", 65),
                 ("in1", -1)):
        c2 = capi.LsmHeadConfig.from_buffer_copy(st)
        setattr(c2, k, v)
        bad(cfg=c2)
        assert lib.lsm_head_backward_workspace_bytes(c2, 1, 1) == 0
    # C == 0 is legal and writes nothing
    run(lib, case.cfg, case.blob, case.inp, case.dout, 0, 3, device)
