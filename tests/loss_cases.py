"""The PPO loss tests' cases and checks (shared by tests/test_loss_capi.py on the host entry point and
tests/test_gpu_loss.py on the kernels), with tests/loss_model.py's models computed once per case, and the ctypes
call: inputs on the host or on a torch device (tests/recurrent_abi.py's Placed), every output, the scratch and
vn_state between canaries.

The kernels' group is 256 rows, so M takes 1, 63, 64, 65, 257 and 2 * 256 + 1; A takes 1, 5, 25 and 64. The two
one-workgroup launches add the groups' sums 256 groups at a time: MANY = 257 * 256 + 1 rows (258 groups, two
stages, the second with two groups) at A = 5 takes that path.

Tolerance: the project's rule per case and output tensor, max |out - model64| <= 4 * e32 + 4 * 2^-23 * s, with
e32 the float32 torch lines' distance from the float64 model and s the tensor's largest magnitude in the model.

Branch points. The losses branch on ratio against 1 -+ c, |values - value_preds| against c, |e| against delta,
and on which of the two min / max arguments wins; float32 and float64 may resolve a near-tie differently, and
the gradient jumps there. A generated case therefore redraws, from the float64 model alone, the rows that come
within a relative 1e-3 of a branch point (old_log_probs, values, value_preds and returns of those rows are drawn
again, until none is left), except where both branches have the same gradient: ratio inside [1 - c, 1 + c]
(surr1 == surr2) and |values - value_preds| <= c (the two errors agree up to rounding). No row is ever left out
of a comparison. The exactly representable branch points have named rows of their own (named_case)."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import loss_model as lm
import recurrent_abi as ra
from lsm import capi
from lsm.loss import LossConfig

GROUP = capi.LSM_LOSS_GROUP
MS = (1, 63, 64, 65, 257, 2 * GROUP + 1)
AS = (1, 5, 25, 64)
MANY = 257 * GROUP + 1
EPS = 2.0 ** -23
MARGIN = 1e-3
DEFAULTS = LossConfig(num_actions=25)
FLAGS = ("use_clipped_value_loss", "use_huber_loss", "use_value_active_masks", "use_policy_active_masks",
         "use_valuenorm")
INPUTS = {"logits": "logits", "actions": "actions", "avail": "available_actions", "old": "old_log_probs",
          "adv": "advantages", "active": "active_masks", "values": "values", "vpreds": "value_preds",
          "returns": "returns"}
ACTOR_IN = ("logits", "actions", "avail", "old", "adv")
CRITIC_IN = ("values", "vpreds", "returns")
VN_STATE = np.array([0.1, 0.75, 0.5], np.float32)   # a normaliser that has seen data: mean 0.2, mean_sq 1.5


def near_branch(cfg, w):
    """Rows of the float64 model's values w that lie within MARGIN of a branch point with a jump behind it."""
    c, dl = lm.f32(cfg.clip_param), lm.f32(cfg.huber_delta)
    bad = np.zeros(w["ratio"].shape, bool)
    with np.errstate(all="ignore"):
        for end in (lm.f32(1.0 - c), lm.f32(1.0 + c)):
            bad |= np.abs(w["ratio"] - end) <= MARGIN * end
        bad |= np.abs(np.abs(w["d"]) - c) <= MARGIN * c
        for e in (w["e_o"], w["e_c"]):
            bad |= np.abs(np.abs(e) - dl) <= MARGIN * dl
        out = np.abs(w["d"]) > c
        top = np.maximum(np.abs(w["l_o"]), np.abs(w["l_c"]))
        bad |= out & (top > 0) & (np.abs(w["l_o"] - w["l_c"]) <= MARGIN * top)
    return bad


def draw_rows(rng, inp, logp, rows):
    """old_log_probs, values, value_preds and returns of `rows`, drawn again."""
    k = len(rows)
    inp["old"][rows] = (logp[rows] + 0.25 * rng.normal(size=k)).astype(np.float32)
    inp["values"][rows] = rng.normal(size=k).astype(np.float32)
    inp["vpreds"][rows] = inp["values"][rows] + (0.3 * rng.normal(size=k)).astype(np.float32)
    ret = 0.5 + 2.0 * rng.normal(size=k)
    far = rng.random(k) < 0.15                       # beyond the Huber delta, on either side
    inp["returns"][rows] = np.where(far, np.where(rng.random(k) < 0.5, 40.0, -40.0) + ret, ret).astype(np.float32)


def random_inputs(cfg, M, seed=0, avail=None, active="some"):
    """avail 'some': row 1 with a single available action, row 2 with none, row 3 storing an unavailable
    action (M >= 4). active: 'some' (about a fifth zero), 'ones', 'zero'. Returns (inputs, redraw rounds)."""
    rng = np.random.default_rng(1000 + seed)
    A = cfg.num_actions
    inp = {"logits": (1.5 * rng.normal(size=(M, A))).astype(np.float32),
           "actions": rng.integers(0, A, size=M).astype(np.float32),
           "adv": rng.normal(size=M).astype(np.float32), "avail": None, "vn_state": VN_STATE.copy()}
    for k in ("old", "values", "vpreds", "returns"):
        inp[k] = np.zeros(M, np.float32)
    if avail == "some":
        assert M >= 4 and A >= 3
        av = (rng.random((M, A)) < 0.7).astype(np.float32)
        av[np.arange(M), inp["actions"].astype(int)] = 1.0
        av[1] = 0.0
        av[1, int(inp["actions"][1])] = 1.0
        av[2] = 0.0
        av[3] = 1.0
        av[3, int(inp["actions"][3])] = 0.0
        inp["avail"] = av
    act = np.ones(M, np.float32)
    if active == "some":
        act = (rng.random(M) >= 0.2).astype(np.float32)
        act[0] = 1.0
        if M > 1:
            act[M - 1] = 0.0
    elif active == "zero":
        act[:] = 0.0
    inp["active"] = act
    return settle(cfg, inp, rng)


def settle(cfg, inp, rng):
    """Draw old_log_probs, values, value_preds and returns of every row, then again those of the rows near a
    branch point until none is left. Returns (inputs, redraw rounds)."""
    M = inp["adv"].size
    w = lm.model64(cfg, dict(inp, old=np.zeros(M), values=np.zeros(M), vpreds=np.zeros(M), returns=np.zeros(M)),
                   critic=False)
    logp = np.where(w["logp"] < -1e30, -2.0, w["logp"])   # a stored unavailable action: an ordinary old value
    rows = np.arange(M)
    for rounds in range(100):
        draw_rows(rng, inp, logp, rows)
        rows = np.nonzero(near_branch(cfg, lm.model64(cfg, inp)))[0]
        if rows.size == 0:
            return inp, rounds
    raise AssertionError("the generator did not terminate: rows %s stay near a branch point" % rows[:8])


def redraw(cfg, inp, seed):
    """settle() again, after a change to the logits, the actions or the availability."""
    return settle(cfg, inp, np.random.default_rng(2000 + seed))


def io_shapes(M, A):
    return {"dlogits": M * A, "dvalues": M, "imp_weights": M, "stats": 4, "denorm": 2}


def run(lib, cfg, inp, device=None, actor=True, critic=True, M=None, expect_rc=0, over=None, add=None, alias=None,
        bad_init=0, skip=()):
    """lsm_host_ppo_loss (device None) or lsm_ppo_loss on `device`. actor / critic False: that half's logits /
    values are passed as NULL. skip: optional outputs passed as NULL. over: replace io fields (header names) or
    'cfg' / 'M' / 'io'; add: {field: bytes added to the pointer}; alias: (field, other field, bytes). Returns
    ({name: float32 array}, bad, vn_state after). With expect_rc != 0 every output, the scratch and vn_state
    must be untouched, the text must start with "loss: " and bad must be untouched."""
    A = cfg.num_actions
    if M is None:
        M = int(np.asarray(inp["adv"]).size)
    keep, io = [], capi.LsmLossIo()
    for key, field in INPUTS.items():
        a = inp.get(key)
        if a is None or (key in ACTOR_IN and not actor) or (key in CRITIC_IN and not critic):
            continue
        a = np.ascontiguousarray(a, dtype=np.float32)
        p = ra.Placed(a if a.size else np.zeros(1, np.float32), 0, device)   # M == 0: a pointer all the same
        keep.append(p)
        setattr(io, field, p.ptr)
    dsts = {}
    for name, n in io_shapes(max(M, 0), A).items():
        if name in skip:
            continue
        dsts[name] = ra.destination(max(n, 1), 0, device)
        setattr(io, name, dsts[name][0].ptr + 4 * ra.PRE)
    words = max(int(lib.lsm_ppo_loss_scratch_bytes(max(M, 0))), 8) // 4
    sc = ra.destination(words, 0, device)
    io.scratch = sc[0].ptr + 4 * ra.PRE
    state0 = np.asarray(inp.get("vn_state", VN_STATE), np.float32)
    vn_buf = np.full(ra.PRE + 3 + ra.TAIL, ra.CANARY, np.int32)
    vn_buf[ra.PRE:ra.PRE + 3] = state0.view(np.int32)
    vn = (ra.Placed(vn_buf, 0, device), 3)
    io.vn_state = vn[0].ptr + 4 * ra.PRE
    bad = ra.Placed(np.array([bad_init], np.int64), 0, device)
    io.bad = bad.ptr
    args = dict(cfg=cfg.struct() if hasattr(cfg, "struct") else cfg, io=C.byref(io), M=M)
    for k, v in (over or {}).items():
        if k in args:
            args[k] = v
        else:
            setattr(io, k, v)
    for k, v in (add or {}).items():
        setattr(io, k, getattr(io, k) + v)
    if alias:
        setattr(io, alias[0], getattr(io, alias[1]) + alias[2])
    if device is None:
        rc = lib.lsm_host_ppo_loss(args["cfg"], args["io"], args["M"])
    else:
        import torch
        rc = lib.lsm_ppo_loss(args["cfg"], args["io"], args["M"], C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_loss_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    badv = int(bad.read().view(np.int64)[0])
    scw = ra.read_destination(sc, "loss scratch")
    state = ra.read_destination(vn, "loss vn_state").view(np.float32)
    untouched = expect_rc or M == 0
    if untouched:
        assert (scw == ra.CANARY).all(), "a refused or empty call wrote scratch"
        assert (state.view(np.int32) == state0.view(np.int32)).all(), "a refused or empty call wrote vn_state"
    got = {}
    for name, d in dsts.items():
        w = ra.read_destination(d, "loss " + name)
        n = io_shapes(max(M, 0), A)[name]
        half_off = (name in ("dlogits", "imp_weights") and not actor) or (name in ("dvalues", "denorm") and not critic)
        if untouched or n == 0 or half_off or (name == "denorm" and not cfg.use_valuenorm):
            assert (w == ra.CANARY).all(), "%s was written by a call that must not" % name
            continue
        if name == "stats":   # a skipped half's scalars keep their canaries
            for i in ((0, 2, 3) if not actor else ()) + ((1,) if not critic else ()):
                assert w[i] == ra.CANARY, "stats[%d] was written by a skipped half" % i
        got[name] = w[:n].view(np.float32).copy()
        if name == "stats":
            got[name][[i for i in range(4) if w[i] == ra.CANARY]] = np.nan
    if "dlogits" in got:
        got["dlogits"] = got["dlogits"].reshape(M, A)
    if expect_rc:
        assert err.startswith("loss: ") and len(err) > len("loss: "), err
        assert badv == bad_init, "a refused call wrote bad"
    return got, badv, state.copy()


class Case:
    def __init__(self, name, cfg, inp, actor=True, critic=True):
        self.name, self.cfg, self.inp, self.actor, self.critic = name, cfg, inp, actor, critic
        self.M = int(np.asarray(inp["adv"]).size)
        import torch
        self.w64 = lm.model64(cfg, inp, actor, critic)
        self.w32 = lm.model_torch(cfg, inp, torch.float32, actor, critic)
        self.tol = {k: lm.tensor_bound(self.w64[k], self.w32[k])
                    for k in ("dlogits", "dvalues", "imp_weights", "stats", "vn_state", "denorm") if k in self.w32}


@functools.lru_cache(maxsize=None)
def shape_case(M, A, avail=None, active="some", **flags):
    cfg = dataclasses.replace(DEFAULTS, num_actions=A, **flags)
    inp, _ = random_inputs(cfg, M, seed=M + 7 * A, avail=avail, active=active)
    return Case("M%d A%d %s %s %s" % (M, A, avail, active, flags), cfg, inp)


def named_inputs():
    """Rows at the exactly representable branch points, c = 0.25, delta = 10, no normaliser: values -
    value_preds = +-c; e = +-delta; e < -delta (loss and gradient 0); adv = 0; logp = old (filled by the caller
    where it must be exact); plus two ordinary rows. A = 3."""
    cfg = dataclasses.replace(DEFAULTS, num_actions=3, clip_param=0.25, use_valuenorm=False)
    rows = {  # name: (values, value_preds, returns, adv)
        "d = +c": (1.0, 0.75, 2.0, 0.5), "d = -c": (1.0, 1.25, 0.5, -0.5),
        "e = +delta": (1.0, 1.0, 11.0, 1.0), "e = -delta": (1.0, 1.0, -9.0, 1.0),
        "e < -delta": (1.0, 1.0, -20.0, -1.0), "e > delta": (1.0, 1.5, 30.0, 2.0),
        "adv = 0": (0.5, 0.25, 1.0, 0.0), "logp = old": (0.5, 2.0, 1.0, 1.5),
        "plain": (0.25, 0.5, -0.75, -1.25), "clipped wins outside": (1.0, 3.0, 0.5, 0.75),
    }
    names = list(rows)
    M = len(names)
    v, vp, ret, adv = (np.array([rows[n][i] for n in names], np.float64) for i in range(4))
    rng = np.random.default_rng(77)
    inp = {"logits": rng.normal(size=(M, 3)), "actions": (np.arange(M) % 3).astype(np.float64), "avail": None,
           "adv": adv, "active": np.where(np.arange(M) == 8, 0.0, 1.0), "values": v, "vpreds": vp, "returns": ret,
           "vn_state": VN_STATE.copy()}
    logp = lm.model64(cfg, dict(inp, old=np.zeros(M)), critic=False)["logp"]
    inp["old"] = logp + np.where(np.arange(M) == names.index("logp = old"), 0.0, 0.3 * np.cos(np.arange(M)))
    return cfg, inp, names


def check(lib, case, device=None):
    """Parity of the entry point (host, or the kernels on `device`) with model64 within the measured
    tolerance, per output tensor; the same call twice is bit-equal. Returns the outputs."""
    where = "host" if device is None else "device"
    got, bad, state = run(lib, case.cfg, case.inp, device, case.actor, case.critic)
    again, _, state2 = run(lib, case.cfg, case.inp, device, case.actor, case.critic)
    assert bad == int(case.w64.get("bad", np.zeros(1, bool)).any())
    assert set(got) == set(again)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), again[k].view(np.int32), err_msg="twice: " + k)
    np.testing.assert_array_equal(state.view(np.int32), state2.view(np.int32))
    if case.critic and case.cfg.use_valuenorm:
        got = dict(got, vn_state=state)
    else:
        np.testing.assert_array_equal(state.view(np.int32), case.inp["vn_state"].view(np.int32))
    for k, (tol, e32) in case.tol.items():
        assert_close(got[k], case.w64[k], tol, e32, "loss %s %s %s" % (where, case.name, k))
    if case.actor and case.inp.get("avail") is not None:
        assert (got["dlogits"][case.inp["avail"] == 0] == 0).all(), "dlogits on an unavailable action"
    return got


RATIOS = []   # (what, max |out - model64| / e32, the same / tolerance) of every comparison made in this session


def assert_close(out, w64, tol, e32, what):
    """max |out - model64| <= tol; NaN exactly where the model has it; prints the figures first."""
    out = np.asarray(out, dtype=np.float64).reshape(-1)
    w64 = np.asarray(w64, dtype=np.float64).reshape(-1)
    nan = np.isnan(w64)
    err = float(np.abs(out - w64)[~nan].max()) if (~nan).any() else 0.0
    r32 = err / e32 if e32 > 0 else float("inf") if err > 0 else 0.0
    rtol = err / tol if tol > 0 else float("inf") if err > 0 else 0.0
    RATIOS.append((what, r32, rtol))
    print("%s: err %.3e  e32 %.3e  tol %.3e  err/e32 %.2f  err/tol %.2f" % (what, err, e32, tol, r32, rtol))
    assert (np.isnan(out) == nan).all(), what
    assert err <= tol, (what, err, tol, e32)
