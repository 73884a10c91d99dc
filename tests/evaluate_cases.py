"""The evaluate tests' cases and checks (shared by tests/test_evaluate_capi.py on the host entry point and
tests/test_gpu_evaluate.py on the kernel), with tests/evaluate_model.py's two models computed once per case,
and the ctypes call: inputs on the host or on a torch device (tests/recurrent_abi.py's Placed), every
requested output between canaries.

The kernel's tile is 64 chunks and a minibatch is time-major, so (C, T) takes (1, 1), (1, 3), (63, 2),
(64, 3), (65, 10) and (129, 2); the options run at C = 65, T = 3.

Tolerance: the project's rule per case and output tensor, 4 * e32 + 4 * 2^-23 * s from the two models
alone (policy_model.tensor_bound). dist_entropy: the case's entropy tolerance (a weighted mean of errors
is at most their maximum) plus 2^-23 * |value|. The log-probability of a stored action that is unavailable
must only be <= -1e37.

Which seeds make a case. The rule takes e32, one float32 evaluation's error, as the measure of every float32
evaluation's error. That holds while no single row dominates by its conditioning. A LayerNorm scales an
error of its input by 1 / sqrt(var + eps), and at hidden 5 a ReLU row such as [0, 0, 0, 0, 3e-2] has a gain of
30 or more, and several LayerNorms in a row multiply. Where the gains above 1 of a row multiply to 1000, one
rounding of 2^-23 at the row's input shows as 1.2e-4 at its output, some forty times e32 of these cases (1e-6
to 1e-5): whichever of two correct float32 evaluations happens to round that input well wins by an order of
magnitude, and e32, one sample, says nothing about the other. (Measured on the host entry point before the
rule existed: over 30 seeds of the two hidden-5 options err / e32 was 0.2 to 2.9, and 5.3 -- 1.2 times the
tolerance -- for one seed whose worst row has a product of 1813.) So a case admits only inputs in which the
float64 model (alone) finds no row with a product above MAX_AMP = 1000 (rows at hidden 48 and more: 5 to 20;
at hidden 5: a median of 10, a tail of a few hundred); a generated case takes the first seed from its own on
that qualifies, a case with given inputs asserts it."""
import ctypes as C
import dataclasses
import functools

import numpy as np

import evaluate_model as em
import launch_plans as lp
import policy_abi as pa
import policy_cases as pc
import policy_model as pm
import recurrent_abi as ra
from lsm import capi

ACTOR, CRITIC = pc.ACTOR, pc.CRITIC
SHAPES = ((1, 1), (1, 3), (63, 2), (64, 3), (65, 10), (129, 2))
OPTION_C, OPTION_T = 65, 3
ACTOR_OUT = ("log_probs", "entropy", "dist_entropy", "logits", "features", "rnn_out")
CRITIC_OUT = ("values", "features", "rnn_out")
INPUTS = {"x0": "x0", "x1": "x1", "states": "rnn_states", "masks": "masks", "actions": "actions",
          "avail": "available_actions", "active": "active_masks"}
EPS = 2.0 ** -23
MAX_AMP = 1000.0


def out_shapes(cfg, Cn, T):
    R = Cn * T
    return {"log_probs": (R,), "entropy": (R,), "dist_entropy": (1,), "logits": (R, cfg.num_actions or 1),
            "values": (R,), "features": (R, cfg.hidden), "rnn_out": (Cn, cfg.recurrent_N, cfg.hidden)}


def default_outputs(cfg):
    names = ACTOR_OUT if cfg.kind == "actor" else CRITIC_OUT
    return tuple(n for n in names if n != "rnn_out" or cfg.recurrent_N)


def run(lib, cfg, blob, inp, Cn, T, device=None, outputs=None, bad_init=0, expect_rc=0, over=None, add=None,
        alias=None, scratch=True):
    """lsm_host_head_evaluate (device None) or lsm_head_evaluate on `device`. outputs: the names to request
    (the others are passed as NULL). Returns ({name: array}, bad). over: replace io fields (by their header
    name), or 'cfg' / 'weights' / 'C' / 'T' / 'io'; add: {field or 'weights': bytes added to that pointer};
    alias: (field, other field, bytes). With expect_rc != 0 the outputs must hold their canaries, the text
    must start with "evaluate: " and bad must be untouched."""
    outputs = default_outputs(cfg) if outputs is None else tuple(outputs)
    keep = [ra.Placed(np.ascontiguousarray(blob, dtype=np.float32), 0, device)]
    io = capi.LsmEvalIo()
    for key, field in INPUTS.items():
        a = inp.get(key)
        if a is None or np.asarray(a).size == 0:
            continue
        p = ra.Placed(np.ascontiguousarray(a, dtype=np.float32), 0, device)
        keep.append(p)
        setattr(io, field, p.ptr)
    shapes = out_shapes(cfg, Cn, T)
    dsts = {}
    for name in outputs:
        d = ra.destination(max(int(np.prod(shapes[name])), 1), 0, device)
        dsts[name] = d
        setattr(io, name, d[0].ptr + 4 * ra.PRE)
    sc = None
    if scratch:
        words = max(int(lib.lsm_head_evaluate_scratch_bytes(max(Cn, 0), max(T, 1))), 16) // 4
        sc = ra.destination(words, 0, device)
        io.scratch = sc[0].ptr + 4 * ra.PRE
    bad = ra.Placed(np.array([bad_init], np.int64), 0, device)
    io.bad = bad.ptr
    args = dict(cfg=cfg.struct() if hasattr(cfg, "struct") else cfg, weights=C.c_void_p(keep[0].ptr), io=C.byref(io),
                C=Cn, T=T)
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
        rc = lib.lsm_host_head_evaluate(args["cfg"], args["weights"], args["io"], args["C"], args["T"])
    else:
        import torch
        rc = lib.lsm_head_evaluate(args["cfg"], args["weights"], args["io"], args["C"], args["T"],
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
    err = lib.lsm_policy_last_error().decode()
    assert (rc != 0) == (expect_rc != 0), (rc, err)
    badv = int(bad.read().view(np.int64)[0])
    if sc is not None:
        w = ra.read_destination(sc, "evaluate scratch")     # the canaries around the scratch
        if expect_rc:
            assert (w == ra.CANARY).all(), "a refused call wrote scratch"
    got = {}
    for name, d in dsts.items():
        words = ra.read_destination(d, "evaluate " + name)
        n = int(np.prod(shapes[name]))
        if expect_rc or n == 0 or Cn == 0:
            assert (words == ra.CANARY).all(), "a refused or empty call wrote %s" % name
            continue
        got[name] = words[:n].view(np.float32).reshape(shapes[name]).copy()
    if expect_rc:
        assert err.startswith("evaluate: ") and len(err) > len("evaluate: "), err
        assert badv == bad_init, "a refused call wrote bad"
    return got, badv


class Case:
    def __init__(self, name, cfg, Cn, T, seed=0, mask_zeros=False, avail=None, active=None, inp=None):
        self.name, self.cfg, self.C, self.T, self.R = name, cfg, Cn, T, Cn * T
        self.sd, self.blob = pc.weights(cfg, seed)
        self.inp = inp if inp is not None else em.random_inputs(cfg, Cn, T, seed, mask_zeros, avail, active)
        self.w64 = em.model64(cfg, self.sd, self.inp, Cn, T)
        assert self.w64["amp"].max() <= MAX_AMP, "%s: a row's LayerNorm gains multiply to %.0f; pick another seed" % (
            name, self.w64["amp"].max())
        self.w32 = em.model32(cfg, self.sd, self.inp, Cn, T)
        # the tolerance per output tensor, from the two models alone
        self.tol = {}
        for k in ("features", "rnn_out", "values"):
            if k in self.w64:
                self.tol[k] = pm.tensor_bound(self.w64[k], self.w32[k])
        if cfg.kind == "actor":
            self.fin = pm.finite_logits(self.w64["logits"])
            self.some = self.fin.any(axis=1)                  # rows with at least one available action
            a, _ = em.clamp_actions(self.inp["actions"], cfg.num_actions)
            # rows whose stored action is unavailable although others are: only <= -1e37 is asked of them
            self.unavail = self.some & ~self.fin[np.arange(self.R), a]
            self.tol["logits"] = pm.tensor_bound(self.w64["logits"], self.w32["logits"], self.fin)
            self.tol["log_probs"] = pm.tensor_bound(self.w64["log_probs"], self.w32["log_probs"],
                                                    self.some & ~self.unavail)
            self.tol["entropy"] = pm.tensor_bound(self.w64["entropy"], self.w32["entropy"], self.some)


def admitted(name, cfg, Cn, T, seed, **kw):
    """The Case of the first seed from `seed` on whose rows are all within MAX_AMP (see above)."""
    for s in range(seed, seed + 50):
        sd, _ = pc.weights(cfg, s)
        if em.model64(cfg, sd, em.random_inputs(cfg, Cn, T, s, **kw), Cn, T)["amp"].max() <= MAX_AMP:
            return Case(name, cfg, Cn, T, seed=s, **kw)
    raise AssertionError("%s: no admissible seed" % name)


@functools.lru_cache(maxsize=None)
def shape_case(kind, Cn, T):
    return admitted("%s C%d T%d" % (kind, Cn, T), ACTOR if kind == "actor" else CRITIC, Cn, T, (Cn + T) % 7)


OPTIONS = {
    "recurrent_N 0": (ACTOR, dict(recurrent_N=0)),
    "critic recurrent_N 0": (CRITIC, dict(recurrent_N=0)),
    "recurrent_N 2": (ACTOR, dict(recurrent_N=2)),
    "critic recurrent_N 2 hidden48": (CRITIC, dict(recurrent_N=2, hidden=48)),
    "hidden5 A5": (ACTOR, dict(hidden=5, num_actions=5)),
    "critic hidden5": (CRITIC, dict(hidden=5)),
    "hidden48": (ACTOR, dict(hidden=48)),
    "A1": (ACTOR, dict(num_actions=1)),
    "A5": (ACTOR, dict(num_actions=5)),
    "A64": (ACTOR, dict(num_actions=64)),
    "tanh": (ACTOR, dict(relu=False)),
    "critic tanh": (CRITIC, dict(relu=False)),
    "no feature norm": (ACTOR, dict(feature_norm=False)),
    "critic no feature norm": (CRITIC, dict(feature_norm=False)),
    "layer_N 0": (ACTOR, dict(layer_N=0)),
    "layer_N 2": (ACTOR, dict(layer_N=2)),
    "critic layer_N 2": (CRITIC, dict(layer_N=2)),
    "critic x0 null": (CRITIC, dict(in0=0)),
}


@functools.lru_cache(maxsize=None)
def option_case(name):
    base, over = OPTIONS[name]
    return admitted("option " + name, dataclasses.replace(base, **over), OPTION_C, OPTION_T,
                    1 + sorted(OPTIONS).index(name))


# ---- one case per launch plan and size limit (lsm_head_plan, include/lsm_policy.h) ---------------------------
# Run by the evaluate and the backward tests alike (heads_backward_cases.plan_case), at C = 65; T = 3, or 2 for
# the cases at a limit. "max" is resolved per routine by walking the library's own plan call
# (tests/launch_plans.py): the evaluate takes every in <= 256 at hidden 64 and hidden 128 / 124 with
# recurrent_N 1 / 2 (so the forward's `hidden128 recurrent_N 2` is refused here, see
# test_launch_plans.py); the backward's limits are include/lsm_backward.h's 240, 172, 88, 76 and 248.
# tests/test_launch_plans.py asserts that these cases' plans cover every branch of the backward's plan.
PLAN_OPTIONS = {
    "hidden128 rn0 in22": (ACTOR, dict(hidden=128, recurrent_N=0)),
    "hidden128 rn0 max in": (ACTOR, dict(hidden=128, recurrent_N=0, width="max")),
    "hidden64 rn1 max in": (ACTOR, dict(width="max")),
    "critic hidden64 rn2 max in": (CRITIC, dict(recurrent_N=2, width="max")),
    "rn1 max hidden": (CRITIC, dict(in0=6, hidden="max")),
    "rn2 max hidden": (ACTOR, dict(recurrent_N=2, hidden="max")),
    "layer_N 3": (ACTOR, dict(layer_N=3)),
    "critic layer_N 4": (CRITIC, dict(layer_N=4)),
    "hidden63": (ACTOR, dict(hidden=63)),
    "hidden65": (ACTOR, dict(hidden=65)),
    "critic hidden65 rn2": (CRITIC, dict(hidden=65, recurrent_N=2)),
    "in63": (ACTOR, dict(width=63)),
    "in65": (CRITIC, dict(width=65)),
    "in127": (ACTOR, dict(width=127)),
    "in128": (CRITIC, dict(width=128)),
    "in129": (ACTOR, dict(width=129)),
    "A64 hidden48": (ACTOR, dict(num_actions=64, hidden=48)),       # A > max(in, hidden)
    # in0 + in1 = 1: eval_tile parks the dist_entropy partials in the input rows. Without the feature norm;
    # with it LayerNorm(1) returns beta whatever the input (x - mean is 0), which the admission rule takes
    # (no amplification: the gain is 0) but which tests nothing of the input path, so it is one case only.
    "in1": (ACTOR, dict(in0=0, in1=1, feature_norm=False)),
    "in1 x1 null": (ACTOR, dict(in0=1, in1=0, feature_norm=False)),
    "in1 feature norm": (ACTOR, dict(in0=0, in1=1)),
}
# the forward's `hidden128 recurrent_N 2` is refused by the evaluate at every width (168960 bytes at in = 22);
# what it does take of hidden 128 with an RNN is recurrent_N 1 up to in = 240, a tile of the whole LDS, which
# the backward refuses at every width
EVALUATE_ONLY = {"hidden128 rn1 max in": (ACTOR, dict(hidden=128, width="max"))}
PLAN_OPTIONS.update(EVALUATE_ONLY)
BACKWARD_PLAN_NAMES = tuple(n for n in sorted(PLAN_OPTIONS) if n not in EVALUATE_ONLY)
PLAN_LIMITS = tuple(n for n in sorted(PLAN_OPTIONS) if "max" in PLAN_OPTIONS[n][1].values())


def plan_cfg(name, which="evaluate"):
    """The case's config for the routine `which` ('evaluate' or 'backward'): a 'max' is that routine's."""
    base, over = PLAN_OPTIONS[name]
    over = dict(over)
    width, hidden = over.pop("width", None), over.pop("hidden", None)
    cfg = dataclasses.replace(base, **over)
    if hidden == "max":
        cfg = dataclasses.replace(cfg, hidden=lp.largest_hidden(cfg, which))
    elif hidden is not None:
        cfg = dataclasses.replace(cfg, hidden=hidden)
    if width == "max":
        cfg = lp.with_in(cfg, lp.largest_in(cfg, which))
    elif width is not None:
        cfg = lp.with_in(cfg, width)
    return cfg


def plan_T(name):
    return 2 if name in PLAN_LIMITS else OPTION_T


def beyond(name, which="evaluate"):
    """The limit case's config one step past its limit (None where the ABI's own limit, 256 or 128, is it)."""
    cfg = plan_cfg(name, which)
    if PLAN_OPTIONS[name][1].get("hidden") == "max":
        return dataclasses.replace(cfg, hidden=cfg.hidden + 1) if cfg.hidden < 128 else None
    return lp.with_in(cfg, cfg.in0 + cfg.in1 + 1) if cfg.in0 + cfg.in1 < 256 else None


@functools.lru_cache(maxsize=None)
def plan_case(name):
    return admitted("plan " + name, plan_cfg(name), OPTION_C, plan_T(name), 30 + sorted(PLAN_OPTIONS).index(name))


def plan_checks(lib, name, device):
    """The case against the model; a case at an LDS limit also shows the next size refused, nothing written."""
    case = plan_case(name)
    check(lib, case, device)
    past = beyond(name) if name in PLAN_LIMITS else None
    if past is not None:
        small = em.random_inputs(past, 1, 1, 0)
        run(lib, past, np.zeros(400000, np.float32), small, 1, 1, device, expect_rc=1)
        assert "bytes of LDS" in lib.lsm_policy_last_error().decode()


@functools.lru_cache(maxsize=None)
def masks_case(kind):
    cfg = dataclasses.replace(ACTOR if kind == "actor" else CRITIC, recurrent_N=2)
    return admitted("masks " + kind, cfg, OPTION_C, OPTION_T, 3, mask_zeros=True)


@functools.lru_cache(maxsize=None)
def avail_case(active=None):
    return admitted("available_actions active=%s" % active, ACTOR, OPTION_C, OPTION_T, 5, avail="some", active=active)


@functools.lru_cache(maxsize=None)
def nan_case():
    cfg = dataclasses.replace(ACTOR, recurrent_N=0)
    inp = em.random_inputs(cfg, OPTION_C, OPTION_T, seed=8)
    inp["x1"][70, 3] = np.nan
    return Case("nan", cfg, OPTION_C, OPTION_T, seed=8, inp=inp)


def check(lib, case, device=None):
    """Parity of the entry point (host, or the kernel on `device`) with model64 within the measured
    tolerance, per output tensor. Returns the outputs."""
    where = "host" if device is None else "device"
    got, bad = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device)
    what = "evaluate %s %s" % (where, case.name)
    assert bad == 0, what
    w64 = case.w64
    for k in ("features", "rnn_out", "values"):
        if k in w64:
            pm.assert_close(got[k], w64[k], *case.tol[k], "%s %s" % (what, k))
    if case.cfg.kind == "actor":
        pm.assert_close(got["logits"], w64["logits"], *case.tol["logits"], what + " logits", sel=case.fin)
        assert (got["logits"][~case.fin] == np.float32(pm.FLT_MIN)).all(), what
        pm.assert_close(got["log_probs"], w64["log_probs"], *case.tol["log_probs"], what + " log_probs",
                        sel=~case.unavail)
        assert (got["log_probs"][case.unavail] <= -1e37).all(), what
        pm.assert_close(got["entropy"], w64["entropy"], *case.tol["entropy"], what + " entropy")
        want = w64["dist_entropy"]
        de = float(got["dist_entropy"][0])
        if np.isnan(want):
            assert np.isnan(de), what
        else:
            tol = case.tol["entropy"][0] + EPS * abs(want)
            print("%s dist_entropy: err %.3e tol %.3e" % (what, abs(de - want), tol))
            assert abs(de - want) <= tol, (what, de, want, tol)
    return got


def same_bytes(a, b, what=""):
    assert set(a) == set(b), what
    for k in a:
        np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg="%s %s" % (what, k))


def masks_checks(lib, kind, device):
    """A third of the masks zero, at l = 0 (1e30 / -7.5e20 in the initial states under them) and later, in
    chunks whose tile neighbours have 1: the outputs are the model's, and equal, to the byte, those of the
    same call with zeros in place of the garbage; the state does count where the mask is 1."""
    case = masks_case(kind)
    mk = case.inp["masks"].reshape(case.T, case.C)
    z0 = mk[0] == 0
    assert z0.any() and (~z0).any() and (mk[1:] == 0).any() and (np.abs(case.inp["states"][z0]) > 1e20).all()
    assert mk[case.T - 1, 0] == 0 and mk[case.T - 1, 1] == 1
    got = check(lib, case, device)
    clean = dict(case.inp, states=np.where(z0[:, None, None], np.float32(0), case.inp["states"]))
    again, _ = run(lib, case.cfg, case.blob, clean, case.C, case.T, device)
    same_bytes(got, again, "masks")
    other = dict(case.inp, states=case.inp["states"] + np.float32(0.25))
    moved, _ = run(lib, case.cfg, case.blob, other, case.C, case.T, device)
    d = np.abs(moved["features"][:case.C] - got["features"][:case.C]).max(axis=1)
    assert (d[~z0] > 1e-3).all()
    # a zero mask at the last step cuts the chunk's history: its last-step outputs do not depend on the
    # initial state at all
    cut = mk[case.T - 1] == 0
    rows = (case.T - 1) * case.C + np.nonzero(cut)[0]
    np.testing.assert_array_equal(moved["features"][rows].view(np.int32), got["features"][rows].view(np.int32))


def avail_checks(lib, device):
    """Some actions masked; row 1 with a single available action (entropy 0, log-probability 0), row 2 with
    none (-log A, log A), row 3 storing an unavailable action (<= -1e37); with active_masks None, with
    zeros mixed in, and all zero (NaN)."""
    for active in (None, "some", "zero"):
        case = avail_case(active)
        av, A = case.inp["avail"], case.cfg.num_actions
        assert av[1].sum() == 1 and av[2].sum() == 0 and case.unavail[3] and case.unavail.sum() == 1
        assert (case.some == (np.arange(case.R) != 2)).all() and (av == 0).sum() > case.R
        np.testing.assert_allclose(case.w64["log_probs"][2], -np.log(A), rtol=0, atol=1e-12)
        np.testing.assert_allclose(case.w64["entropy"][2], np.log(A), rtol=0, atol=1e-12)
        got = check(lib, case, device)
        tl, te = case.tol["log_probs"][0], case.tol["entropy"][0]
        assert abs(float(got["log_probs"][1])) <= tl and abs(float(got["entropy"][1])) <= te
        assert abs(float(got["log_probs"][2]) + np.log(A)) <= tl and abs(float(got["entropy"][2]) - np.log(A)) <= te
        assert (got["logits"][2] == np.float32(pm.FLT_MIN)).all()
        assert float(got["log_probs"][3]) <= -1e37
        if active == "zero":
            assert np.isnan(got["dist_entropy"][0]) and np.isnan(case.w64["dist_entropy"])
        if active == "some":
            am = case.inp["active"].reshape(-1)
            assert (am == 0).any() and (am == 1).any()
            assert abs(case.w64["dist_entropy"] - em.dist_entropy(case.w64["entropy"], None)) > 1e-4


def nan_checks(lib, device):
    """One x1 entry NaN without an RNN: that row's features are zeroed, its logits equal the output bias, and
    every other row is what the same call without the NaN gives, to the byte."""
    case = nan_case()
    got = check(lib, case, device)
    bias = case.sd["act.action_out.linear.bias"]
    np.testing.assert_array_equal(got["logits"][70], bias)
    assert (got["features"][70] == 0).all()
    inp = dict(case.inp, x1=np.where(np.isnan(case.inp["x1"]), np.float32(0.5), case.inp["x1"]))
    clean, _ = run(lib, case.cfg, case.blob, inp, case.C, case.T, device)
    keep = np.arange(case.R) != 70
    for k in ("features", "logits", "log_probs", "entropy"):
        np.testing.assert_array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32), err_msg=k)


def bad_action_checks(lib, device):
    """2.5, -1, A and NaN in one row each: *bad is set, the log-probability is the clamped action's, every
    other row and output is unchanged; *bad is never cleared by a call."""
    case = shape_case("actor", 65, 10)
    A = case.cfg.num_actions
    clean, bad = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device)
    assert bad == 0
    rows = {3: 2.5, 130: -1.0, 400: float(A), 649: np.nan}
    want = {3: 2, 130: 0, 400: A - 1, 649: 0}
    tol = case.tol["log_probs"][0]
    for r, v in rows.items():
        acts = case.inp["actions"].copy()
        acts[r] = v
        c, flagged = em.clamp_actions(acts, A)
        assert np.nonzero(flagged)[0].tolist() == [r] and c[r] == want[r]
        got, bad = run(lib, case.cfg, case.blob, dict(case.inp, actions=acts), case.C, case.T, device)
        assert bad == 1, (r, v)
        assert abs(float(got["log_probs"][r]) - case.w64["logp"][r, want[r]]) <= tol, (r, v)
        keep = np.arange(case.R) != r
        np.testing.assert_array_equal(got["log_probs"][keep].view(np.int32), clean["log_probs"][keep].view(np.int32))
        for k in ("entropy", "dist_entropy", "logits", "features", "rnn_out"):
            np.testing.assert_array_equal(got[k].view(np.int32), clean[k].view(np.int32), err_msg=k)
    got, bad = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device, bad_init=5)
    assert bad == 5


def twice_and_null_checks(lib, device):
    """The same call twice: identical bytes on every output, dist_entropy included. Null optional outputs
    are left unwritten (their canaried buffers are not even passed) and do not change the others."""
    for case in (shape_case("actor", 129, 2), masks_case("actor"), masks_case("critic")):
        a, _ = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device)
        b, _ = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device)
        same_bytes(a, b, case.name)
        names = default_outputs(case.cfg)
        subsets = [(n,) for n in names] + ([("log_probs", "entropy")] if case.cfg.kind == "actor" else [()])
        for only in subsets:
            c, _ = run(lib, case.cfg, case.blob, case.inp, case.C, case.T, device, outputs=only,
                       scratch="dist_entropy" in only)
            assert set(c) == set(only)
            for k in c:
                np.testing.assert_array_equal(c[k].view(np.int32), a[k].view(np.int32), err_msg=k)


def t1_checks(lib, device):
    """T = 1: features, rnn_out, logits and values agree with lsm_head_forward on the same inputs within the
    bound, and log_probs equals the forward's log-probability of the action it chose (the mode)."""
    for kind in ("actor", "critic"):
        cfg, seed = (ACTOR if kind == "actor" else CRITIC), 4
        _, blob = pc.weights(cfg, seed)
        inp = em.random_inputs(cfg, 65, 1, seed=2, mask_zeros=True)
        # the same inputs as lsm_head_forward takes them (tests/policy_abi.py)
        fwd_inp = {"x0": inp["x0"], "x1": inp["x1"], "states": inp["states"], "masks": inp["masks"], "u": None,
                   "avail": None}
        fwd, _ = pa.run(lib, cfg, blob, fwd_inp, device, mode=True)
        if kind == "actor":
            inp = dict(inp, actions=fwd["actions_f32"].copy())
        case = Case("T1 " + kind, cfg, 65, 1, seed=seed, inp=inp)
        got = check(lib, case, device)
        pairs = [("features", "features"), ("rnn_out", "rnn_out")]
        pairs += [("logits", "logits"), ("log_probs", "log_probs")] if kind == "actor" else [("values", "values")]
        for k, kf in pairs:
            err = float(np.abs(got[k].astype(np.float64) - fwd[kf]).max())
            equal = bool((got[k].view(np.int32) == fwd[kf].view(np.int32)).all())
            print("evaluate T=1 vs forward %s %s: %.3e (tol %.3e) bit-equal %s" % (kind, k, err, case.tol[k][0], equal))
            assert err <= case.tol[k][0], (kind, k, err)
