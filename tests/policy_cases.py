"""The policy-head tests' cases (shared by tests/test_policy_capi.py on the host entry point and
tests/test_gpu_policy.py on the kernel): a few rows each, with tests/policy_model.py's two models computed
once per case, and the checks both files run.

The kernel's tile is 64 rows, so the row counts are 1, 63, 64, 65 and 257 (five workgroups, the last with
one row)."""
import dataclasses
import functools

import numpy as np

import policy_abi as pa
import policy_model as pm
from lsm.policy import HeadConfig, pack_head_weights

OBS = 6                                            # the env's obs width; 48 = 8 agents' obs, the shared row
ACTOR = HeadConfig(kind="actor", in0=OBS, in1=16, num_actions=25)    # the reference's defaults otherwise
CRITIC = HeadConfig(kind="critic", in0=48, in1=16)
SHAPE_M = (1, 63, 64, 65, 257)
MAX_UNDECIDABLE = 0.05


@functools.lru_cache(maxsize=None)
def weights(cfg, seed=0):
    """The case's state dict and its packed blob (HeadConfig is hashable)."""
    sd = pm.random_head_weights(cfg, seed)
    return sd, pack_head_weights(sd, cfg)


class Case:
    def __init__(self, name, cfg, M, seed=0, mask_zeros=False, avail=None, inp=None):
        self.name, self.cfg, self.M, self.seed = name, cfg, M, seed
        self.sd, self.blob = weights(cfg, seed)
        self.inp = inp if inp is not None else pm.random_inputs(cfg, M, seed, mask_zeros, avail)
        self.w64 = pm.model64(cfg, self.sd, self.inp)
        self.w32 = pm.model32(cfg, self.sd, self.inp)
        # the tolerance per output tensor, from the two models alone
        self.tol = {}
        for k in ("features", "rnn_out", "values"):
            if k in self.w64:
                self.tol[k] = pm.tensor_bound(self.w64[k], self.w32[k])
        if cfg.kind == "actor":
            self.fin = pm.finite_logits(self.w64["logits"])
            self.tol["logits"] = pm.tensor_bound(self.w64["logits"], self.w32["logits"], self.fin)
            self.tol["log_probs"] = pm.tensor_bound(self.w64["logp"], self.w32["logp"], self.fin)
            lb = self.tol["logits"][0]
            self.delta = sample_delta(lb)
            self.u, _ = pm.clamp_u(self.inp["u"])
            self.sampled = pm.sample64(self.w64["cdf"], self.u)
            self.mode = pm.mode64(self.w64["logits"])
            self.dec_sample = decidable_sample(self.w64, self.u, lb)
            self.dec_mode = decidable_mode(self.w64, lb)
            for what, dec in (("sample", self.dec_sample), ("mode", self.dec_mode)):
                frac = 1.0 - dec.mean()
                assert frac <= MAX_UNDECIDABLE, "%s: %.1f %% of the rows undecidable (%s); pick another seed" % (
                    name, 100 * frac, what)


@functools.lru_cache(maxsize=None)
def shape_case(kind, M):
    return Case("%s M%d" % (kind, M), ACTOR if kind == "actor" else CRITIC, M, seed=M % 7)


OPTIONS = {
    "hidden48": (ACTOR, dict(hidden=48)),
    "hidden5 A5": (ACTOR, dict(hidden=5, num_actions=5)),
    "critic hidden5": (CRITIC, dict(hidden=5)),
    "critic x0 null": (CRITIC, dict(in0=0)),
    "actor in 48+16": (ACTOR, dict(in0=48)),
    "layer_N 0": (ACTOR, dict(layer_N=0)),
    "layer_N 2": (ACTOR, dict(layer_N=2)),
    "critic layer_N 2 tanh": (CRITIC, dict(layer_N=2, relu=False)),
    "recurrent_N 0": (ACTOR, dict(recurrent_N=0)),
    "critic recurrent_N 0": (CRITIC, dict(recurrent_N=0)),
    "recurrent_N 2": (ACTOR, dict(recurrent_N=2)),
    "critic recurrent_N 2 hidden48": (CRITIC, dict(recurrent_N=2, hidden=48)),
    "tanh": (ACTOR, dict(relu=False)),
    "no feature norm": (ACTOR, dict(feature_norm=False)),
    "critic no feature norm": (CRITIC, dict(feature_norm=False)),
    "A5": (ACTOR, dict(num_actions=5)),
    "A1": (ACTOR, dict(num_actions=1)),
    "A64 in 250": (ACTOR, dict(num_actions=64, in0=234)),
    "hidden128 recurrent_N 2": (ACTOR, dict(hidden=128, recurrent_N=2)),
}
OPTION_M = 65


@functools.lru_cache(maxsize=None)
def option_case(name):
    base, over = OPTIONS[name]
    return Case("option " + name, dataclasses.replace(base, **over), OPTION_M, seed=1 + sorted(OPTIONS).index(name))


# The forward's own limits (lsm_head_plan, include/lsm_policy.h): its tile has no state rows, so the ABI's
# limits (in 256, hidden 128) are its LDS limit too -- the largest tile the kernel's LDS is raised to -- and
# in0 + in1 = 1 is the narrowest input row. tests/test_launch_plans.py walks the library to both.
PLAN_OPTIONS = {
    "hidden128 recurrent_N 2 in256": (ACTOR, dict(hidden=128, recurrent_N=2, in0=240)),
    "critic hidden128 in256": (CRITIC, dict(hidden=128, in0=240)),
    "in1": (ACTOR, dict(in0=0, in1=1, feature_norm=False)),
    "in1 x1 null": (ACTOR, dict(in0=1, in1=0, feature_norm=False)),
}


@functools.lru_cache(maxsize=None)
def plan_case(name):
    base, over = PLAN_OPTIONS[name]
    return Case("plan " + name, dataclasses.replace(base, **over), OPTION_M, seed=40 + sorted(PLAN_OPTIONS).index(name))


@functools.lru_cache(maxsize=None)
def masks_case(kind):
    """Some rows' masks zero, with large finite garbage in their states."""
    cfg = dataclasses.replace(ACTOR if kind == "actor" else CRITIC, recurrent_N=2)
    return Case("masks " + kind, cfg, OPTION_M, seed=3, mask_zeros=True)


@functools.lru_cache(maxsize=None)
def avail_case():
    return Case("available_actions", ACTOR, OPTION_M, seed=5, avail="some")


def sample_delta(lb):
    """How far u must be from a CDF boundary for the row to be decidable: ten times the logit bound + 1e-6."""
    return 10.0 * lb + 1e-6


def decidable_sample(w64, u, lb):
    """A sampled row is decidable when u is farther than delta from every float64 CDF boundary below 1."""
    cdf = w64["cdf"]
    inner = np.where(cdf < 1.0 - 1e-12, cdf, np.inf)
    return np.abs(inner - np.asarray(u, dtype=np.float64)[:, None]).min(axis=1) > sample_delta(lb)


def decidable_mode(w64, lb):
    """A mode row is decidable when the float64 top-two logit gap exceeds twice the logit bound."""
    return w64["gap"] > 2.0 * lb


def assert_actions(w64, act, lb, u, what):
    """The issue's rule for the discrete output of rows with float64 model w64 and logit bound lb: decidable
    rows match the model's action exactly (u None: the mode; else the sample for the clamped uniforms u);
    every other row returns one of the actions adjacent to the boundary, or one of the tied top actions.
    Returns the number of undecidable rows."""
    M = len(act)
    rows = np.arange(M)
    if u is None:
        dec, want = decidable_mode(w64, lb), pm.mode64(w64["logits"])
        tied = w64["logits"][rows, act] >= w64["logits"].max(axis=1) - 2.0 * lb
        assert tied[~dec].all(), what
    else:
        u64 = np.asarray(u, dtype=np.float64)
        dec, want = decidable_sample(w64, u, lb), pm.sample64(w64["cdf"], u)
        delta = sample_delta(lb)
        lo = pm.sample64(w64["cdf"], np.maximum(u64 - delta, 0.0))
        hi = pm.sample64(w64["cdf"], np.minimum(u64 + delta, 1.0 - 1e-16))
        assert ((act >= lo) & (act <= hi))[~dec].all(), what
        assert (np.exp(w64["logp"][rows, act])[~dec] > 0).all(), what
    print("head %s: %d of %d rows undecidable" % (what, int((~dec).sum()), M))
    np.testing.assert_array_equal(act[dec], want[dec], err_msg=what)
    return int((~dec).sum())


def check_discrete(case, got, mode, what):
    """The discrete outputs of one run: assert_actions' rule; the two action outputs agree; log_probs is the
    float64 log-probability of the action actually returned."""
    cfg, w64 = case.cfg, case.w64
    act = got["actions_i32"]
    assert act.dtype == np.int32 and ((act >= 0) & (act < cfg.num_actions)).all(), what
    np.testing.assert_array_equal(got["actions_f32"], act.astype(np.float32), err_msg=what)
    dec = case.dec_mode if mode else case.dec_sample
    assert assert_actions(w64, act, case.tol["logits"][0], None if mode else case.u, what) == int((~dec).sum())
    if case.inp.get("avail") is not None:
        some = case.inp["avail"].any(axis=1)
        assert (case.inp["avail"][np.arange(case.M), act][dec & some] != 0).all(), what + ": a masked action"
    tol, e32 = case.tol["log_probs"]
    pm.assert_close(got["log_probs"], w64["logp"][np.arange(case.M), act], tol, e32, what + " log_probs")


def check(lib, case, device=None):
    """Parity of the entry point (host, or the kernel on `device`) with model64 within the measured
    tolerance, per output tensor; for an actor with u (sample) and with u = NULL (mode). Returns the runs."""
    where = "host" if device is None else "device"
    runs = {}
    for mode in ((False, True) if case.cfg.kind == "actor" else (False,)):
        got, bad = pa.run(lib, case.cfg, case.blob, case.inp, device, mode=mode)
        what = "%s %s%s" % (where, case.name, " mode" if mode else "")
        assert bad == 0, what
        for k in ("features", "rnn_out", "values"):
            if k in case.w64:
                pm.assert_close(got[k], case.w64[k], *case.tol[k], "%s %s" % (what, k))
        if case.cfg.kind == "actor":
            pm.assert_close(got["logits"], case.w64["logits"], *case.tol["logits"], what + " logits", sel=case.fin)
            assert (got["logits"][~case.fin] == np.float32(pm.FLT_MIN)).all(), what
            check_discrete(case, got, mode, what)
        runs[mode] = got
    return runs


def _where(device):
    return "host" if device is None else "device"


def masks_checks(lib, kind, device):
    """Rows whose mask is 0 carry 1e30 / -7.5e20 in their states: the outputs are the model's (whose h is 0
    there), and equal, to the byte, those of the same call with zeros in place of the garbage."""
    case = masks_case(kind)
    zero = case.inp["masks"].reshape(-1) == 0
    assert zero.any() and (~zero).any() and (np.abs(case.inp["states"][zero]) > 1e20).all()
    got = check(lib, case, device)[False]
    clean = dict(case.inp, states=np.where(zero[:, None, None], np.float32(0), case.inp["states"]))
    again, _ = pa.run(lib, case.cfg, case.blob, clean, device)
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), again[k].view(np.int32), err_msg=k)
    # and the state does count where the mask is 1
    other = dict(case.inp, states=case.inp["states"] + np.float32(0.25))
    moved, _ = pa.run(lib, case.cfg, case.blob, other, device)
    d = np.abs(moved["features"] - got["features"]).max(axis=1)
    assert (d[~zero] > 1e-3).all()


def avail_checks(lib, device):
    """Some actions masked (never returned on a decidable row: check_discrete), row 1 with a single
    available action (that action, log-probability 0 within the tolerance), row 2 with none (uniform)."""
    case = avail_case()
    av = case.inp["avail"]
    A = case.cfg.num_actions
    assert av[1].sum() == 1 and av[2].sum() == 0 and (av[3:].sum(axis=1) >= 1).all() and (av == 0).sum() > case.M
    np.testing.assert_allclose(case.w64["logp"][2], -np.log(A), rtol=0, atol=1e-12)
    runs = check(lib, case, device)
    tol = case.tol["log_probs"][0]
    for mode, got in runs.items():
        assert got["actions_i32"][1] == A // 2 and abs(float(got["log_probs"][1])) <= tol
        assert abs(float(got["log_probs"][2]) + np.log(A)) <= tol
        assert (got["logits"][2] == np.float32(pm.FLT_MIN)).all()
    assert runs[True]["actions_i32"][2] == 0                                  # the first of the tied maxima
    assert runs[False]["actions_i32"][2] == int(case.u[2] * np.float32(A))    # uniform: floor(u * A), exact in f32


STRAT_M = 4096


@functools.lru_cache(maxsize=None)
def stratified_case():
    """One input row repeated 4096 times, u_i = (i + 0.5) / 4096; A = 5 and the first seed for which every
    row is decidable by the model alone (no u_i within delta of a CDF boundary), so the counts are the
    model's own."""
    cfg = dataclasses.replace(ACTOR, num_actions=5)
    for seed in range(200):
        one = pm.random_inputs(cfg, 1, seed)
        inp = {k: (np.repeat(v, STRAT_M, axis=0) if v is not None else None) for k, v in one.items()}
        inp["u"] = ((np.arange(STRAT_M) + 0.5) / STRAT_M).astype(np.float32)
        sd, _ = weights(cfg, 0)
        cdf = pm.model64(cfg, sd, one)["cdf"][0]
        if np.abs(cdf[:-1, None] - inp["u"][None, :].astype(np.float64)).min() > 2e-5 and np.diff(cdf, prepend=0).min() > 0.02:
            case = Case("stratified", cfg, STRAT_M, seed=0, inp=inp)
            if case.dec_sample.all():
                return case
    raise AssertionError("no seed gives a stratified case the model decides alone")


def stratified_checks(lib, device):
    case = stratified_case()
    got, bad = pa.run(lib, case.cfg, case.blob, case.inp, device, outputs=("actions_i32",))
    assert bad == 0
    p = np.exp(case.w64["logp"][0])
    counts = np.bincount(got["actions_i32"], minlength=5)
    print("head %s stratified: counts %s, 4096 p %s" % (_where(device), counts.tolist(), np.round(STRAT_M * p, 2).tolist()))
    assert counts.sum() == STRAT_M and (np.abs(counts - STRAT_M * p) <= 1.0).all()
    assert (np.diff(got["actions_i32"]) >= 0).all()     # the inverse CDF is monotone in u
    np.testing.assert_array_equal(got["actions_i32"], case.sampled)


def twice_and_null_checks(lib, device):
    """The same call twice: identical bytes on every output. Null optional outputs are left unwritten
    (their canaried buffers are not even passed) and do not change the others."""
    for case in (shape_case("actor", 257), masks_case("critic")):
        a, _ = pa.run(lib, case.cfg, case.blob, case.inp, device)
        b, _ = pa.run(lib, case.cfg, case.blob, case.inp, device)
        for k in a:
            np.testing.assert_array_equal(a[k].view(np.int32), b[k].view(np.int32), err_msg=k)
        for only in (("actions_f32",), ("actions_i32", "log_probs")) if case.cfg.kind == "actor" else (("values",), ("rnn_out",), ()):
            c, _ = pa.run(lib, case.cfg, case.blob, case.inp, device, outputs=only)
            assert set(c) == set(only)
            for k in c:
                np.testing.assert_array_equal(c[k].view(np.int32), a[k].view(np.int32), err_msg=k)


def bad_u_checks(lib, device):
    """NaN, 1.0 and -0.1 (and inf): *bad is set, the action is the clamped uniform's, every other row is
    unchanged; *bad is never cleared by a call."""
    case = shape_case("actor", 65)
    clean, bad = pa.run(lib, case.cfg, case.blob, case.inp, device)
    assert bad == 0
    rows = {3: np.nan, 17: 1.0, 40: -0.1, 64: np.inf}
    u = case.inp["u"].copy()
    for r, v in rows.items():
        u[r] = v
    got, bad = pa.run(lib, case.cfg, case.blob, dict(case.inp, u=u), device)
    assert bad == 1
    uc, flagged = pm.clamp_u(u)
    assert sorted(np.nonzero(flagged)[0].tolist()) == sorted(rows)
    want = pm.sample64(case.w64["cdf"], uc)
    A = case.cfg.num_actions
    for r in rows:
        assert 0 <= got["actions_i32"][r] < A and got["actions_i32"][r] == want[r], r
    last = case.w64["cdf"].shape[1] - 1
    assert want[3] == want[40] == 0 and want[17] == want[64] == last     # u = 0: the first action; u -> 1: the last
    keep = np.array([r for r in range(case.M) if r not in rows])
    for k in clean:
        np.testing.assert_array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32), err_msg=k)
    for r in rows:     # the row's network outputs do not depend on u
        np.testing.assert_array_equal(got["features"][r].view(np.int32), clean["features"][r].view(np.int32))
    got, bad = pa.run(lib, case.cfg, case.blob, case.inp, device, bad_init=5)
    assert bad == 5
    # the mode ignores u altogether
    got, bad = pa.run(lib, case.cfg, case.blob, dict(case.inp, u=u), device, mode=True)
    assert bad == 0
