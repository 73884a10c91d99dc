"""CPU tests of the PPO loss (include/lsm_loss.h): the header and its exports, the float64 model pinned against
the same lines as torch ops with autograd in double and against fixtures recorded from the reference's own
GR_MAPPO.ppo_update in float64 (tests/golden/loss/), lsm_host_ppo_loss -- the per-row text the kernels run --
against tests/loss_model.py within the tolerance measured per case and output tensor (4 * e32 + 4 * 2^-23 * s),
the normaliser's state bit for bit, the chain rule through torch modules, and the argument refusals (which
return before any launch or write, so they need no device)."""
import dataclasses
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import evaluate_model as em
import loss_cases as lc
import loss_model as lm
import policy_model as pm
from lsm import capi, policy
from lsm.loss import LossConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_loss.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "loss")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


# ---- the ABI ----------------------------------------------------------------------------------------------------

def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    from lsm import build
    hdr = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_LOSS) and len(declared) == 4
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE):
        assert not declared & set(other)
    assert "lsm_loss.hip" in build.UNITS and "lsm_head_tile.h" in build.UNITS["lsm_loss.hip"]
    body = hdr[hdr.index("typedef struct lsm_loss_io"):hdr.index("} lsm_loss_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmLossIo._fields_]
    body = hdr[hdr.index("typedef struct lsm_loss_config"):hdr.index("} lsm_loss_config")]
    fields = [n for decl in re.findall(r"(?:double|float|int32_t)\s+([^;]+);", body) for n in re.split(r",\s*", decl)]
    assert fields == [f for f, _ in capi.LsmLossConfig._fields_]
    assert int(re.search(r"#define LSM_LOSS_GROUP (\d+)", hdr).group(1)) == capi.LSM_LOSS_GROUP


def test_the_loss_reuses_the_heads_softmax_and_stays_out_of_the_build_id(lib):
    """masked_softmax and clamp_action live in csrc/lsm_head_tile.h alone (the log-probability is the text
    lsm_head_evaluate runs); the rollout's build id does not cover the loss's files."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_loss.hip", "lsm_loss.h", "lsm_head_tile.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    shared = open(os.path.join(build.CSRC, "lsm_head_tile.h")).read()
    for unit in ("lsm_evaluate.hip", "lsm_loss.hip"):
        src = open(os.path.join(build.CSRC, unit)).read()
        assert '#include "lsm_head_tile.h"' in src and "lsm_rollout.h" not in src
        for piece in ("void masked_softmax(", "int clamp_action("):
            assert piece in shared and piece not in src, (unit, piece)
    src = open(os.path.join(build.CSRC, "lsm_loss.hip")).read()
    assert "atomicAdd" not in src and "__threadfence" not in src


def test_scratch_bytes(lib):
    f = lib.lsm_ppo_loss_scratch_bytes
    G = capi.LSM_LOSS_GROUP
    assert f(-1) == 0
    assert f(0) == f(1) == f(G) == 128 and f(G + 1) == 192 and f(2 * G + 1) == 256


def test_loss_config_from_args():
    import argparse
    args = argparse.Namespace(clip_param=0.1, huber_delta=5.0, value_loss_coef=0.5, entropy_coef=0.02,
                              use_clipped_value_loss=False, use_huber_loss=True, use_value_active_masks=False,
                              use_policy_active_masks=True, use_valuenorm=True, use_popart=False)
    cfg = LossConfig.from_args(args, 7)
    assert cfg == LossConfig(num_actions=7, clip_param=0.1, huber_delta=5.0, value_loss_coef=0.5, entropy_coef=0.02,
                             use_clipped_value_loss=False, use_value_active_masks=False)
    st = cfg.struct()
    assert st.num_actions == 7 and st.vn_beta == 0.99999 and st.use_clipped_value_loss == 0
    from lsm.loss import LossError
    args.use_popart = True
    with pytest.raises(LossError, match="popart"):
        LossConfig.from_args(args, 7)


# ---- the yardstick itself -----------------------------------------------------------------------------------

PIN = {"defaults": {}, "avail": dict(avail="some"), "ones": dict(active="ones"),
       "all off": {f: False for f in lc.FLAGS}, "A1": dict(A=1), "A64": dict(A=64)}


@pytest.mark.parametrize("name", sorted(PIN))
def test_model64_agrees_with_torch_autograd_in_double(name):
    """model64's closed-form gradients against the same lines as torch ops with autograd in double: about
    1e-14 relative on every tensor, so the yardstick does not depend on the code under test."""
    import torch
    kw = dict(PIN[name])
    case = lc.shape_case(65, kw.pop("A", 25), **kw)
    ref = lm.model_torch(case.cfg, case.inp, torch.float64)
    for k in ("dlogits", "dvalues", "imp_weights", "stats", "vn_state", "denorm"):
        if k not in ref:
            continue
        scale = max(1e-300, float(np.abs(case.w64[k]).max()))
        err = float(np.abs(ref[k] - case.w64[k]).max())
        print("pin %s %s: %.3e relative" % (name, k, err / scale))
        assert err <= 1e-13 * scale, (name, k, err)


def test_named_branch_points_agree_with_torch_autograd_in_double_ties_included():
    """Rows exactly on a branch point -- values - value_preds = +-c, e = +-delta, e < -delta, adv = 0, logp =
    old -- against torch's autograd in double, which resolves the ties by its own rules (half the gradient to
    each argument of min / max, clamp's ends included)."""
    import torch
    cfg, inp, names = lc.named_inputs()
    w, ref = lm.model64(cfg, inp), lm.model_torch(cfg, inp, torch.float64)
    i = names.index
    assert w["d"][i("d = +c")] == 0.25 and w["d"][i("d = -c")] == -0.25
    assert w["e_o"][i("e = +delta")] == 10 and w["e_o"][i("e = -delta")] == -10
    assert w["l_o"][i("e < -delta")] == 0 and w["dvalues"][i("e < -delta")] == 0 and w["l_o"][i("e = -delta")] == 50
    assert w["l_o"][i("d = +c")] == w["l_c"][i("d = +c")] and w["dvalues"][i("d = +c")] != 0
    assert abs(w["ratio"][i("logp = old")] - 1) < 1e-15 and (w["dlogits"][i("adv = 0")] != 0).any()
    assert w["dvalues"][i("clipped wins outside")] == 0 and w["dvalues"][i("plain")] == 0   # cut by the clamp; inactive
    for k in ("dlogits", "dvalues", "imp_weights", "stats"):
        np.testing.assert_allclose(ref[k], w[k], rtol=0, atol=1e-14, err_msg=k)


def test_the_reference_fixtures_are_there():
    assert sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz"))) == ["all_off", "all_on"]


def _fixture(name):
    z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    cfg = LossConfig(num_actions=int(z["num_actions"]),
                     **{k: float(z[k]) for k in ("clip_param", "huber_delta", "value_loss_coef", "entropy_coef", "vn_beta")},
                     **{k: bool(z[k]) for k in lc.FLAGS})
    inp = {k[3:]: v for k, v in z.items() if k.startswith("in_")}
    inp.setdefault("avail", None)
    return z, cfg, inp


@pytest.mark.parametrize("name", ["all_on", "all_off"])
def test_model64_reproduces_the_reference(name):
    """GR_MAPPO.ppo_update itself in float64 on a stub policy (tests/golden/make_loss_golden.py): model64
    agrees to 1e-12 on both gradients, the importance weights, the four scalars and the normaliser."""
    z, cfg, inp = _fixture(name)
    on = name == "all_on"
    assert all(getattr(cfg, f) == on for f in lc.FLAGS) and (inp["active"] == 0).any()
    assert (inp["avail"] is not None and (inp["avail"] == 0).any()) == on
    got = lm.model64(cfg, inp)
    w = got["ratio"]
    assert (w < 0.75).any() and (w > 1.25).any() and ((w > 0.75) & (w < 1.25)).any()
    assert (np.abs(got["d"]) > 0.25).any() and (np.abs(got["d"]) < 0.25).any()
    if on:
        assert cfg.huber_delta == 1 and (got["e_o"] > 1).any() and (got["e_o"] < -1).any() and (np.abs(got["e_o"]) < 1).any()
    for k in ("dlogits", "dvalues", "imp_weights", "stats"):
        assert got[k].shape == z[k].shape, k
        np.testing.assert_allclose(got[k], z[k], rtol=0, atol=1e-12, err_msg=k)
    if on:
        np.testing.assert_allclose(got["vn_state"], z["vn_state_out"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(got["denorm"], z["denorm"], rtol=0, atol=1e-12)
    else:
        assert "denorm" not in z


@pytest.mark.parametrize("name", ["all_on", "all_off"])
def test_host_reproduces_the_reference_fixture(lib, name):
    _, cfg, inp = _fixture(name)
    lc.check(lib, lc.Case("fixture " + name, cfg, inp))


def _listed_cases():
    out = [dict(M=M, A=25) for M in lc.MS] + [dict(M=65, A=A) for A in lc.AS]
    out += [dict(M=257, A=25, **{f: not getattr(lc.DEFAULTS, f)}) for f in lc.FLAGS]
    out += [dict(M=65, A=25, avail="some"), dict(M=65, A=25, active="zero"), dict(M=65, A=25, active="ones")]
    return out


def test_the_generator_terminates_and_leaves_no_row_near_a_branch_point():
    """Every listed case: the redraws end (a few rounds), no row of the case is within the margin of a branch
    point in the float64 model, and every row is still there."""
    for kw in _listed_cases():
        kw = dict(kw)
        M, A = kw.pop("M"), kw.pop("A")
        avail, active = kw.pop("avail", None), kw.pop("active", "some")
        cfg = dataclasses.replace(lc.DEFAULTS, num_actions=A, **kw)
        inp, rounds = lc.random_inputs(cfg, M, seed=M + 7 * A, avail=avail, active=active)
        assert rounds <= 20, (kw, rounds)
        w = lm.model64(cfg, inp)
        assert not lc.near_branch(cfg, w).any() and w["ratio"].shape == (M,) and inp["old"].shape == (M,)
        if M >= 63:   # the branches are all taken
            lo, hi = 1 - cfg.clip_param, 1 + cfg.clip_param
            assert (w["ratio"] < lo).any() and (w["ratio"] > hi).any() and (np.abs(w["d"]) > cfg.clip_param).any()
            assert (np.abs(w["e_o"]) > cfg.huber_delta).any()


# ---- parity of the host entry point -----------------------------------------------------------------------

@pytest.mark.parametrize("M", lc.MS)
def test_host_rows(lib, M):
    lc.check(lib, lc.shape_case(M, 25))


def test_host_more_groups_than_one_stage(lib):
    lc.check(lib, lc.shape_case(lc.MANY, 5))


@pytest.mark.parametrize("A", lc.AS)
def test_host_actions(lib, A):
    lc.check(lib, lc.shape_case(65, A))


@pytest.mark.parametrize("flag", lc.FLAGS)
def test_host_one_flag_off(lib, flag):
    case = lc.shape_case(257, 25, **{flag: False})
    got = lc.check(lib, case)
    base = lc.shape_case(257, 25)
    assert not getattr(case.cfg, flag) and getattr(base.cfg, flag)
    assert np.abs(case.w64["stats"] - lm.model64(base.cfg, case.inp)["stats"]).max() > 1e-4   # the flag counts
    assert ("denorm" in got) == (flag != "use_valuenorm")


def test_host_every_flag_off(lib):
    lc.check(lib, lc.shape_case(65, 25, **{f: False for f in lc.FLAGS}))


@pytest.mark.parametrize("half", ["actor", "critic"])
def test_host_one_half_alone(lib, half):
    """A null logits / values skips that half: its outputs, its statistics and (actor alone) the normaliser
    are not written, and the other half's outputs are the same bytes as in the full call."""
    full = lc.shape_case(257, 25)
    both, _, _ = lc.run(lib, full.cfg, full.inp)
    case = lc.Case("only " + half, full.cfg, full.inp, actor=half == "actor", critic=half == "critic")
    got = lc.check(lib, case)
    assert set(got) - {"vn_state"} == ({"dlogits", "imp_weights", "stats"} if half == "actor"
                                        else {"dvalues", "stats", "denorm"})
    for k in got:
        if k == "stats":
            keep = [0, 2, 3] if half == "actor" else [1]
            np.testing.assert_array_equal(got[k][keep].view(np.int32), both[k][keep].view(np.int32))
        elif k != "vn_state":
            np.testing.assert_array_equal(got[k].view(np.int32), both[k].view(np.int32), err_msg=k)
    # a half alone does not need the other half's inputs, nor active_masks when only the other half's flag asks
    cfg = dataclasses.replace(full.cfg, **{"use_value_active_masks" if half == "critic" else "use_policy_active_masks": False})
    lc.run(lib, cfg, dict(full.inp, active=None), actor=half == "actor", critic=half == "critic")


def test_host_available_actions(lib):
    """Row 1 with one available action, row 2 with none (uniform), row 3 storing an unavailable action (ratio
    0): the model's values, and dlogits exactly 0 on every unavailable entry (lc.check asserts it)."""
    case = lc.shape_case(65, 25, avail="some")
    av = case.inp["avail"]
    assert av[1].sum() == 1 and av[2].sum() == 0 and av[3, int(case.inp["actions"][3])] == 0 and (av == 0).sum() > 65
    got = lc.check(lib, case)
    assert (got["dlogits"][2] == 0).all() and got["imp_weights"][3] == 0
    np.testing.assert_allclose(case.w64["logp"][2], -np.log(25), rtol=0, atol=1e-12)
    assert (got["dlogits"][av != 0] != 0).sum() > 500
    # logits that already hold the mask (as lsm_head_evaluate writes them) give the same bytes, with the
    # availability passed again or not at all -- except the exact zeros, which need it
    masked = np.where(av == 0, np.float32(lm.FLT_MIN), case.inp["logits"])
    twice, _, _ = lc.run(lib, case.cfg, dict(case.inp, logits=masked))
    alone, _, _ = lc.run(lib, case.cfg, dict(case.inp, logits=masked, avail=None))
    for k in got:
        if k != "vn_state":
            np.testing.assert_array_equal(twice[k].view(np.int32), got[k].view(np.int32), err_msg=k)
    for k in ("imp_weights", "stats", "dvalues"):
        np.testing.assert_array_equal(alone[k].view(np.int32), got[k].view(np.int32), err_msg=k)
    some = av.sum(axis=1) > 0
    np.testing.assert_array_equal(alone["dlogits"][some][av[some] != 0], got["dlogits"][some][av[some] != 0])


def test_host_bad_actions(lib):
    """2.5, -1, A and NaN in one row each: *bad is set, the row is the clamped action's, every other row is
    unchanged; *bad is never cleared by a call."""
    case = lc.shape_case(257, 25)
    clean, bad, _ = lc.run(lib, case.cfg, case.inp)
    assert bad == 0
    for r, v, want in ((3, 2.5, 2), (130, -1.0, 0), (200, 25.0, 24), (256, np.nan, 0)):
        acts = case.inp["actions"].copy()
        acts[r] = v
        inp = dict(case.inp, actions=acts)
        c, flagged = lm.clamp_actions(acts, 25)
        assert np.nonzero(flagged)[0].tolist() == [r] and c[r] == want
        got, bad, _ = lc.run(lib, case.cfg, inp)
        assert bad == 1, (r, v)
        w = lm.model64(case.cfg, inp)
        assert abs(float(got["imp_weights"][r]) - w["ratio"][r]) <= case.tol["imp_weights"][0] + lc.EPS * w["ratio"][r]
        keep = np.arange(case.M) != r
        for k in ("dlogits", "imp_weights", "dvalues"):
            np.testing.assert_array_equal(got[k][keep].view(np.int32), clean[k][keep].view(np.int32), err_msg=k)
    _, bad, _ = lc.run(lib, case.cfg, case.inp, bad_init=5)
    assert bad == 5


@pytest.mark.parametrize("active", ["ones", "zero"])
def test_host_active_masks(lib, active):
    """All active: the weighted means are the plain means. None active: 0 / 0 -- the two weighted losses and
    dist_entropy are NaN, the gradients NaN or (where torch's masked_fill cuts a branch) exactly 0, as in
    torch; the unweighted mean ratio and the normaliser are not affected."""
    case = lc.shape_case(65, 25, active=active)
    got = lc.check(lib, case)
    if active == "zero":
        assert np.isnan(got["stats"][:3]).all() and np.isfinite(got["stats"][3])
        assert np.isnan(got["dlogits"]).all() and np.isnan(got["dvalues"]).any() and (got["dvalues"] == 0).any()
        assert np.isfinite(got["denorm"]).all()
    else:
        off = dataclasses.replace(case.cfg, use_value_active_masks=False, use_policy_active_masks=False)
        plain, _, _ = lc.run(lib, off, case.inp)
        np.testing.assert_array_equal(plain["stats"].view(np.int32), got["stats"].view(np.int32))


def test_host_named_branch_points(lib):
    """The named rows through the host entry point: on float32 inputs the branch points are exact there too."""
    cfg, inp, names = lc.named_inputs()
    inp = {k: (np.asarray(v, np.float32) if v is not None else None) for k, v in inp.items()}
    w = lm.model64(cfg, inp)
    i = names.index
    assert w["d"][i("d = +c")] == 0.25 and w["e_o"][i("e = -delta")] == -10 and w["e_o"][i("e = +delta")] == 10
    case = lc.Case("named", cfg, inp)
    got = lc.check(lib, case)
    assert got["dvalues"][i("e < -delta")] == 0 and got["dvalues"][i("clipped wins outside")] == 0
    assert got["dvalues"][i("d = +c")] != 0 and got["dvalues"][i("d = -c")] != 0


# ---- the normaliser -----------------------------------------------------------------------------------------

def _reference_valuenorm_f32(state, returns, beta=0.99999, epsilon=1e-5):
    """ValueNorm.update and running_mean_var (onpolicy/utils/valuenorm.py) as float32 torch ops, its Python
    scalars as they are: (state', sqrt(var), mean)."""
    import torch
    rm, rms, db = (torch.tensor([float(v)], dtype=torch.float32) for v in state)
    x = torch.tensor(np.asarray(returns), dtype=torch.float32).reshape(-1, 1)
    batch_mean, batch_sq_mean = x.mean(dim=(0,)), (x ** 2).mean(dim=(0,))
    weight = beta
    rm.mul_(weight).add_(batch_mean * (1.0 - weight))
    rms.mul_(weight).add_(batch_sq_mean * (1.0 - weight))
    db.mul_(weight).add_(1.0 * (1.0 - weight))
    mean = rm / db.clamp(min=epsilon)
    var = (rms / db.clamp(min=epsilon) - mean ** 2).clamp(min=1e-2)
    return np.array([rm.item(), rms.item(), db.item()], np.float32), np.float32(torch.sqrt(var).item()), np.float32(mean.item())


@pytest.mark.parametrize("state", [(0.0, 0.0, 0.0), (0.1, 0.75, 0.5)], ids=["fresh", "seen data"])
def test_valuenorm_state_is_the_reference_formulas_bit_for_bit(lib, state):
    """Returns that are small integers (M = 512, sums and sums of squares exact in float32 and float64): the
    state after the update is bit-equal to the reference's formulas run as float32 torch, denorm is sqrtf(var)
    and mean of that state, and a second call gives the second update."""
    cfg = lc.DEFAULTS
    inp, _ = lc.random_inputs(cfg, 512, seed=9)
    rng = np.random.default_rng(5)
    inp = dict(inp, returns=rng.integers(-8, 9, 512).astype(np.float32), vn_state=np.array(state, np.float32))
    want, sd, mean = _reference_valuenorm_f32(state, inp["returns"])
    got, _, st = lc.run(lib, cfg, inp)
    np.testing.assert_array_equal(st.view(np.int32), want.view(np.int32))
    np.testing.assert_array_equal(got["denorm"].view(np.int32), np.array([sd, mean], np.float32).view(np.int32))
    inp2 = dict(inp, returns=rng.integers(-8, 9, 512).astype(np.float32), vn_state=st)
    want2, sd2, mean2 = _reference_valuenorm_f32(want, inp2["returns"])
    got2, _, st2 = lc.run(lib, cfg, inp2)
    np.testing.assert_array_equal(st2.view(np.int32), want2.view(np.int32))
    np.testing.assert_array_equal(got2["denorm"].view(np.int32), np.array([sd2, mean2], np.float32).view(np.int32))
    assert (st2 != st).all()
    # every row was normalised with the updated state
    tg = (inp["returns"].astype(np.float64) - float(mean)) / float(sd)
    w = lm.model64(cfg, inp)
    assert np.abs(w["e_o"] - (tg - inp["values"])).max() < 1e-5


# ---- the chain rule, end to end -----------------------------------------------------------------------------

def _heads_forward(mods, inp, Cn, T, dtype):
    """tests/evaluate_model.py's TorchEval with the graph kept: logits [R, A] or values [R]."""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
    x = torch.cat([t(inp[k]) for k in ("x0", "x1") if inp[k] is not None], dim=1)
    x = mods.fn(x)
    for seq in mods.fc:
        x = seq(x)
    h = t(inp["states"]).transpose(0, 1).contiguous()
    mk = t(inp["masks"]).view(T, Cn)
    tops = []
    for l in range(T):
        h = h * mk[l].view(1, Cn, 1)
        y, h = mods.gru(x[l * Cn:(l + 1) * Cn].unsqueeze(0), h)
        tops.append(y.squeeze(0))
    out = mods.out(mods.norm(torch.cat(tops, dim=0)))
    return out if mods.cfg.kind == "actor" else out.reshape(-1)


def _params(mods):
    out = {}
    for name, mod in [("fn", mods.fn), ("gru", mods.gru), ("norm", mods.norm), ("out", mods.out)] + \
            [("fc%d" % k, m) for k, m in enumerate(mods.fc)]:
        for pn, p in mod.named_parameters():
            out["%s.%s" % (name, pn)] = p
    return out


def test_chain_rule_through_the_heads(lib):
    """The torch modules of tests/evaluate_model.py in float32 produce logits and values; the host entry point
    turns them into dlogits and dvalues; torch.autograd.backward([logits, values], [dlogits, dvalues]) gives
    every parameter's gradient. Each must match the all-torch loss.backward() of the same minibatch within the
    measured criterion, e32 being the float32-against-double difference of the all-torch gradients."""
    import torch
    A, Cn, T = 5, 7, 3
    R = Cn * T
    acfg = policy.HeadConfig(kind="actor", in0=6, in1=4, hidden=16, recurrent_N=1, num_actions=A)
    ccfg = policy.HeadConfig(kind="critic", in0=9, in1=4, hidden=16, recurrent_N=1)
    asd, csd = pm.random_head_weights(acfg, 21), pm.random_head_weights(ccfg, 22)
    ain = em.random_inputs(acfg, Cn, T, seed=3, mask_zeros=True, active="some")
    cin = em.random_inputs(ccfg, Cn, T, seed=4, mask_zeros=True)
    for d in (ain, cin):   # ordinary initial states under the zero masks: this test is about gradients
        d["states"] = np.clip(d["states"], -1, 1)
    cfg = LossConfig(num_actions=A)

    def forward(dtype):
        am, cm = pm.TorchHead(acfg, asd, dtype), pm.TorchHead(ccfg, csd, dtype)
        for p in list(_params(am).values()) + list(_params(cm).values()):
            p.requires_grad_(True)
        return am, cm, _heads_forward(am, ain, Cn, T, dtype), _heads_forward(cm, cin, Cn, T, dtype)

    am, cm, logits, values = forward(torch.float32)
    rng = np.random.default_rng(11)
    inp = {"logits": logits.detach().numpy(), "values": values.detach().numpy(), "actions": ain["actions"],
           "avail": None, "adv": rng.normal(size=R).astype(np.float32), "active": ain["active"].reshape(R),
           "vn_state": lc.VN_STATE.copy(), "old": np.zeros(R, np.float32), "vpreds": np.zeros(R, np.float32),
           "returns": np.zeros(R, np.float32)}
    logp = lm.model64(cfg, inp, critic=False)["logp"]
    rows = np.arange(R)
    for _ in range(100):   # lc.settle, with the values left to the network
        k = len(rows)
        inp["old"][rows] = (logp[rows] + 0.25 * rng.normal(size=k)).astype(np.float32)
        inp["vpreds"][rows] = inp["values"][rows] + (0.3 * rng.normal(size=k)).astype(np.float32)
        inp["returns"][rows] = (0.5 + 2.0 * rng.normal(size=k)).astype(np.float32)
        rows = np.nonzero(lc.near_branch(cfg, lm.model64(cfg, inp)))[0]
        if rows.size == 0:
            break
    assert rows.size == 0
    got, bad, _ = lc.run(lib, cfg, inp)
    assert bad == 0
    torch.autograd.backward([logits, values], [torch.from_numpy(got["dlogits"]), torch.from_numpy(got["dvalues"])])
    mine = {"actor." + k: p.grad.double().numpy() for k, p in _params(am).items()}
    mine.update({"critic." + k: p.grad.double().numpy() for k, p in _params(cm).items()})

    def all_torch(dtype):
        am_, cm_, lg, vl = forward(dtype)
        obj = lm.torch_objectives(cfg, lg, vl, inp, dtype)
        obj["actor"].backward()
        obj["critic"].backward()
        g = {"actor." + k: p.grad.double().numpy() for k, p in _params(am_).items()}
        g.update({"critic." + k: p.grad.double().numpy() for k, p in _params(cm_).items()})
        return g

    g32, g64 = all_torch(torch.float32), all_torch(torch.float64)
    assert set(mine) == set(g64) and len(mine) == 2 * (2 + 2 * 4 + 4 + 2 + 2)
    for k in sorted(g64):
        tol, e32 = lm.tensor_bound(g64[k], g32[k])
        assert np.abs(g64[k]).max() > 0, k
        lc.assert_close(mine[k], g64[k], tol, e32, "chain rule " + k)


# ---- argument refusals: nonzero and a text, before any launch or write -------------------------------------

REFUSALS = {
    "null io": dict(over=dict(io=None)),
    "null stats": dict(over=dict(stats=None)),
    "null scratch": dict(over=dict(scratch=None)),
    "both halves null": dict(over=dict(logits=None, values=None)),
    "actor without actions": dict(over=dict(actions=None)),
    "actor without old_log_probs": dict(over=dict(old_log_probs=None)),
    "actor without advantages": dict(over=dict(advantages=None)),
    "actor without dlogits": dict(over=dict(dlogits=None)),
    "critic without value_preds": dict(over=dict(value_preds=None)),
    "critic without returns": dict(over=dict(returns=None)),
    "critic without dvalues": dict(over=dict(dvalues=None)),
    "flags without active_masks": dict(over=dict(active_masks=None)),
    "policy flag without active_masks": dict(over=dict(active_masks=None), cfg=dict(use_value_active_masks=False)),
    "value flag without active_masks": dict(over=dict(active_masks=None), cfg=dict(use_policy_active_masks=False)),
    "valuenorm without vn_state": dict(over=dict(vn_state=None)),
    "misaligned logits": dict(add=dict(logits=2)),
    "misaligned actions": dict(add=dict(actions=1)),
    "misaligned returns": dict(add=dict(returns=2)),
    "misaligned dvalues": dict(add=dict(dvalues=2)),
    "misaligned stats": dict(add=dict(stats=2)),
    "misaligned vn_state": dict(add=dict(vn_state=2)),
    "misaligned scratch": dict(add=dict(scratch=4)),
    "misaligned bad": dict(add=dict(bad=4)),
    "M < 0": dict(over=dict(M=-1)),
    "M * A = 2^31": dict(over=dict(M=2 ** 31 // 25 + 1)),
    "A = 0": dict(cfg=dict(num_actions=0)),
    "A = 65": dict(cfg=dict(num_actions=65)),
    "clip < 0": dict(cfg=dict(clip_param=-0.1)),
    "clip NaN": dict(cfg=dict(clip_param=float("nan"))),
    "clip inf": dict(cfg=dict(clip_param=float("inf"))),
    "delta < 0": dict(cfg=dict(huber_delta=-1.0)),
    "delta NaN": dict(cfg=dict(huber_delta=float("nan"))),
    "beta < 0": dict(cfg=dict(vn_beta=-0.5)),
    "beta inf": dict(cfg=dict(vn_beta=float("inf"))),
    "dlogits overlaps logits": dict(alias=("dlogits", "logits", 0)),
    "dlogits overlaps the end of logits": dict(alias=("dlogits", "logits", 4 * (9 * 25 - 1))),
    "dvalues overlaps values": dict(alias=("dvalues", "values", 0)),
    "dvalues overlaps returns": dict(alias=("dvalues", "returns", 4)),
    "imp_weights overlaps old_log_probs": dict(alias=("imp_weights", "old_log_probs", 0)),
    "stats overlaps advantages": dict(alias=("stats", "advantages", 8)),
    "scratch overlaps active_masks": dict(alias=("scratch", "active_masks", 0)),
    "vn_state overlaps returns": dict(alias=("vn_state", "returns", 0)),
    "denorm overlaps vn_state": dict(alias=("denorm", "vn_state", 4)),
    "dvalues overlaps imp_weights": dict(alias=("dvalues", "imp_weights", 0)),
}


def _refusal_case():
    return lc.shape_case(9, 25)


@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_refusals(lib, what):
    spec = REFUSALS[what]
    case = _refusal_case()
    cfg = dataclasses.replace(case.cfg, **spec.get("cfg", {}))
    if cfg.num_actions != 25:   # the buffers keep their 25 columns
        st = cfg.struct()
        cfg = dataclasses.replace(cfg, num_actions=25)
        lc.run(lib, cfg, case.inp, expect_rc=1, bad_init=3, over=dict(cfg=st))
        return
    lc.run(lib, cfg, case.inp, expect_rc=1, bad_init=3, over=spec.get("over"), add=spec.get("add"),
           alias=spec.get("alias"))


def test_refusal_case_is_accepted_unchanged_and_empty_is_legal(lib):
    """The refusal tests' call succeeds without its one change; M == 0 writes nothing (lc.run checks every
    output, the scratch and vn_state) and is no error."""
    case = _refusal_case()
    lc.check(lib, case)
    inp = {k: (v[:0] if isinstance(v, np.ndarray) and k != "vn_state" else v) for k, v in case.inp.items()}
    got, bad, st = lc.run(lib, case.cfg, inp, M=0)
    assert got == {} and bad == 0


def test_optional_outputs_may_be_null(lib):
    case = lc.shape_case(65, 25)
    full, _, _ = lc.run(lib, case.cfg, case.inp)
    got, _, _ = lc.run(lib, case.cfg, case.inp, skip=("imp_weights", "denorm"), over=dict(bad=None))
    assert set(got) == {"dlogits", "dvalues", "stats"}
    for k in got:
        np.testing.assert_array_equal(got[k].view(np.int32), full[k].view(np.int32), err_msg=k)
