"""CPU tests of the heads' backward pass (include/lsm_backward.h): the header and its exports, the float64
yardstick (tests/heads_backward_model.py: the torch.nn modules under autograd) pinned against fixtures recorded
from the reference's own MLPBase / RNNLayer / ACTLayer under loss.backward() (tests/golden/heads_backward/),
lsm_host_head_backward -- the per-chunk text the kernels run, with the kernels' slab grouping -- against it
within the tolerance measured per case and gradient tensor (4 * e32 + 4 * 2^-23 * s), masks, availability,
slab boundaries, the exact-zero structure, the chain through lsm_host_ppo_loss's seeds, and the argument
refusals (which return before any launch or write, so they need no device)."""
import glob
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import evaluate_cases as ec
import evaluate_model as em
import heads_backward_cases as hc
import heads_backward_model as hm
import loss_cases as lc
import loss_model as lm
import policy_model as pm
from lsm import capi, policy
from lsm.loss import LossConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_backward.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "heads_backward")


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
    text = open(HDR).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_BACKWARD) and len(declared) == 3
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE, capi.EXPORTED_LOSS):
        assert not declared & set(other)
    assert "lsm_head_tile.h" in build.UNITS["lsm_backward.hip"]
    body = hdr[hdr.index("typedef struct lsm_bwd_io"):hdr.index("} lsm_bwd_io")]
    assert re.findall(r"\*\s*(\w+);", body) == [f for f, _ in capi.LsmBwdIo._fields_]
    assert int(re.search(r"#define LSM_BWD_SLAB (\d+)", text).group(1)) == capi.LSM_BWD_SLAB


def test_the_forward_pieces_are_the_shared_ones(lib):
    """The backward recomputes the forward with csrc/lsm_head_tile.h's text, and the rollout's build id does
    not cover the new unit."""
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_backward.hip", "lsm_backward.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    src = open(os.path.join(build.CSRC, "lsm_backward.hip")).read()
    assert '#include "lsm_head_tile.h"' in src and "lsm_rollout.h" not in src
    shared = open(os.path.join(build.CSRC, "lsm_head_tile.h")).read()
    for piece in ("void dot4(", "void linear(", "void layer_norm(", "float row_sum(", "void save_rows(",
                  "void load_rows(", "void mlp(", "void gru_layer("):
        assert piece in shared and piece not in src, piece
    # stage 1 has no MLP or GRU cell of its own: it calls the shared ones with its hook, and copies through the
    # shared loops
    stage1 = src.split("// ---- stage 2")[0].split("namespace {")[1]
    for call in ("mlp(n, w, ", "gru_layer(n, w, ", ", keep);", "load_rows(", "save_rows("):
        assert call in stage1, call
    for text in ("linear(", "sigmoid_(", "gru_layer_save"):
        assert text not in stage1, text
    assert "ranges_overlap" not in src and "groups_of" not in src
    # no atomics: the launches' once-per-device flags live in lsm_head_tile.h's launch()
    assert "atomic" not in src


def test_workspace_bytes(lib):
    f = lib.lsm_head_backward_workspace_bytes
    st = hc.ACTOR.struct()
    assert f(st, -1, 1) == 0 and f(st, 1, 0) == 0 and f(st, 2 ** 30, 2) == 0
    nw = int(lib.lsm_head_weights_floats(st))
    assert f(st, 0, 1) == 8
    c = hc.ACTOR
    n, Hd, L, RN, A = c.in0 + c.in1, c.hidden, c.layer_N, c.recurrent_N, c.num_actions
    # the header's list: stage 1's saves, then stage 2's, in floats per row
    per_row = (n + (L + 1) * 2 * Hd + RN * 6 * Hd + Hd) + (A + 2 * Hd + RN * 6 * Hd + (L + 1) * 3 * Hd + 2 * n)
    up8 = lambda b: (b + 7) // 8 * 8
    S = capi.LSM_BWD_SLAB
    assert f(st, 1, 1) == up8(4 * (per_row + nw)) and f(st, S, 1) == up8(4 * (S * per_row + nw))
    assert f(st, S + 1, 1) == up8(4 * ((S + 1) * per_row + 2 * nw))      # a second slab's partial blob
    assert f(st, 64, 32) == f(st, S, 1)                                  # by rows, however they are chunked


# ---- the yardstick itself -----------------------------------------------------------------------------------

def _fixtures():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")))


def test_the_reference_fixtures_are_there():
    assert _fixtures() == ["t4_c3_rn1", "t4_c3_rn2"]


@pytest.mark.parametrize("name", ["t4_c3_rn1", "t4_c3_rn2"])
def test_model64_agrees_with_the_reference_backward(name):
    """The reference's own modules in float64 backpropagated J = sum_m c_m * log_probs_m + kappa * dist_entropy;
    the fixture holds c, kappa and every parameter's .grad. dlogits follows from c and kappa in closed form
    (tests/loss_model.py's), and the float64 yardstick seeded with it must give the same gradients within
    1e-10 * max |grad| on every tensor."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    cfg = policy.HeadConfig(kind="actor", in0=int(z["in0"]), in1=int(z["in1"]), hidden=int(z["hidden"]),
                            layer_N=int(z["layer_N"]), relu=bool(z["relu"]), feature_norm=bool(z["feature_norm"]),
                            recurrent_N=int(z["recurrent_N"]), num_actions=int(z["num_actions"]))
    Cn, T = int(z["C"]), int(z["T"])
    names = [n for n, _ in policy.head_weight_entries(cfg)]
    sd = {k: z["w_" + k] for k in names}
    inp = {k: z[k] for k in ("x0", "x1", "states", "masks", "actions", "avail", "active")}
    import torch
    model = hm.TorchBackward(cfg, sd, torch.float64)
    logits = model.forward(inp, Cn, T)[0].detach().numpy()
    seed = hm.dlogits_of(logits, inp["actions"], z["c"], float(z["kappa"]), inp["avail"], inp["active"])
    g = model(inp, seed, Cn, T)
    for k in names:
        want = z["g_" + k]
        scale = float(np.abs(want).max())
        err = float(np.abs(g[k] - want).max())
        print("reference pin %s %s: %.3e of %.3e" % (name, k, err, scale))
        assert scale > 0 and err <= 1e-10 * scale, (name, k, err, scale)


# ---- the host entry point against the yardstick --------------------------------------------------------------

@pytest.mark.parametrize("kind", ["actor", "critic"])
@pytest.mark.parametrize("shape", hc.SHAPES, ids=lambda s: "C%d_T%d" % s)
def test_host_shapes(lib, kind, shape):
    hc.check(lib, hc.shape_case(kind, *shape))


@pytest.mark.parametrize("name", sorted(ec.OPTIONS))
def test_host_options(lib, name):
    hc.check(lib, hc.option_case(name))


@pytest.mark.parametrize("name", ec.BACKWARD_PLAN_NAMES)
def test_host_plan_cases(lib, name):
    """One case per launch plan and size limit (evaluate_cases.PLAN_OPTIONS, the limits found through
    lsm_head_plan); past an LDS limit the call is refused and writes nothing."""
    hc.plan_checks(lib, name, None)


@pytest.mark.parametrize("name", hc.TWICE_PLAN)
def test_host_plan_cases_twice(lib, name):
    hc.plan_twice_checks(lib, name, None)


@pytest.mark.parametrize("which", [0, 1], ids=["actor recurrent_N 2 masks", "critic recurrent_N 1"])
def test_host_backwards_forward_is_evaluates(lib, which):
    """lsm_host_head_backward's saved features and last h' are lsm_host_head_evaluate's outputs to the byte
    (workspace offsets from lsm_head_plan)."""
    hc.forward_is_evaluates(lib, hc.forward_cases()[which], None)


@pytest.mark.parametrize("kind", ["actor", "critic"])
def test_host_zero_masks(lib, kind):
    case = hc.masks_case(kind)
    mk = case.inp["masks"].reshape(case.T, case.C)
    assert (mk[0] == 0).any() and (mk[1:] == 0).any() and (mk == 1).any()
    hc.check(lib, case)


def test_host_available_actions(lib):
    hc.avail_checks(lib, None)


@pytest.mark.parametrize("kind", ["actor", "critic"])
@pytest.mark.parametrize("rows", [hc.SLAB - 1, hc.SLAB, hc.SLAB + 1, 3 * hc.SLAB + 2])
def test_host_slab_boundaries(lib, kind, rows):
    hc.check(lib, hc.slab_case(kind, rows))


def test_host_structure(lib):
    hc.structure_checks(lib, None)


def test_host_twice_and_null_outputs(lib):
    hc.twice_and_null_checks(lib, None)


def test_refusals(lib):
    hc.refusal_checks(lib, None)


def test_the_ratios(lib):
    """The largest err / e32 and err / tol of the comparisons this session made (for DESIGN.md)."""
    rows = [r for r in pm.RATIOS if r[0].startswith("backward ")]
    if rows:
        fin = [r for r in rows if np.isfinite(r[1])]
        print("backward: %d comparisons, max err/e32 %.2f (%s), max err/tol %.3f (%s)" % (
            len(rows), max(r[1] for r in fin), max(fin, key=lambda r: r[1])[0], max(r[2] for r in rows),
            max(rows, key=lambda r: r[2])[0]))


# ---- through the public seeds ---------------------------------------------------------------------------------

def test_chain_rule_from_the_loss_to_the_weights(lib):
    """The torch modules in float32 produce logits and values; lsm_host_ppo_loss turns them into dlogits and
    dvalues; lsm_host_head_backward turns those into every parameter's gradient and dx. Each must match the
    all-torch loss.backward() of the same minibatch within the criterion, e32 being the float32-against-double
    difference of the all-torch gradients (tests/test_loss_capi.py's chain-rule case, one stage further)."""
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
        am, cm = hm.TorchBackward(acfg, asd, dtype), hm.TorchBackward(ccfg, csd, dtype)
        return am, cm, am.forward(ain, Cn, T), cm.forward(cin, Cn, T)

    am, cm, fa, fc = forward(torch.float32)
    rng = np.random.default_rng(11)
    inp = {"logits": fa[0].detach().numpy(), "values": fc[0].detach().numpy().reshape(R), "actions": ain["actions"],
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
    mine = {}
    for pre, hcfg, sd, hin, seed in (("actor.", acfg, asd, ain, got["dlogits"]), ("critic.", ccfg, csd, cin, got["dvalues"])):
        g = hc.run(lib, hcfg, policy.pack_head_weights(sd, hcfg), hin, seed, Cn, T)
        mine.update({pre + k: v for k, v in hc.entries(hcfg, g["dweights"]).items()})
        mine[pre + "dx0"], mine[pre + "dx1"] = g["dx0"], g["dx1"]

    def all_torch(dtype):
        am_, cm_, a, c = forward(dtype)
        obj = lm.torch_objectives(cfg, a[0], c[0].reshape(-1), inp, dtype)
        obj["actor"].backward()
        obj["critic"].backward()
        g = {}
        for pre, m, f in (("actor.", am_, a), ("critic.", cm_, c)):
            g.update({pre + k: p.grad.double().numpy() for k, p in m.params.items()})
            g[pre + "dx0"], g[pre + "dx1"] = f[1].grad.double().numpy(), f[2].grad.double().numpy()
        return g

    g32, g64 = all_torch(torch.float32), all_torch(torch.float64)
    assert set(mine) == set(g64)
    for k in sorted(g64):
        tol, e32 = lm.tensor_bound(g64[k], g32[k])
        assert np.abs(g64[k]).max() > 0, k
        lc.assert_close(mine[k], g64[k], tol, e32, "backward chain rule " + k)
