"""CPU tests of the launch plans of the four learner-side kernels, read through lsm_gnn_plan (include/lsm_gnn.h)
and lsm_head_plan (include/lsm_policy.h), which fill a struct from the launches' own make_net / make_eval /
make_plan and launch nothing:

- every acceptance boundary is found by walking the library (tests/launch_plans.py) and compared with the
  numbers the headers state; the last accepted size fits the 163840 bytes of LDS and the next one is refused
  with the LDS text;
- the plan agrees with what the headers document about it (the row strides hold their rows, the adjacency is
  staged exactly when E * E more floats fit, the stage-3 tiles cover every job);
- the coverage assertion: the plans of the cases that tests/gnn_cases.py, evaluate_cases.py and
  heads_backward_cases.py export (run by the *_capi.py files on the host entry points and by the test_gpu_*.py
  files on the kernels) contain every branch of the plan. Retune a heuristic and this names the branch that
  lost its case."""
import dataclasses
import os
import re

import pytest

import evaluate_cases as ec
import gnn_cases as gc
import heads_backward_cases as hc
import launch_plans as lp
import policy_cases as pc
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTINES = ("forward", "evaluate", "backward")
KINDS = {"actor": pc.ACTOR, "critic": pc.CRITIC}


def pad(w):
    """The headers' pad(w) = round_up(w, 4) + 4."""
    return (w + 3) // 4 * 4 + 4


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def struct_fields(text, name):
    body = text[text.index("typedef struct %s {" % name):text.index("} %s;" % name)]
    body = re.sub(r"/\*.*?\*/", "", body[body.index("{") + 1:], flags=re.S)
    out = []
    for decl in re.findall(r"(?:int32_t|int64_t|lsm_head_plan_job)\s+([^;]+);", body):
        out += [re.sub(r"\[.*", "", f.strip()) for f in decl.split(",")]
    return out


def test_the_structs_are_the_headers():
    assert struct_fields(header("lsm_gnn.h"), "lsm_gnn_launch_plan") == [f for f, _ in capi.LsmGnnLaunchPlan._fields_]
    pol = header("lsm_policy.h")
    assert struct_fields(pol, "lsm_head_launch_plan") == [f for f, _ in capi.LsmHeadLaunchPlan._fields_]
    assert struct_fields(pol, "lsm_head_plan_job") == [f for f, _ in capi.LsmHeadPlanJob._fields_]
    assert "#define LSM_HEAD_PLAN_MAX_JOBS %d" % capi.LSM_HEAD_PLAN_MAX_JOBS in pol


def test_plan_refusals_carry_the_routines_own_text():
    bad = dataclasses.replace(pc.ACTOR, hidden=129)
    for which, prefix in (("forward", "head: "), ("evaluate", "evaluate: "), ("backward", "backward: ")):
        plan, err = lp.head_plan(bad, which)
        assert plan is None and err.startswith(prefix) and "hidden" in err
        assert lp.head_plan(pc.ACTOR, which, 65, 0)[1].startswith(prefix)
        assert lp.head_plan(pc.ACTOR, which, -1, 3)[1].startswith(prefix)
        assert lp.head_plan(pc.ACTOR, which, 2 ** 30, 3)[1].startswith(prefix)
        assert lp.head_plan(pc.ACTOR, which, 0, 3)[0] is not None                 # an empty minibatch is legal
    lib, p = lp._lib(), capi.LsmHeadLaunchPlan()
    import ctypes
    assert lib.lsm_head_plan(pc.ACTOR.struct(), 3, 65, 3, ctypes.byref(p)) != 0
    assert lib.lsm_head_plan(pc.ACTOR.struct(), 0, 65, 3, None) != 0
    assert lib.lsm_gnn_plan(gc.DEFAULT.struct(), 5, 24, 1, 0, None) != 0
    for over, E, N, masked in ((dict(H=5), 24, 1, 0), ({}, 0, 1, 0), ({}, 257, 1, 0), ({}, 24, 3, 1), ({}, 24, 0, 1)):
        plan, err = lp.gnn_plan(dataclasses.replace(gc.DEFAULT, **over), 5, E, N, bool(masked))
        assert plan is None and err.startswith("gnn: ") and len(err) > 5
    assert lp.gnn_plan(gc.DEFAULT, 0, 24)[0] is not None
    assert lp.gnn_plan(gc.DEFAULT, 10, 24, 5, True)[0] == lp.gnn_plan(gc.DEFAULT, 10, 24)[0]


# ---- the heads' boundaries ----------------------------------------------------------------------------------

# What the headers state: include/lsm_backward.h ("hidden 64 fits up to in = 240 with recurrent_N 1 and up to
# in = 172 with recurrent_N 2; hidden 128 with an RNN does not fit"), include/lsm_evaluate.h ("hidden 64 with
# recurrent_N 1 fits at every input width") and lsm_policy.h's limits (in <= 256, hidden <= 128), which are
# all the forward has. None: the header states no number; the walk's result is then only checked against the
# LDS itself.
STATED_IN = {("backward", 0): 256, ("backward", 1): 240, ("backward", 2): 172,
             ("evaluate", 0): 256, ("evaluate", 1): 256, ("evaluate", 2): 256,
             ("forward", 0): 256, ("forward", 1): 256, ("forward", 2): 256}
STATED_HIDDEN = {("backward", 0): 128, ("backward", 1): 88, ("backward", 2): 76,
                 ("evaluate", 0): 128, ("evaluate", 1): 128, ("evaluate", 2): 124,
                 ("forward", 0): 128, ("forward", 1): 128, ("forward", 2): 128}


def check_boundary(which, last, past):
    """`last` fits the LDS; `past` (one step further) is refused: with the LDS text, unless the step left the
    ABI's own limits."""
    plan, err = lp.head_plan(last, which)
    assert err is None and 0 < max(plan["lds_bytes"]) <= lp.LDS
    plan2, err2 = lp.head_plan(past, which)
    assert plan2 is None
    if past.in0 + past.in1 <= 256 and past.hidden <= 128:
        assert "bytes of LDS" in err2 and str(lp.LDS) in err2, err2
    else:
        assert "must be in" in err2, err2
    return plan


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("rn", [0, 1, 2])
@pytest.mark.parametrize("which", ROUTINES)
def test_largest_in_at_hidden_64(which, rn, kind):
    cfg = dataclasses.replace(KINDS[kind], recurrent_N=rn)
    assert cfg.hidden == 64
    width = lp.largest_in(cfg, which)
    plan = check_boundary(which, lp.with_in(cfg, width), lp.with_in(cfg, width + 1))
    print("%s %s recurrent_N %d: largest in %d, lds %s" % (which, kind, rn, width, plan["lds_bytes"]))
    assert width == STATED_IN[(which, rn)]
    if which == "backward" and rn > 0:
        assert plan["lds_bytes"][1] == lp.LDS           # the headers' "exactly the whole LDS"


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("rn", [0, 1, 2])
@pytest.mark.parametrize("which", ROUTINES)
def test_largest_hidden_at_in_22(which, rn, kind):
    cfg = lp.with_in(dataclasses.replace(KINDS[kind], recurrent_N=rn), 22)
    hidden = lp.largest_hidden(cfg, which)
    plan = check_boundary(which, dataclasses.replace(cfg, hidden=hidden), dataclasses.replace(cfg, hidden=hidden + 1))
    print("%s %s recurrent_N %d: largest hidden %d, lds %s" % (which, kind, rn, hidden, plan["lds_bytes"]))
    assert hidden == STATED_HIDDEN[(which, rn)]


def test_hidden_128():
    """The backward: hidden 128 with an RNN does not fit at any input width; without one in <= 248 does. The
    evaluate takes hidden 128 with recurrent_N 1 up to in = 240 and refuses it with recurrent_N 2 at every
    width (168960 bytes at in = 22), which the forward accepts."""
    for rn in (1, 2):
        for width in (1, 22, 256):
            cfg = lp.with_in(dataclasses.replace(pc.ACTOR, hidden=128, recurrent_N=rn), width)
            assert "bytes of LDS" in lp.head_plan(cfg, "backward")[1]
            assert lp.head_plan(cfg, "forward")[0] is not None
            if rn == 2:
                assert "bytes of LDS" in lp.head_plan(cfg, "evaluate")[1], width
    one = dataclasses.replace(pc.ACTOR, hidden=128, recurrent_N=1)
    assert lp.largest_in(one, "evaluate") == 240
    assert lp.head_plan(lp.with_in(one, 240), "evaluate")[0]["lds_bytes"][0] == lp.LDS
    assert "bytes of LDS" in lp.head_plan(lp.with_in(one, 241), "evaluate")[1]
    none = dataclasses.replace(pc.ACTOR, hidden=128, recurrent_N=0)
    assert lp.largest_in(none, "backward") == 248 and lp.largest_in(none, "evaluate") == 256
    assert lp.head_plan(lp.with_in(none, 248), "backward")[0]["lds_bytes"][1] <= lp.LDS
    assert "bytes of LDS" in lp.head_plan(lp.with_in(none, 249), "backward")[1]


def head_configs():
    """Every config the heads' cases run, with its sizes: the options, the plan cases, the shapes."""
    out = []
    for name in sorted(ec.OPTIONS):
        base, over = ec.OPTIONS[name]
        out.append(("option " + name, dataclasses.replace(base, **over), ec.OPTION_C, ec.OPTION_T))
    for name in ec.BACKWARD_PLAN_NAMES:
        out.append(("plan " + name, ec.plan_cfg(name, "backward"), ec.OPTION_C, ec.plan_T(name)))
    for Cn, T in ec.SHAPES:
        out += [("actor C%d T%d" % (Cn, T), pc.ACTOR, Cn, T), ("critic C%d T%d" % (Cn, T), pc.CRITIC, Cn, T)]
    return out


def test_the_heads_plans_are_what_the_headers_document():
    """Per tile row, in floats: lsm_evaluate.h's and lsm_backward.h's LDS formulas with the plan's own sizes,
    the stage-3 tiling of every job, and the workspace's arrays in the documented order."""
    for name, cfg, Cn, T in head_configs():
        n_in, Hd, RN = cfg.in0 + cfg.in1, cfg.hidden, cfg.recurrent_N
        A = cfg.num_actions if cfg.kind == "actor" else 1
        fwd, _ = lp.head_plan(cfg, "forward", Cn, T)
        assert (fwd["SX"], fwd["SA"]) == (pad(max(n_in, Hd)), pad(max(Hd, A))), name
        assert fwd["lds_bytes"][0] == 256 * (fwd["SX"] + 2 * fwd["SA"]), name
        ev, err = lp.head_plan(cfg, "evaluate", Cn, T)
        if ev is not None:
            assert (ev["SX"], ev["SA"], ev["SH"]) == (fwd["SX"], fwd["SA"], pad(Hd)), name
            assert ev["lds_bytes"][0] == 256 * (ev["SX"] + 2 * ev["SA"] + RN * ev["SH"]) <= lp.LDS, name
        bw, err = lp.head_plan(cfg, "backward", Cn, T)
        assert bw is not None, (name, err)
        G = 4 * ((Hd + 3) // 4 * 4) if RN else Hd
        assert (bw["SX"], bw["SA"], bw["SH"]) == (pad(max(n_in, Hd)), pad(Hd), pad(Hd)), name
        assert (bw["S0"], bw["S1"], bw["S2"]) == (pad(max(n_in, G)), pad(max(n_in, Hd, A)), pad(Hd)), name
        assert bw["lds_bytes"][0] == 256 * (bw["SX"] + 2 * bw["SA"] + RN * bw["SH"]) <= lp.LDS, name
        assert bw["lds_bytes"][1] == 256 * (bw["S0"] + bw["S1"] + bw["S2"] + RN * bw["SH"]) <= lp.LDS, name
        R = Cn * T
        assert bw["slabs"] == -(-R // capi.LSM_BWD_SLAB), name
        # stage 3: the jobs cover the blob, each tiled 64 x 64 over (nout, nin + 1), the tiles numbered in turn
        nw = int(lp._lib().lsm_head_weights_floats(cfg.struct()))
        covered = sum(j["nout"] * (j["nin"] + 1) for j in bw["jobs"]) + (0 if cfg.feature_norm else 2 * n_in)
        assert covered == nw, name
        tile = 0
        for j in bw["jobs"]:
            assert j["tile0"] == tile and j["ti_n"] == -(-(j["nin"] + 1) // 64), (name, j)
            tile += j["ti_n"] * -(-j["nout"] // 64)
        assert tile == bw["ntiles"] and len(bw["jobs"]) == bw["njobs"] <= capi.LSM_HEAD_PLAN_MAX_JOBS, name
        # the workspace (lsm_backward.h): stage 1's arrays, the features last; stage 2's; the slabs' partials
        stage1 = n_in + 2 * Hd * (cfg.layer_N + 1) + 6 * Hd * RN
        assert bw["o_feat"] == R * stage1, name
        for k in range(RN):
            assert bw["o_ho"][k] == R * (n_in + 2 * Hd * (cfg.layer_N + 1) + 6 * Hd * k + 5 * Hd), name
        stage2 = A + (2 * Hd + 6 * Hd * RN if RN else 0) + 3 * Hd * (cfg.layer_N + 1) + (2 * n_in if cfg.feature_norm else 0)
        assert bw["ws_floats"] == R * (stage1 + Hd + stage2) + bw["slabs"] * nw, name
        want = max((bw["ws_floats"] * 4 + 7) // 8 * 8, 8)
        assert int(lp._lib().lsm_head_backward_workspace_bytes(cfg.struct(), Cn, T)) == want, name


# ---- the encoder's boundaries -------------------------------------------------------------------------------

def test_the_wide_encoder_fits_up_to_the_headers_E():
    """include/lsm_gnn.h: "reference defaults: every E <= 256 fits; H * C = 256 fits up to E = 39"."""
    wide = gc.plan_cfg("wide corner max E")
    assert (wide.H, wide.C, wide.concat, wide.embed_hidden, wide.F, wide.embed_layer_N, wide.layer_N) == (
        4, 64, True, 64, 64, 4, 4)
    last = lp.largest_E(wide)
    plan, _ = lp.gnn_plan(wide, 2, last)
    print("wide encoder: largest E %d, plan %s" % (last, plan))
    assert last == 39 and plan["lds_bytes"] <= lp.LDS
    assert "exceed the LDS" in lp.gnn_plan(wide, 2, last + 1)[1]
    assert lp.largest_E(gc.DEFAULT) == 256
    # H * C = 256 without concat: narrower activation rows, and E = 65 still does not fit
    flat = gc.plan_cfg("H4 C64 max E")
    assert not flat.concat and 39 < lp.largest_E(flat) < 65
    assert "exceed the LDS" in lp.gnn_plan(flat, 5, 65)[1]


def gnn_configs():
    out = [("shape E%d" % E, gc.DEFAULT, 5, E) for E in gc.SHAPE_E]
    out += [("option " + n, dataclasses.replace(gc.DEFAULT, **gc.OPTIONS[n]), 5, 24) for n in sorted(gc.OPTIONS)]
    out += [("plan " + n, gc.plan_cfg(n), gc.plan_B(n), gc.plan_E(n)) for n in sorted(gc.PLAN_CASES)]
    return out


def gnn_rows(cfg, E, plan):
    """include/lsm_gnn.h's LDS need of one graph without its adjacency, in floats, with the plan's strides."""
    return E * (2 * plan["SA"] + 2 * plan["SK"] + 1)


def test_the_encoders_plans_are_what_the_header_documents():
    """The strides hold their rows; a team is the power of two >= E (at least 32); a workgroup packs
    256 / TS graphs unless their LDS does not fit; the adjacency is staged in LDS exactly when E * E more
    floats fit beside the graph's rows (up to the 16-byte rounding of the two parts)."""
    configs = gnn_configs()
    for cfg in {c for _, c, _, _ in configs}:
        configs += [("every E", cfg, 5, E) for E in range(1, lp.largest_E(cfg) + 1)]
    for name, cfg, B, E in configs:
        plan, err = lp.gnn_plan(cfg, B, E)
        assert plan is not None, (name, E, err)
        HC = cfg.H * cfg.C
        assert plan["SA"] == pad(max(cfg.embed_hidden, cfg.out_dim)) and plan["SK"] == pad(max(cfg.embed_hidden, HC))
        assert plan["fast"] == int(cfg.embed_hidden == 16 and cfg.C == 16), name
        TS, G = plan["TS"], plan["G"]
        assert TS in (32, 64, 128, 256) and TS >= E and (TS == 32 or TS // 2 < E), (name, E)
        assert 1 <= G <= 256 // TS and plan["lds_bytes"] <= lp.LDS and plan["lds_bytes"] % (16 * G) == 0, (name, E)
        per_graph = plan["lds_bytes"] // G
        rows = 4 * gnn_rows(cfg, E, plan)
        slack = 2 * 12                                   # each part is rounded up to 16 bytes
        if plan["adj_lds"]:
            assert rows + 4 * E * E <= per_graph <= rows + 4 * E * E + slack, (name, E)
        else:
            assert rows <= per_graph <= rows + slack and rows + 4 * E * E + slack > lp.LDS, (name, E)
        if G < 256 // TS:                                # cut by the LDS: one more graph would not fit
            assert (G + 1) * per_graph > lp.LDS, (name, E)


# ---- the coverage assertion ---------------------------------------------------------------------------------

def test_the_encoders_cases_cover_every_plan():
    plans = {name: lp.gnn_plan(cfg, B, E)[0] for name, cfg, B, E in gnn_configs()}
    assert all(plans.values())
    have = lambda pred: sorted(n for n, p in plans.items() if pred(p))
    required = {
        "the <16, 16> instance with the adjacency in LDS": lambda p: p["fast"] and p["adj_lds"],
        "the <16, 16> instance with the adjacency read from memory": lambda p: p["fast"] and not p["adj_lds"],
        "the generic instance with the adjacency in LDS": lambda p: not p["fast"] and p["adj_lds"],
        "the generic instance with the adjacency read from memory": lambda p: not p["fast"] and not p["adj_lds"],
        "the generic instance with TS 256": lambda p: not p["fast"] and p["TS"] == 256,
        "the generic instance with G cut by the LDS": lambda p: not p["fast"] and p["G"] < 256 // p["TS"],
        "G cut by the LDS": lambda p: p["G"] < 256 // p["TS"],
        "G cut by the LDS to 1 below TS 256": lambda p: p["G"] == 1 and p["TS"] < 256,
        "G not cut": lambda p: p["G"] == 256 // p["TS"] and p["G"] > 1,
        "G not a power of two": lambda p: p["G"] & (p["G"] - 1),
        "TS 32": lambda p: p["TS"] == 32,
        "TS 64": lambda p: p["TS"] == 64,
        "TS 128": lambda p: p["TS"] == 128,
        "TS 256": lambda p: p["TS"] == 256,
        "a workgroup's LDS within 1 % of the limit": lambda p: p["lds_bytes"] > 0.99 * lp.LDS,
    }
    missing = [what for what, pred in required.items() if not have(pred)]
    assert not missing, "no encoder case runs: " + "; ".join(missing)
    # both sides of each instance's adj_lds switch are adjacent sizes
    for inst in ("default", "generic"):
        a, b = gc.plan_E(inst + " adj_lds last"), gc.plan_E(inst + " adj_lds first")
        assert b == a + 1 and plans["plan %s adj_lds last" % inst]["adj_lds"] == 1
        assert plans["plan %s adj_lds first" % inst]["adj_lds"] == 0
    # the sizes the issue names stay in: BASELINE config 4's graph, the N = 33 env's, the exact team size
    sizes = {gc.plan_E(n) for n in gc.PLAN_CASES if not gc.PLAN_CASES[n][0]}
    assert {33, 48, 64, 99, 128, 256} <= sizes


def test_the_backwards_cases_cover_every_plan():
    plans = {}
    for name, cfg, Cn, T in head_configs():
        plan, err = lp.head_plan(cfg, "backward", Cn, T)
        assert plan is not None, (name, err)
        A = cfg.num_actions if cfg.kind == "actor" else 1
        plans[name] = dict(plan, A=A, n_in=cfg.in0 + cfg.in1, Hd=cfg.hidden, cfg=cfg)
    jobs = lambda p: p["jobs"]
    required = {
        "a job whose second tile along i holds weight columns (nin >= 65)":
            lambda p: any(j["ti_n"] >= 2 and j["nin"] > 64 for j in jobs(p)),
        "a job with three tiles along i": lambda p: any(j["ti_n"] == 3 for j in jobs(p)),
        "a job with three tiles along i whose third holds weight columns (nin >= 129)":
            lambda p: any(j["ti_n"] == 3 and j["nin"] > 128 for j in jobs(p)),
        "the bias column last in a tile (nin = 63 mod 64)": lambda p: any(j["nin"] % 64 == 63 for j in jobs(p)),
        "the bias column last in the second tile (nin = 127)": lambda p: any(j["nin"] == 127 for j in jobs(p)),
        "the bias column alone in the next tile (nin = 64)": lambda p: any(j["nin"] == 64 for j in jobs(p)),
        "the bias column alone in the third tile (nin = 128)": lambda p: any(j["nin"] == 128 for j in jobs(p)),
        "more than three tiles along j (a GRU job's 3 * hidden above 192)":
            lambda p: any(j["nout"] > 192 and j["nin"] > 0 for j in jobs(p)),
        "more than three tiles along j and two along i": lambda p: any(j["nout"] > 192 and j["ti_n"] >= 2 for j in jobs(p)),
        "A > max(in, hidden): the A branch of S1": lambda p: p["A"] > max(p["n_in"], p["Hd"]),
        "in > max(hidden, A): the in branch of S1": lambda p: p["n_in"] > max(p["A"], p["Hd"]),
        "a sweep tile of exactly 163840 bytes": lambda p: p["lds_bytes"][1] == lp.LDS,
        "a sweep tile of exactly 163840 bytes with recurrent_N 2":
            lambda p: p["lds_bytes"][1] == lp.LDS and p["cfg"].recurrent_N == 2,
        "hidden 128 at its widest input (a sweep tile within 2048 bytes of the limit)":
            lambda p: p["cfg"].hidden == 128 and p["lds_bytes"][1] > lp.LDS - 2048,
        "layer_N 3": lambda p: p["cfg"].layer_N == 3,
        "layer_N 4 (the most jobs)": lambda p: p["cfg"].layer_N == 4,
        "in0 + in1 = 1": lambda p: p["n_in"] == 1,
        "in0 + in1 = 1 with x1 null": lambda p: p["n_in"] == 1 and p["cfg"].in1 == 0,
        "hidden not a multiple of 4 above 64 (HP > hidden)": lambda p: p["HP"] > p["Hd"] > 64,
        "more than one slab": lambda p: p["slabs"] > 1,
    }
    # the slab cases are the backward's own (heads_backward_cases.slab_case)
    slab = dataclasses.replace(pc.ACTOR, num_actions=5, **hc.SMALL)
    p = lp.head_plan(slab, "backward", (3 * hc.SLAB + 2) // 2, 2)[0]
    plans["slab"] = dict(p, A=5, n_in=7, Hd=8, cfg=slab)
    missing = [what for what, pred in required.items() if not any(pred(p) for p in plans.values())]
    assert not missing, "no backward case runs: " + "; ".join(missing)
    # the bit-equality cases sit at nin = 64, 65 and 128
    for name, nin in zip(hc.TWICE_PLAN, (64, 65, 128)):
        assert any(j["nin"] == nin and j["nout"] > 1 for j in hc.plan_of(name)["jobs"]), (name, nin)


def test_the_evaluates_cases_reach_its_limits():
    """The evaluate's plan has no branches beyond its strides; its cases reach a tile of exactly 163840 bytes
    (hidden 124, recurrent_N 2), hidden 128, in 256 and in0 + in1 = 1."""
    plans = [(ec.plan_cfg(n), lp.head_plan(ec.plan_cfg(n), "evaluate", ec.OPTION_C, ec.plan_T(n))[0])
             for n in sorted(ec.PLAN_OPTIONS)]
    assert all(p for _, p in plans)
    assert any(p["lds_bytes"][0] == lp.LDS for _, p in plans)
    assert any(c.hidden == 128 and c.recurrent_N == 1 and p["lds_bytes"][0] == lp.LDS for c, p in plans)
    assert any(c.in0 + c.in1 == 256 and c.recurrent_N == 2 for c, _ in plans)
    assert any(c.in0 + c.in1 == 1 and c.kind == "actor" and not c.feature_norm for c, _ in plans)
    assert any(c.kind == "actor" and c.num_actions > max(c.hidden, c.in0 + c.in1) for c, _ in plans)
    fwd = [dataclasses.replace(b, **o) for b, o in pc.PLAN_OPTIONS.values()]
    big = max(lp.head_plan(c, "forward", pc.OPTION_M, 1)[0]["lds_bytes"][0] for c in fwd)
    assert big == 64 * 4 * (pad(256) + 2 * pad(128)) and any(c.in0 + c.in1 == 1 for c in fwd)
