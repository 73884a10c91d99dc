"""CPU tests of the train_info accumulator's C ABI (include/lsm_train_info.h): the header and its exports, and
lsm_host_train_info_add / _mean -- the text the kernels run -- on tests/train_info_model.py's cases: bit-equal to the
header restated in numpy float64 on sum, n, updates, first_nonfinite and out, with the state and out between
canaries; and every argument refusal through both pairs of entry points (a refusal comes before any launch or
write, so it needs no device)."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import train_info_model as tm
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_train_info.h")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.fixture(scope="module")
def runner(lib):
    return functools.partial(tm.run, lib)


# ---- the ABI ----------------------------------------------------------------------------------------------------

def test_header_is_plain_c_abi():
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++11", "c++")):
        if shutil.which(cc) is None:
            pytest.skip("%s not available" % cc)
        subprocess.check_call([cc, std, "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", lang, HDR])


def test_exports_every_declared_symbol(lib):
    text = open(HDR).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"^\s*(?:[\w\*]+\s+)+\**(lsm_\w+)\s*\(", hdr, re.M))
    assert declared == set(capi.EXPORTED_TRAIN_INFO) and len(declared) == 5
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE, capi.EXPORTED_LOSS,
                  capi.EXPORTED_BACKWARD, capi.EXPORTED_GNN_BACKWARD, capi.EXPORTED_GNN_EMBED_BACKWARD,
                  capi.EXPORTED_OPTIM):
        assert not declared & set(other)
    body = hdr[hdr.index("typedef struct lsm_train_info_src"):hdr.index("} lsm_train_info_src")]
    assert re.findall(r"(\w+)(?:\[\w+\])?;", body) == [f for f, _ in capi.LsmTrainInfoSrc._fields_]
    assert C.sizeof(capi.LsmTrainInfoSrc) == 8 * capi.LSM_TRAIN_INFO_SLOTS
    for name in ("LSM_TRAIN_INFO_SLOTS", "LSM_TRAIN_INFO_MEANS", "LSM_TRAIN_INFO_STATE_WORDS",
                 "LSM_TRAIN_INFO_LANES"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(capi, name), name
    assert capi.LSM_TRAIN_INFO_STATE_WORDS == 2 * capi.LSM_TRAIN_INFO_SLOTS + 2
    assert len(capi.TRAIN_INFO_SLOTS) == capi.LSM_TRAIN_INFO_SLOTS
    # the reference's six keys in its own order (graph_mappo.py:273-278), then the two counts
    assert capi.TRAIN_INFO_SLOTS == ("value_loss", "policy_loss", "dist_entropy", "actor_grad_norm",
                                     "critic_grad_norm", "ratio", "actor_skipped", "critic_skipped")
    for k, name in enumerate(capi.TRAIN_INFO_SLOTS):
        assert re.search(r"\b%d %s\b" % (k, name), text), "the header names slot %d %s" % (k, name)
    flat = " ".join(text.replace("\n *", " ").split())
    assert "it is not the state's `updates`" in flat and "even when a generator yielded fewer minibatches" in flat


def test_the_unit_is_built_apart_in_plain_cpp(lib):
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_train_info.hip", "lsm_train_info.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    assert "../../include/lsm_train_info.h" in build.UNITS["lsm_train_info.hip"]
    assert "lsm_train_info" not in open(os.path.join(ROOT, "include", "lsm_rollout.h")).read()
    src = open(os.path.join(build.CSRC, "lsm_train_info.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "asm" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert code.count("<<<") == 2, "one launch per entry point"
    assert code.count("<<<dim3(1), dim3(LANES)") == 2, "each of a single small workgroup"


# ---- the cases --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(tm.CASES))
def test_host_entry_points_equal_the_model(runner, name):
    tm.check_case(runner, name)


def test_null_slots_count_per_slot(runner):
    seq, num, _ = tm.CASES["actor_every_other_update"]
    got = runner(seq, num)
    assert [int(got["n"][k]) for k in tm.CRITIC] == [4, 4, 4] and [int(got["n"][k]) for k in tm.ACTOR] == [2] * 5
    got = runner(*tm.CASES["critic_only"][:2])
    assert all(got["n"][k] == 0 and got["sum"][k] == 0 and got["out"][k] == 0 for k in tm.ACTOR)
    assert all(got["n"][k] == 3 for k in tm.CRITIC) and got["updates"] == 3 and got["first_nonfinite"] == -1


def test_float64_keeps_what_a_float32_accumulator_loses(runner):
    """1e20, -1e20, 1 sums to 1 in any accumulator (1e20 - 1e20 is exactly 0 before the 1 arrives), so that
    sequence is held to the model and to 1 / 3 only; 1e10, 1, -1e10 is the one a float32 accumulator gets wrong."""
    third = np.float32(1.0 / 3.0)
    seq, num, _ = tm.CASES["cancellation"]
    got = runner(seq, num)
    assert all(got["out"][k] == third and got["sum"][k] == 1.0 for k in range(tm.MEANS))
    seq, num, _ = tm.CASES["absorption"]
    got, m32 = runner(seq, num), tm.model(seq, num, acc=np.float32)
    assert all(got["out"][k] == third and got["sum"][k] == 1.0 for k in range(tm.MEANS))
    assert all(m32["out"][k] == 0 for k in range(tm.MEANS)), "the float32 model must differ, or the case shows nothing"
    assert got["first_nonfinite"] == -1


def test_nonfinite_values_are_added_and_remembered(runner):
    seq, num, _ = tm.CASES["nonfinite"]
    got, want = runner(seq, num), tm.model(seq, num)
    assert got["first_nonfinite"] == 2 and got["updates"] == 5
    assert np.isnan(got["sum"][1]) and np.isnan(got["out"][1]) and np.isposinf(got["sum"][4]) and np.isposinf(got["out"][4])
    rest = [k for k in range(tm.SLOTS) if k not in (1, 4)]
    np.testing.assert_array_equal(tm.bits(got["sum"][rest]), tm.bits(want["sum"][rest]))
    np.testing.assert_array_equal(tm.bits(got["out"][rest]), tm.bits(want["out"][rest]))
    assert np.isfinite(got["out"][rest]).all() and (got["n"] == 5).all()


def test_the_divisor_is_the_callers(runner):
    seq = tm.CASES["more_updates_than_adds"][0]
    three, four = runner(seq, 3), runner(seq, 4)
    np.testing.assert_array_equal(tm.bits(three["sum"]), tm.bits(four["sum"]))
    assert three["updates"] == four["updates"] == 3
    for k in range(tm.MEANS):
        assert four["out"][k] == np.float32(four["sum"][k] / 4.0) and three["out"][k] == np.float32(three["sum"][k] / 3.0)
    for k in range(tm.MEANS, tm.SLOTS):
        assert four["out"][k] == three["out"][k] == np.float32(four["sum"][k]), "a count is not divided"


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_refusals(lib):
    state = np.full(tm.WORDS + 2, tm.CANARY64, np.int64)
    out = np.full(tm.SLOTS + 2, tm.CANARY32, np.float32)
    vals = np.full(tm.SLOTS + 2, tm.CANARY32, np.float32)
    sp, op, vp = state.ctypes.data + 8, out.ctypes.data + 4, vals.ctypes.data + 4
    good = [vp + 4 * k for k in range(tm.SLOTS)]
    err = lambda: lib.lsm_train_info_last_error().decode()

    def adds(state_ptr, ptrs, text):
        for call in (lambda: lib.lsm_train_info_add(state_ptr, tm._src(ptrs), 1, None),
                     lambda: lib.lsm_host_train_info_add(state_ptr, tm._src(ptrs), 1)):
            assert call() != 0 and err() == "train info: " + text, err()

    def means(state_ptr, num, out_ptr, text):
        for call in (lambda: lib.lsm_train_info_mean(state_ptr, num, out_ptr, None),
                     lambda: lib.lsm_host_train_info_mean(state_ptr, num, out_ptr)):
            assert call() != 0 and err() == "train info: " + text, err()

    adds(None, good, "state is null")
    adds(C.c_void_p(sp + 4), good, "state must be 8-byte aligned")
    for k in (0, 7):
        adds(C.c_void_p(sp), good[:k] + [good[k] + 2] + good[k + 1:], "a src pointer is not 4-byte aligned")
        for inside in (sp, sp + 8 * tm.WORDS - 4):    # the state's first and last four bytes
            adds(C.c_void_p(sp), good[:k] + [inside] + good[k + 1:], "a src pointer overlaps the state")
    means(None, 1, C.c_void_p(op), "state is null")
    means(C.c_void_p(sp + 4), 1, C.c_void_p(op), "state must be 8-byte aligned")
    means(C.c_void_p(sp), 1, None, "out is null")
    for num in (0, -3):
        means(C.c_void_p(sp), num, C.c_void_p(op), "num_updates must be >= 1")
    means(C.c_void_p(sp), 1, C.c_void_p(op + 2), "out is not 4-byte aligned")
    for o in (sp - 4 * (tm.SLOTS - 1), sp, sp + 8 * tm.WORDS - 4):    # out's last float, all of it, its first float
        means(C.c_void_p(sp), 1, C.c_void_p(o), "out overlaps the state")
    # nothing was written by any of them
    assert (state == tm.CANARY64).all() and (out == tm.CANARY32).all() and (vals == tm.CANARY32).all()
    # and the neighbours are legal: a value right before and right after the state, out right after it
    arena = np.zeros(1 + tm.WORDS + tm.SLOTS, np.int64)
    sp = arena.ctypes.data + 8
    edge = [sp - 4, sp + 8 * tm.WORDS] + good[2:]
    assert lib.lsm_host_train_info_add(C.c_void_p(sp), tm._src(edge), 1) == 0, err()
    assert lib.lsm_host_train_info_mean(C.c_void_p(sp), 1, C.c_void_p(sp + 8 * tm.WORDS)) == 0, err()
    assert arena[2 * tm.SLOTS + 1] == 1 and arena[0] == 0, "one update, and the word before the state untouched"
