"""CPU tests of the device optimiser's C ABI (include/lsm_optim.h): the header and its exports, and
lsm_host_optim_step -- the text the kernels run, in the kernels' order -- on tests/optim_cases.py's cases: bit-equal
to tests/optim_model.py's numpy float32 model on weights, exp_avg, exp_avg_sq, state and info; the norm within one
float32 ulp of the float64 truth; weights and moments within the project's criterion of torch.optim.Adam +
clip_grad_norm_; and every argument refusal through both entry points (a refusal comes before any launch or write,
so it needs no device)."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import optim_cases as oc
import optim_model as om
from lsm import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lsm_optim.h")


@pytest.fixture(scope="module")
def lib():
    from lsm import build
    build.build(verbose=False)
    return capi.load_library()


@pytest.fixture(scope="module")
def runner(lib):
    return functools.partial(oc.run, lib)


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
    assert declared == set(capi.EXPORTED_OPTIM) and len(declared) == 4
    for name in declared:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    for other in (capi.EXPORTED, capi.EXPORTED_LEARNER, capi.EXPORTED_RECURRENT, capi.EXPORTED_MB_EDGES,
                  capi.EXPORTED_GNN, capi.EXPORTED_POLICY, capi.EXPORTED_EVALUATE, capi.EXPORTED_LOSS,
                  capi.EXPORTED_BACKWARD, capi.EXPORTED_GNN_BACKWARD, capi.EXPORTED_GNN_EMBED_BACKWARD):
        assert not declared & set(other)
    fields = lambda body: [n for n in re.findall(r"(\w+)(?:\[\w+\])?;", body)]
    body = hdr[hdr.index("typedef struct lsm_optim_segment"):hdr.index("} lsm_optim_segment")]
    assert fields(body) == [f for f, _ in capi.LsmOptimSegment._fields_]
    body = hdr[hdr.index("typedef struct lsm_optim_group"):hdr.index("} lsm_optim_group")]
    assert fields(body) == [f for f, _ in capi.LsmOptimGroup._fields_]
    for name in ("LSM_OPT_MAX_GROUPS", "LSM_OPT_MAX_SEGMENTS", "LSM_OPT_CHUNK", "LSM_OPT_LANES"):
        assert int(re.search(r"#define %s (\d+)" % name, hdr).group(1)) == getattr(capi, name), name
    assert (om.CHUNK, om.LANES) == (capi.LSM_OPT_CHUNK, capi.LSM_OPT_LANES)


def test_the_unit_is_built_apart_and_has_no_atomics(lib):
    from lsm import build
    deps = [os.path.basename(p) for p in build._rollout_deps()]
    assert not {"lsm_optim.hip", "lsm_optim.h"} & set(deps)
    assert lib.lsm_build_id().decode() == build.build_id()
    assert "../../include/lsm_optim.h" in build.UNITS["lsm_optim.hip"]
    src = open(os.path.join(build.CSRC, "lsm_optim.hip")).read()
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "fma" not in code and "hipMalloc" not in code and "Synchronize" not in code
    assert code.count("<<<") == 3, "three launches, whatever n_groups is"


def test_workspace_bytes(lib):
    tab = (capi.LsmOptimGroup * 2)()
    tab[0].n_segments, tab[1].n_segments = 2, 1
    tab[0].segments[0].n, tab[0].segments[1].n, tab[1].segments[0].n = oc.CHUNK + 1, 0, oc.CHUNK
    f = lib.lsm_optim_workspace_bytes
    assert f(tab, 2) == 8 * (16 + 3) and f(tab, 1) == 8 * (16 + 2) and f(tab, 0) == f(None, 0) == 8 * 16
    assert f(None, 1) == 0 and f(tab, 5) == 0 and f(tab, -1) == 0
    tab[1].segments[0].n = -1
    assert f(tab, 2) == 0 and lib.lsm_optim_last_error().decode() == "optim: a segment has n < 0"


# ---- the cases --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", oc.SIZES)
def test_segment_sizes(runner, n):
    oc.check_size(runner, n)


def test_three_segments_at_odd_offsets(runner):
    oc.check_odd_offsets(runner)


def test_two_groups_in_one_call(runner):
    oc.check_two_groups(runner)


def test_clipping(runner):
    oc.check_clipping(runner)


def test_weight_decay(runner):
    oc.check_weight_decay(runner)


def test_six_steps_with_a_changed_lr(runner):
    oc.check_six_steps(runner)


def test_small_magnitudes(runner):
    oc.check_small_magnitudes(runner)


def test_the_criterion_rejects_a_misplaced_eps():
    """The yardstick itself: at the small magnitudes, (sqrt(v) + eps) / s2 in place of sqrt(v) / s2 + eps is
    outside the criterion after one step (at weights of order 1 it would not be noticed)."""
    segs = oc.data([37], 31, 1e-3, 1e-5)
    t64, _ = om.truth64(oc.H, [tuple(a.astype(np.float64) for a in s) for s in segs], 0)
    ref, _ = om.Torch32(oc.H, [segs[0][0]]).step([segs[0][1]])
    (w, _, m, v), = om.model32(oc.H, segs, om.fresh_state())[0]
    s2, step_size = np.float32(np.sqrt(1.0 - 0.999)), np.float32(7e-4 / (1.0 - 0.9))
    wrong = segs[0][0] - step_size * (m / ((np.sqrt(v) + np.float32(1e-5)) / s2))
    om.within(w, t64[0][0], ref[0][0], "the formula")
    with pytest.raises(AssertionError):
        om.within(wrong, t64[0][0], ref[0][0], "a misplaced eps")


@pytest.mark.parametrize("value", [float("nan"), float("inf")])
def test_nonfinite_gradient(runner, value):
    oc.check_nonfinite(runner, value)


def test_gradient_of_1e20(runner):
    oc.check_huge_gradient(runner)


def test_the_same_call_twice(runner):
    oc.check_twice(runner)


def test_refusals(lib):
    oc.check_refusals(lib)
