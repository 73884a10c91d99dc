"""The cases of include/lsm_optim.h, shared by tests/test_optim_capi.py (lsm_host_optim_step on host memory) and
tests/test_gpu_optim.py (lsm_optim_step on the device): `run` lays a call's groups out in one allocation per array
kind, with canaries between and around the segments, calls the library and returns what it left; the check_*
functions compare that with tests/optim_model.py. A runner is run with the library and the device bound."""
import ctypes as C
import dataclasses

import numpy as np

import optim_model as om
from lsm import capi

CHUNK = capi.LSM_OPT_CHUNK
SIZES = (1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5)
ODD = (CHUNK + 1, 3, 2 * CHUNK + 5)    # the three segments at odd float offsets of one allocation
CANARY = np.float32(-7.25)
H = om.Hyper()
bits = lambda a: np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


def data(sizes, seed, wscale=1.0, gscale=1.0):
    """[(w, g, m, v)] float32 with fresh moments."""
    rng = np.random.default_rng(seed)
    return [((wscale * rng.standard_normal(n)).astype(np.float32), (gscale * rng.standard_normal(n)).astype(np.float32),
             np.zeros(n, np.float32), np.zeros(n, np.float32)) for n in sizes]


def grads(sizes, seed, gscale=1.0):
    rng = np.random.default_rng(seed)
    return [(gscale * rng.standard_normal(n)).astype(np.float32) for n in sizes]


def group(h=H, segs=(), state=None, offsets=None, goff=0):
    """One group of a call. offsets: each segment's float offset in the arenas (default: odd offsets, two or
    three canaries apart); goff: the grads arena's segments sit goff floats further (another alignment class)."""
    if offsets is None:
        offsets, o = [], 1
        for s in segs:
            offsets.append(o)
            o += s[0].size + 2
            o += 1 - o % 2
    return dict(h=h, segs=list(segs), state=om.fresh_state() if state is None else state.copy(), offsets=offsets,
                goff=goff)


def table(groups, bases, state_ptrs, info_ptrs):
    """The ctypes table: bases[gi] = the byte addresses of the (w, g, m, v) arenas."""
    tab = (capi.LsmOptimGroup * max(len(groups), 1))()
    for gi, G in enumerate(groups):
        h, t = G["h"], tab[gi]
        t.n_segments = len(G["segs"])
        t.use_max_grad_norm, t.skip_nonfinite = int(h.use_max_grad_norm), int(h.skip_nonfinite)
        t.lr, t.beta1, t.beta2, t.eps = h.lr, h.beta1, h.beta2, h.eps
        t.weight_decay, t.max_grad_norm = h.weight_decay, h.max_grad_norm
        t.state, t.info = state_ptrs[gi], info_ptrs[gi]
        for si, (seg, off) in enumerate(zip(G["segs"], G["offsets"])):
            s = t.segments[si]
            s.n = seg[0].size
            s.weights, s.exp_avg, s.exp_avg_sq = (bases[gi][k] + 4 * off for k in (0, 2, 3))
            s.grads = bases[gi][1] + 4 * (off + G["goff"])
    return tab


def run(lib, groups, dev=None, stream=None):
    """One call. Returns [dict(segs=[(w, g, m, v)], state, info)] per group, after checking the return code and
    every canary (the gaps of the arenas, the ends of the workspace, state's and info's neighbours)."""
    torch = None
    if dev is not None:
        import torch
    arenas = []
    for G in groups:
        size = max([o + s[0].size for s, o in zip(G["segs"], G["offsets"])] + [0]) + G["goff"] + 5
        four = [np.full(size, CANARY, np.float32) for _ in range(4)]
        for seg, off in zip(G["segs"], G["offsets"]):
            for k in range(4):
                o = off + (G["goff"] if k == 1 else 0)
                four[k][o:o + seg[k].size] = seg[k]
        arenas.append(four)
    states = np.full((len(groups), 6), 123.0, np.float64)    # [1:5] is the state
    infos = np.full((len(groups), 6), CANARY, np.float32)
    for gi, G in enumerate(groups):
        states[gi, 1:5] = G["state"]
    before = [[a.copy() for a in four] for four in arenas]
    if dev is None:
        held = (arenas, states, infos)
        addr = lambda a: a.ctypes.data
    else:
        up = lambda a: torch.from_numpy(a).to(dev)
        held = ([[up(a) for a in four] for four in arenas], up(states), up(infos))
        addr = lambda t: t.data_ptr()
    bases = [[addr(a) for a in four] for four in held[0]]
    tab = table(groups, bases, [addr(held[1]) + 8 * (6 * gi + 1) for gi in range(len(groups))],
                [addr(held[2]) + 4 * (6 * gi + 1) for gi in range(len(groups))])
    need = int(lib.lsm_optim_workspace_bytes(tab, len(groups)))
    chunks = sum((s[0].size + CHUNK - 1) // CHUNK for G in groups for s in G["segs"])
    assert need == 8 * (4 * capi.LSM_OPT_MAX_GROUPS + chunks), lib.lsm_optim_last_error()
    ws = np.full(need // 8 + 2, 321.0, np.float64)
    if dev is None:
        rc = lib.lsm_host_optim_step(tab, len(groups), C.c_void_p(ws.ctypes.data + 8))
    else:
        wst = up(ws)
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.device(dev):
            sh = torch.cuda.current_stream(dev).cuda_stream
            rc = lib.lsm_optim_step(tab, len(groups), C.c_void_p(wst.data_ptr() + 8), C.c_void_p(sh))
        torch.cuda.synchronize(dev)
        ws = wst.cpu().numpy()
        arenas = [[t.cpu().numpy() for t in four] for four in held[0]]
        states, infos = held[1].cpu().numpy(), held[2].cpu().numpy()
    assert rc == 0, lib.lsm_optim_last_error().decode()
    assert ws[0] == 321.0 and ws[-1] == 321.0, "the workspace's neighbours were written"
    assert (states[:, [0, 5]] == 123.0).all() and (infos[:, [0, 5]] == CANARY).all()
    out = []
    for gi, G in enumerate(groups):
        mask = [np.ones(a.size, bool) for a in arenas[gi]]
        segs = []
        for seg, off in zip(G["segs"], G["offsets"]):
            got = []
            for k in range(4):
                o = off + (G["goff"] if k == 1 else 0)
                got.append(arenas[gi][k][o:o + seg[k].size].copy())
                mask[k][o:o + seg[k].size] = False
            segs.append(tuple(got))
            np.testing.assert_array_equal(bits(got[1]), bits(seg[1]), "grads were written")
        for k in range(4):
            np.testing.assert_array_equal(bits(arenas[gi][k][mask[k]]), bits(before[gi][k][mask[k]]),
                                          "a float outside the segments was written")
        out.append(dict(segs=segs, state=states[gi, 1:5].copy(), info=infos[gi, 1:5].copy()))
    return out


def value_bits(a):
    """a's bits with every NaN mapped to one pattern, for the one case whose results are NaNs (a non-finite
    gradient without skip_nonfinite): where a NaN stands is the contract, its sign and payload are not -- they
    depend on how each side propagates a NaN operand and which default NaN it generates."""
    b = bits(a).copy()
    b[np.isnan(a)] = bits(np.array([np.nan], a.dtype))[0]
    return b


def same(got, want, what, of=bits):
    """got: one group's dict from run; want: model32's (segs, state, info). Bit for bit (of=value_bits: with all
    NaNs as one value)."""
    segs, state, info = want
    for si, (a, b) in enumerate(zip(got["segs"], segs)):
        for k, name in enumerate(("weights", "grads", "exp_avg", "exp_avg_sq")):
            np.testing.assert_array_equal(of(a[k]), of(b[k]), "%s: segment %d %s" % (what, si, name))
    np.testing.assert_array_equal(of(got["state"]), of(state), what + ": state")
    np.testing.assert_array_equal(of(got["info"]), of(info), what + ": info")


def same_groups(a, b, what):
    same(a, (b["segs"], b["state"], b["info"]), what)


def next_group(G, got, new_grads=None, h=None):
    """The group of the following call: what the call left, with new gradients."""
    segs = [(w, g if new_grads is None else new_grads[i], m, v) for i, (w, g, m, v) in enumerate(got["segs"])]
    return dict(G, segs=segs, state=got["state"].copy(), h=G["h"] if h is None else h)


def two_steps(runner, G, what):
    """G through two calls (the second with moments that are not 0), each against model32."""
    sizes = [s[0].size for s in G["segs"]]
    got = runner([G])[0]
    want = om.model32(G["h"], G["segs"], G["state"])
    same(got, want, what + ", step 1")
    assert want[1][0] == 1.0 and want[2][2] == 0.0
    G2 = next_group(G, got, grads(sizes, 99))
    same(runner([G2])[0], om.model32(G2["h"], G2["segs"], G2["state"]), what + ", step 2")


def check_size(runner, n):
    two_steps(runner, group(segs=data([n], n)), "n = %d" % n)
    two_steps(runner, group(segs=data([n], n), offsets=[0]), "n = %d, aligned" % n)


def check_odd_offsets(runner):
    segs = data(ODD, 7)
    G = group(segs=segs)
    assert all(o % 2 == 1 for o in G["offsets"]) and len({o % 4 for o in G["offsets"]}) > 1
    two_steps(runner, G, "three segments at odd offsets")
    two_steps(runner, group(segs=segs, goff=2), "grads in another alignment class")
    two_steps(runner, group(segs=data([0, 5, 0], 8)), "empty segments")
    got = runner([group(segs=[])])[0]     # no segment: norm 0, an executed step
    assert got["info"].tolist() == [0.0, 1.0, 0.0, 0.0] and got["state"][0] == 1.0
    assert runner([]) == []               # n_groups == 0


def check_two_groups(runner):
    ha, hb = dataclasses.replace(H, lr=1e-3, max_grad_norm=0.5), dataclasses.replace(H, lr=5e-4, weight_decay=0.01)
    A = group(ha, data([CHUNK + 1, 3], 1))
    B = group(hb, data([5, 2 * CHUNK + 5, 17], 2, gscale=0.01))
    B = next_group(B, runner([B])[0], grads([5, 2 * CHUNK + 5, 17], 3, 0.01))    # another step count
    B = next_group(B, runner([B])[0], grads([5, 2 * CHUNK + 5, 17], 4, 0.01))
    assert B["state"][0] == 2.0
    both = runner([A, B])
    alone = [runner([A])[0], runner([B])[0]]
    swapped = runner([B, A])
    for i, G in enumerate((A, B)):
        same(both[i], om.model32(G["h"], G["segs"], G["state"]), "two groups, group %d" % i)
        same_groups(both[i], alone[i], "group %d alone" % i)
        same_groups(swapped[1 - i], alone[i], "group %d, swapped" % i)
    assert both[0]["info"][1] < 1.0 and both[1]["info"][1] == 1.0 and both[0]["info"][0] != both[1]["info"][0]


def check_clipping(runner):
    sizes = [CHUNK + 1, 3]
    active = group(dataclasses.replace(H, max_grad_norm=0.5), data(sizes, 11))
    got = runner([active])[0]
    same(got, om.model32(active["h"], active["segs"], active["state"]), "clipping active")
    assert 0.0 < got["info"][1] < 1.0
    inactive = group(H, data(sizes, 11, gscale=0.01))
    off = group(dataclasses.replace(H, use_max_grad_norm=False), data(sizes, 11, gscale=0.01))
    a, b = runner([inactive])[0], runner([off])[0]
    same(a, om.model32(H, inactive["segs"], inactive["state"]), "clipping inactive")
    assert a["info"][1] == 1.0 and a["info"][0] < H.max_grad_norm
    same_groups(a, b, "a coefficient of 1 is no clipping")
    big = group(dataclasses.replace(H, use_max_grad_norm=False), data(sizes, 11, gscale=100.0))
    got = runner([big])[0]
    same(got, om.model32(big["h"], big["segs"], big["state"]), "use_max_grad_norm = False")
    assert got["info"][1] == 1.0 and got["info"][0] > H.max_grad_norm     # the norm is still reported
    segs = [(w, np.zeros_like(g), m, v) for w, g, m, v in data(sizes, 12)]
    zero = group(H, segs)
    got = runner([zero])[0]
    same(got, om.model32(H, segs, zero["state"]), "all-zero gradients")
    assert got["info"].tolist() == [0.0, 1.0, 0.0, 0.0] and got["state"][0] == 1.0
    for a, b in zip(got["segs"], segs):
        np.testing.assert_array_equal(bits(a[0]), bits(b[0]), "zero gradients moved a weight")
        assert not bits(a[2]).any() and not bits(a[3]).any()


def check_weight_decay(runner):
    h = dataclasses.replace(H, weight_decay=0.01)
    G = group(h, data([CHUNK + 1, 3], 13))
    two_steps(runner, G, "weight decay")
    plain = runner([group(H, G["segs"])])[0]
    assert (bits(plain["segs"][0][0]) != bits(runner([G])[0]["segs"][0][0])).any()


def trajectory(runner, h, sizes, seed, wscale, gscale, what, lrs):
    """len(lrs) consecutive calls: each bit-equal to model32 and, on exp_avg, exp_avg_sq and the weights after
    every step, within the criterion of torch.optim.Adam + clip_grad_norm_ against the float64 truth; the norm
    within one float32 ulp of the truth's. Returns the largest err / tol seen."""
    G = group(h, data(sizes, seed, wscale, gscale))
    t64 = [tuple(a.astype(np.float64) for a in s) for s in G["segs"]]
    t32 = om.Torch32(h, [s[0] for s in G["segs"]])
    worst = 0.0
    for step, lr in enumerate(lrs):
        hs = dataclasses.replace(h, lr=lr)
        if step:
            G = next_group(G, got, grads(sizes, seed + 100 * step, gscale), hs)
            t64 = [(w, g.astype(np.float64), m, v) for (w, _, m, v), g in zip(t64, [s[1] for s in G["segs"]])]
        else:
            G = dict(G, h=hs)
        got = runner([G])[0]
        same(got, om.model32(hs, G["segs"], G["state"]), "%s, step %d" % (what, step + 1))
        t64, norm64 = om.truth64(hs, t64, step)
        ref, _ = t32.step([s[1] for s in G["segs"]], lr)
        assert abs(float(got["info"][0]) - norm64) <= om.ulp32(norm64), (what, step, got["info"][0], norm64)
        assert got["state"][0] == step + 1
        for si in range(len(sizes)):
            for k, j, name in ((0, 0, "weights"), (2, 1, "exp_avg"), (3, 2, "exp_avg_sq")):
                err, _, tol = om.within(got["segs"][si][k], t64[si][k], ref[si][j],
                                        "%s, step %d, segment %d %s" % (what, step + 1, si, name))
                worst = max(worst, err / tol)
    return worst


LRS = (7e-4, 7e-4, 7e-4, 3e-4, 3e-4, 3e-4)    # lr changed after the third step


def check_six_steps(runner):
    sizes = [CHUNK + 1, 37]
    for name, h in (("clipped", dataclasses.replace(H, max_grad_norm=0.5)),
                    ("clipped, weight decay", dataclasses.replace(H, max_grad_norm=0.5, weight_decay=0.01)),
                    ("unclipped", dataclasses.replace(H, use_max_grad_norm=False))):
        trajectory(runner, h, sizes, 21, 1.0, 1.0, "six steps, " + name, LRS)


def check_small_magnitudes(runner):
    """Weights ~1e-3 and gradients ~1e-5: sqrt(v) is comparable to eps, so a misplaced eps shows."""
    for name, h in (("clipped", dataclasses.replace(H, max_grad_norm=1e-4)), ("unclipped", H),
                    ("weight decay", dataclasses.replace(H, weight_decay=0.01))):
        trajectory(runner, h, [CHUNK + 1, 37], 31, 1e-3, 1e-5, "small magnitudes, " + name, LRS)


def check_nonfinite(runner, value):
    sizes = [CHUNK + 1, 5]
    clean = group(H, data(sizes, 41))
    clean = next_group(clean, runner([clean])[0], grads(sizes, 42))     # moments and state that are not fresh
    bad = [g.copy() for g in grads(sizes, 43)]
    bad[-1][-1] = value
    poisoned = next_group(clean, dict(segs=clean["segs"], state=clean["state"]), bad)
    got = runner([poisoned])[0]
    for a, b in zip(got["segs"], poisoned["segs"]):
        for k in (0, 2, 3):
            np.testing.assert_array_equal(bits(a[k]), bits(b[k]), "a skipped step wrote")
    np.testing.assert_array_equal(bits(got["state"]), bits(clean["state"]))
    assert got["info"][2] == 1.0 and not np.isfinite(got["info"][0])
    same(got, om.model32(H, poisoned["segs"], poisoned["state"]), "skipped")
    after = runner([next_group(poisoned, got, [s[1] for s in clean["segs"]])])[0]
    same_groups(after, runner([clean])[0], "the step after a skipped one")
    assert after["info"][2] == 0.0 and after["state"][0] == 2.0
    # without the skip: the model's NaNs, a clean finish
    h = dataclasses.replace(H, skip_nonfinite=False)
    through = dict(poisoned, h=h)
    got = runner([through])[0]
    same(got, om.model32(h, through["segs"], through["state"]), "no skip", of=value_bits)
    assert got["info"][2] == 0.0 and got["state"][0] == 2.0 and np.isnan(got["segs"][-1][0][-1])


def check_huge_gradient(runner):
    segs = data([CHUNK + 1, 5], 51)
    segs[0][1][7] = 1e20
    G = group(H, segs)
    got = runner([G])[0]
    same(got, om.model32(H, segs, G["state"]), "a gradient of 1e20")
    norm64 = om.truth64(H, [tuple(a.astype(np.float64) for a in s) for s in segs], 0)[1]
    assert np.isfinite(got["info"][0]) and got["info"][2] == 0.0
    assert abs(float(got["info"][0]) - norm64) <= om.ulp32(norm64)
    assert all(np.isfinite(s[0]).all() for s in got["segs"])


def check_twice(runner, other=None):
    A = group(dataclasses.replace(H, max_grad_norm=0.5), data(ODD, 61))
    B = group(H, data([5], 62))
    first = runner([A, B])
    for again in (runner([A, B]), (other or runner)([A, B])):
        for a, b in zip(first, again):
            same_groups(a, b, "the same call twice")


# ---- the refusals -----------------------------------------------------------------------------------------------

def refusals():
    """[(what, mutate(tab, n_groups, ws) -> (tab, n_groups, ws), a word of the refusal)] on a valid two-group
    call of host arrays."""
    def field(gi, name, value):
        def f(tab, n, ws):
            setattr(tab[gi], name, value)
            return tab, n, ws
        return f

    def seg(gi, si, name, value):
        def f(tab, n, ws):
            v = value(tab) if callable(value) else value
            setattr(tab[gi].segments[si], name, v)
            return tab, n, ws
        return f

    w00 = lambda tab: tab[0].segments[0].weights
    out = [("a null table", lambda tab, n, ws: (None, n, ws), "table is null"),
           ("n_groups < 0", lambda tab, n, ws: (tab, -1, ws), "n_groups"),
           ("n_groups too large", lambda tab, n, ws: (tab, capi.LSM_OPT_MAX_GROUPS + 1, ws), "n_groups"),
           ("n_segments < 0", field(1, "n_segments", -1), "n_segments"),
           ("n_segments too large", field(0, "n_segments", capi.LSM_OPT_MAX_SEGMENTS + 1), "n_segments"),
           ("n < 0", seg(1, 0, "n", -1), "n < 0"),
           ("a null workspace", lambda tab, n, ws: (tab, n, None), "workspace is null"),
           ("a misaligned workspace", lambda tab, n, ws: (tab, n, ws + 4), "misaligned"),
           ("a null state", field(0, "state", None), "state or info is null"),
           ("a null info", field(1, "info", None), "state or info is null"),
           ("a misaligned state", lambda tab, n, ws: field(0, "state", tab[0].state + 4)(tab, n, ws), "misaligned"),
           ("a misaligned info", lambda tab, n, ws: field(0, "info", tab[0].info + 2)(tab, n, ws), "misaligned"),
           ("weights overlap exp_avg", seg(0, 0, "exp_avg", lambda tab: w00(tab) + 8), "written ranges overlap"),
           ("two groups' weights overlap", seg(1, 0, "weights", lambda tab: w00(tab) + 4), "written ranges overlap"),
           ("exp_avg_sq overlaps grads", seg(0, 1, "exp_avg_sq", lambda tab: tab[1].segments[0].grads), "overlaps grads"),
           ("state overlaps info", lambda tab, n, ws: field(0, "info", tab[1].state + 16)(tab, n, ws), "written ranges overlap"),
           ("the workspace overlaps weights", lambda tab, n, ws: (tab, n, w00(tab) & ~7), "written ranges overlap")]
    for name in ("weights", "grads", "exp_avg", "exp_avg_sq"):
        out.append(("null %s" % name, seg(0, 1, name, None), "null pointer"))
        out.append(("misaligned %s" % name, seg(1, 0, name, lambda tab, name=name: getattr(tab[1].segments[0], name) + 2),
                    "misaligned"))
    for name in ("lr", "eps", "weight_decay", "max_grad_norm"):
        for bad in (-1e-9, float("inf"), float("nan")):
            out.append(("%s = %r" % (name, bad), field(1, name, bad), name))
    for name in ("beta1", "beta2"):
        for bad in (-0.1, 1.0, float("nan")):
            out.append(("%s = %r" % (name, bad), field(0, name, bad), "betas"))
    return out


def check_refusals(lib):
    """Every refusal through both entry points on host arrays (a refusal comes before any launch or write, so it
    needs no device), each leaving every array as it was and the text in last_error."""
    groups = [group(H, data([CHUNK + 1, 3], 71), offsets=[0, CHUNK + 8]),
              group(H, data([9], 72), offsets=[0])]
    for what, mutate, word in refusals():
        arenas = []
        for G in groups:
            size = max(o + s[0].size for s, o in zip(G["segs"], G["offsets"])) + 8
            four = [np.full(size, CANARY, np.float32) for _ in range(4)]
            for s, off in zip(G["segs"], G["offsets"]):
                for k in range(4):
                    four[k][off:off + s[k].size] = s[k]
            arenas.append(four)
        states = np.tile(om.fresh_state(), (2, 1))
        infos = np.full((2, 4), CANARY, np.float32)
        ws = np.full(64, 321.0, np.float64)
        tab = table(groups, [[a.ctypes.data for a in four] for four in arenas],
                    [states[i].ctypes.data for i in range(2)], [infos[i].ctypes.data for i in range(2)])
        held = [a.copy() for four in arenas for a in four] + [states.copy(), infos.copy(), ws.copy()]
        t, n, w = mutate(tab, 2, ws.ctypes.data)
        for entry in ("host", "device"):
            if entry == "host":
                rc = lib.lsm_host_optim_step(t, n, C.c_void_p(w) if w else None)
            else:
                rc = lib.lsm_optim_step(t, n, C.c_void_p(w) if w else None, None)
            text = lib.lsm_optim_last_error().decode()
            assert rc != 0, "%s was accepted (%s)" % (what, entry)
            assert text.startswith("optim: ") and word in text, (what, text)
            now = [a for four in arenas for a in four] + [states, infos, ws]
            for a, b in zip(now, held):
                np.testing.assert_array_equal(bits(a), bits(b), "%s: an array was written" % what)
