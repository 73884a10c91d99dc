"""What the *_bench.py tools share: the alternating timer, the tests' float64 criterion and the writer of the
one JSON line."""
from __future__ import annotations

import json
import os

ROUNDS = 7


def timed(fn, reps):
    """Mean device milliseconds per call of fn over reps calls (events on the current stream)."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternated(sides):
    """sides: {name: (fn, reps)}. ROUNDS rounds, each timing every side once in turn (so that drift of
    the machine falls on all sides alike). Returns {name: {"median", "min", "max"}} of the rounds' means,
    milliseconds per call."""
    ms = {k: [] for k in sides}
    for _ in range(ROUNDS):
        for k, (fn, reps) in sides.items():
            ms[k].append(timed(fn, reps))
    return {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "reps_per_round": sides[k][1],
                "rounds": ROUNDS} for k, v in ms.items()}


def criterion(fused, torch32, truth64, names, label, special=None, bound="the tolerance", enforce=True):
    """The tests' criterion on each of names: truth64[name] is the truth, e32 the error of torch32[name]
    against it, and a fused error above 4 * e32 + 4 * 2^-23 * max|truth| ends the run (enforce=False: it is
    only recorded). special: {name: f(checks so far, truth) -> that name's tolerance instead}. label stands
    before the name in the refusal, bound before the tolerance. Returns {name: {"fused_err_vs_float64",
    "torch_err_vs_float64", "tolerance"}}."""
    checks = {}
    for name in names:
        truth = truth64[name]
        e32 = float((torch32[name].double().reshape(truth.shape) - truth).abs().max().item())
        err = float((fused[name].double().reshape(truth.shape) - truth).abs().max().item())
        tol = 4.0 * e32 + 4.0 * 2.0 ** -23 * float(truth.abs().max().item())
        if special and name in special:
            tol = special[name](checks, truth)
        checks[name] = {"fused_err_vs_float64": err, "torch_err_vs_float64": e32, "tolerance": tol}
        if enforce and not err <= tol:
            raise SystemExit("%s: fused error %g against float64 exceeds %s %g (torch float32: %g)"
                             % ((label + " " + name).strip(), err, bound, tol, e32))
    return checks


def emit(obj, out_path):
    """One JSON line of obj to out_path (when given; its directory is made) and to stdout."""
    line = json.dumps(obj)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(line + "\n")
    print(line)
