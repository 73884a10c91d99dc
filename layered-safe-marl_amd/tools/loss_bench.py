"""Device time of the PPO loss and its gradient at the heads' outputs (the lines of GR_MAPPO.ppo_update and
cal_value_loss between evaluate_actions and the optimiser):

  (A) lsm.loss.PPOLoss.forward: four launches of csrc/lsm_loss.hip (the sums that do not depend on the network,
      the normaliser, the rows, the final scalars);
  (B) the same lines as float32 torch ops on the device, with torch.autograd.grad to the logits and the values
      and a float32 ValueNorm (update, then normalize): Categorical's log_prob and entropy, exp, clamp, min, the
      reference's huber_loss, max, the weighted means.

Shapes: one minibatch of tools/evaluate_bench.py -- M = 512000 rows, A = 25 actions -- with the reference's
defaults: clip 0.2, Huber delta 10, ValueNorm on, both active-mask flags on, 10 % of the active masks zero.
Inputs are seeded; old_log_probs is the row's own log-probability plus N(0, 0.2) (ratios on both sides of the
clip), value_preds the values plus N(0, 0.3).

Method: both sides are run once and checked first by the tests' criterion on the first 4096 rows (as a minibatch
of their own): the same torch lines in float64 are the truth, e32 is the float32 lines' error against it, and a
fused error above 4 * e32 + 4 * 2^-23 * max|truth| on dlogits, dvalues, the importance weights, the four scalars
or the normaliser's state ends the run. Rows of that part within a relative 1e-3 of a branch point where the
gradient jumps (ratio against 1 -+ clip outside it, |values - value_preds| against clip, |e| against delta, the
two losses against each other outside the clip) are moved off it beforehand (old_log_probs := the row's
log-probability, value_preds := values), as the tests redraw them: float32 and float64 may resolve a near-tie
differently. Then a warm-up, HIP events on the stream around `reps` back-to-back calls, the sides in alternating
rounds, and the median / min / max of the rounds' means (tools/bench_common.py's alternated()).

Bytes model of (A): per row A + 8 floats read (logits, actions, old_log_probs, advantages, values, value_preds,
returns, active_masks) and A + 1 written (dlogits, dvalues), so M * (2 A + 9) * 4 bytes, reported as a fraction of
the 8 TB/s HBM peak. Not counted: the first launch's second read of active_masks and returns and the optional
imp_weights (three more floats per row). The 121 MB working set is below the 256 MB last-level cache, so
back-to-back calls do not run cold.

    python layered-safe-marl_amd/tools/loss_bench.py [--out FILE] [--quick]
"""
from __future__ import annotations

import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_common import alternated, criterion, emit  # noqa: E402

DEV = "cuda:0"
ROWS, ACTIONS, CHECK_ROWS = 512000, 25, 4096
HBM_PEAK = 8.0e12
MARGIN = 1e-3


def torch_loss(cfg, logits, values, t, state, grads=True):
    """The reference's lines on device tensors of logits' dtype. t: actions (int64), old, adv, active, vpreds,
    returns; state: ValueNorm's [3]. Returns the outputs and, for the check, the branch quantities."""
    import torch
    dt = logits.dtype
    logits = logits.detach().requires_grad_(grads)
    values = values.detach().requires_grad_(grads)
    dist = torch.distributions.Categorical(logits=logits)
    logp = dist.log_prob(t["actions"])
    ent = dist.entropy()
    imp = torch.exp(logp - t["old"])
    c = float(cfg.clip_param)
    surr1 = imp * t["adv"]
    surr2 = torch.clamp(imp, 1.0 - c, 1.0 + c) * t["adv"]
    am = t["active"]
    policy_loss = (-torch.min(surr1, surr2) * am).sum() / am.sum()
    dist_entropy = (ent * am).sum() / am.sum()
    # ValueNorm.update, then normalize (onpolicy/utils/valuenorm.py)
    ret, beta = t["returns"], float(cfg.vn_beta)
    with torch.no_grad():
        rm = state[0] * beta + ret.mean() * (1.0 - beta)
        rms = state[1] * beta + (ret ** 2).mean() * (1.0 - beta)
        db = state[2] * beta + (1.0 - beta)
        mean = rm / db.clamp(min=1e-5)
        var = (rms / db.clamp(min=1e-5) - mean ** 2).clamp(min=1e-2)
        tg = (ret - mean) / torch.sqrt(var)
    d = values - t["vpreds"]
    vpc = t["vpreds"] + d.clamp(-c, c)
    dl = float(cfg.huber_delta)
    hub = lambda e: (abs(e) <= dl).to(dt) * e ** 2 / 2 + (e > dl).to(dt) * dl * (abs(e) - dl / 2)
    eo, ec = tg - values, tg - vpc
    lo, lc = hub(eo), hub(ec)
    value_loss = (torch.max(lo, lc) * am).sum() / am.sum()
    out = {"imp_weights": imp.detach(), "stats": torch.stack([policy_loss, value_loss, dist_entropy, imp.mean()]).detach(),
           "vn_state": torch.stack([rm, rms, db])}
    if grads:
        out["dlogits"], = torch.autograd.grad(policy_loss - dist_entropy * float(cfg.entropy_coef), logits)
        out["dvalues"], = torch.autograd.grad(value_loss * float(cfg.value_loss_coef), values)
    out["_branch"] = dict(logp=logp.detach(), ratio=imp.detach(), d=d.detach(), eo=eo.detach(), ec=ec.detach(),
                          lo=lo.detach(), lc=lc.detach())
    return out


def near_branch(cfg, b):
    import torch
    c, dl = float(cfg.clip_param), float(cfg.huber_delta)
    bad = torch.zeros_like(b["ratio"], dtype=torch.bool)
    for end in (1.0 - c, 1.0 + c):
        bad |= (b["ratio"] - end).abs() <= MARGIN * end
    bad |= (b["d"].abs() - c).abs() <= MARGIN * c
    for e in (b["eo"], b["ec"]):
        bad |= (e.abs() - dl).abs() <= MARGIN * dl
    top = torch.maximum(b["lo"].abs(), b["lc"].abs())
    bad |= (b["d"].abs() > c) & (top > 0) & ((b["lo"] - b["lc"]).abs() <= MARGIN * top)
    return bad


def run(quick):
    import torch
    from lsm.loss import DeviceValueNorm, LossConfig, PPOLoss
    cfg = LossConfig(num_actions=ACTIONS)
    loss = PPOLoss(cfg, DEV)
    g = torch.Generator(device=DEV).manual_seed(7)
    rnd = lambda *s: torch.randn(s, generator=g, device=DEV)
    logits = 1.5 * rnd(ROWS, ACTIONS)
    values = rnd(ROWS)
    t = {"actions": torch.randint(0, ACTIONS, (ROWS,), generator=g, device=DEV), "adv": rnd(ROWS),
         "active": (torch.rand(ROWS, generator=g, device=DEV) > 0.1).float(), "vpreds": values + 0.3 * rnd(ROWS),
         "returns": 0.5 + 2.0 * rnd(ROWS)}
    far = torch.rand(ROWS, generator=g, device=DEV) < 0.02        # beyond the Huber delta, on either side
    t["returns"] = torch.where(far, t["returns"] + 40.0 * torch.sign(rnd(ROWS)), t["returns"])
    logp = torch.distributions.Categorical(logits=logits).log_prob(t["actions"])
    t["old"] = logp + 0.2 * rnd(ROWS)
    state0 = torch.tensor([0.1, 0.75, 0.5], device=DEV)
    vn = DeviceValueNorm(DEV)

    def fused(lg=logits, vl=values, tt=t):
        vn.state.copy_(state0)
        return loss.forward(lg, vl, actions=tt["actions_f"], old_log_probs=tt["old"], advantages=tt["adv"],
                            value_preds=tt["vpreds"], returns=tt["returns"], active_masks=tt["active"], value_norm=vn)

    def plain(lg=logits, vl=values, tt=t):
        return torch_loss(cfg, lg, vl, tt, state0)

    # ---- the tests' criterion on the first rows as a minibatch of their own --------------------------------
    n = CHECK_ROWS
    s = {k: v[:n].clone() for k, v in t.items()}
    slg, svl = logits[:n].contiguous(), values[:n].contiguous()
    dbl = lambda d: {k: (v.double() if v.is_floating_point() else v) for k, v in d.items()}
    for _ in range(5):
        r = torch_loss(cfg, slg.double(), svl.double(), dbl(s), state0.double())
        bad = near_branch(cfg, r["_branch"])
        if not bool(bad.any()):
            break
        s["old"] = torch.where(bad, r["_branch"]["logp"].float(), s["old"])
        s["vpreds"] = torch.where(bad, svl, s["vpreds"])
    else:
        raise SystemExit("rows of the checked part stay near a branch point")
    s["actions_f"] = s["actions"].float()
    a = {k: v.clone() for k, v in fused(slg, svl, s).items()}
    a["vn_state"] = vn.state.clone()
    b = plain(slg, svl, s)
    checks = criterion(a, b, r, ("dlogits", "dvalues", "imp_weights", "stats", "vn_state"), "")
    # ---- timing --------------------------------------------------------------------------------------------
    t["actions_f"] = t["actions"].float()
    sides = {"fused": (fused, 5 if quick else 20), "torch": (plain, 2 if quick else 5)}
    for fn, _ in sides.values():   # warm-up
        fn()
    ms = alternated(sides)
    nbytes = ROWS * (2 * ACTIONS + 9) * 4
    res = dict(ms, rows=ROWS, num_actions=ACTIONS, checked_rows=n, checks=checks, bytes_model=nbytes,
               fused_fraction_of_hbm_peak=nbytes / (ms["fused"]["median"] * 1e-3) / HBM_PEAK,
               ratio_torch_over_fused=ms["torch"]["median"] / ms["fused"]["median"],
               note="fused includes the 12-byte copy that resets the normaliser's state before each call")
    print("loss: fused %.3f ms, torch %.3f ms (x%.2f), %.1f %% of the HBM peak on the bytes model"
          % (ms["fused"]["median"], ms["torch"]["median"], res["ratio_torch_over_fused"],
             100 * res["fused_fraction_of_hbm_peak"]), file=sys.stderr, flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="fewer calls per round")
    a = ap.parse_args()
    emit({"loss_bench": run(a.quick)}, a.out)


if __name__ == "__main__":
    main()
