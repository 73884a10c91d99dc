"""The yardstick of the PPO loss tests (include/lsm_loss.h): a numpy float64 model written out from the
header's formulas, gradients included as closed forms, and the same lines as torch ops with autograd on the
CPU -- GR_MAPPO.ppo_update / cal_value_loss, huber_loss / mse_loss, ValueNorm.update / normalize and
Categorical, written from the reference's formulas. In double the torch lines pin the model (about 1e-14
relative); in float32 they give e32, one float32 evaluation's error, for the project's tolerance
4 * e32 + 4 * 2^-23 * s per case and output tensor.

Inputs: a dict of float32 arrays -- logits [M, A], actions [M], avail [M, A] or None, old [M], adv [M],
active [M], values [M], vpreds [M], returns [M], vn_state [3]. cfg: lsm.loss.LossConfig. The config's float
fields are the struct's float32 values."""
import numpy as np

FLT_MIN = float(np.finfo(np.float32).min)
STATS = ("policy_loss", "value_loss", "dist_entropy", "ratio")


def f32(v):
    return float(np.float32(v))


def clamp_actions(actions, A):
    """include/lsm_evaluate.h's clamp: (int actions, flagged)."""
    a = np.asarray(actions, dtype=np.float64)
    nan = np.isnan(a)
    c = np.trunc(np.clip(np.where(nan, 0.0, a), 0, A - 1)).astype(np.int64)
    bad = nan | (a < 0) | (a >= A) | (a != np.floor(np.where(nan, 0.0, a)))
    return c, bad


def masked(inp):
    lg = np.asarray(inp["logits"], dtype=np.float64).copy()
    if inp.get("avail") is not None:
        lg[np.asarray(inp["avail"]) == 0] = FLT_MIN
    return lg


def huber64(e, d):
    a = (np.abs(e) <= d).astype(np.float64)
    b = (e > d).astype(np.float64)
    return a * e ** 2 / 2 + b * d * (np.abs(e) - d / 2), a * e + b * d


def valuenorm64(state, returns, beta):
    """ValueNorm.update then running_mean_var in float64 from a float32 state: (state', mean, std)."""
    rm, rms, db = (float(v) for v in np.asarray(state, dtype=np.float32))
    r = np.asarray(returns, dtype=np.float64)
    wb, om = f32(beta), f32(1.0 - beta)
    rm = rm * wb + r.mean() * om
    rms = rms * wb + (r ** 2).mean() * om
    db = db * wb + om
    dm, dms = rm / max(db, f32(1e-5)), rms / max(db, f32(1e-5))
    var = max(dms - dm ** 2, f32(1e-2))
    return np.array([rm, rms, db]), dm, np.sqrt(var)


def model64(cfg, inp, actor=True, critic=True):
    """{dlogits, dvalues, imp_weights, stats [4] (NaN for a skipped half), vn_state, denorm} and the
    intermediate values the case generator needs (ratio, d, e_o, e_c, l_o, l_c), all float64."""
    out = {"stats": np.full(4, np.nan)}
    am = np.asarray(inp["active"], dtype=np.float64) if inp.get("active") is not None else None
    c = f32(cfg.clip_param)
    with np.errstate(all="ignore"):
        if actor:
            lg = masked(inp)
            M, A = lg.shape
            act, out["bad"] = clamp_actions(inp["actions"], A)
            mx = lg.max(axis=1, keepdims=True)
            d = lg - mx
            e = np.exp(d)
            s = e.sum(axis=1, keepdims=True)
            ls = np.log(s)
            lp = d - ls
            p = e / s
            H = -(np.where(e > 0, p * lp, 0.0)).sum(axis=1)
            logp = lp[np.arange(M), act]
            ratio = np.exp(logp - np.asarray(inp["old"], dtype=np.float64))
            adv = np.asarray(inp["adv"], dtype=np.float64)
            lo, hi = f32(1.0 - c), f32(1.0 + c)
            surr1, surr2 = ratio * adv, np.clip(ratio, lo, hi) * adv
            mn = np.where(np.isnan(surr1), surr1, np.minimum(surr1, surr2))
            t1 = np.where(surr1 < surr2, 1.0, np.where(surr2 < surr1, 0.0, 0.5))
            inr = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)
            g = adv * (t1 + (1 - t1) * inr)
            w = am if cfg.use_policy_active_masks else np.ones(M)
            kp = w / w.sum()
            dlogp = -(kp * g * ratio)
            dent = -(f32(cfg.entropy_coef) * kp)
            hot = np.zeros((M, A))
            hot[np.arange(M), act] = 1.0
            dl = dlogp[:, None] * (hot - p) + dent[:, None] * -(p * (lp + H[:, None]))
            dl = np.where(e > 0, dl, dlogp[:, None] * hot)
            if inp.get("avail") is not None:
                dl = np.where(np.asarray(inp["avail"]) == 0, 0.0, dl)
            out.update(dlogits=dl, imp_weights=ratio, logp=logp, entropy=H, ratio=ratio, surr1=surr1, surr2=surr2)
            out["stats"][[0, 2, 3]] = -(w * mn).sum() / w.sum(), (w * H).sum() / w.sum(), ratio.mean()
        if critic:
            v, vp, ret = (np.asarray(inp[k], dtype=np.float64) for k in ("values", "vpreds", "returns"))
            M = v.size
            d = v - vp
            vpc = vp + np.clip(d, -c, c)
            tg = ret
            if cfg.use_valuenorm:
                out["vn_state"], mean, sd = valuenorm64(inp["vn_state"], ret, cfg.vn_beta)
                out["denorm"] = np.array([sd, mean])
                tg = (ret - mean) / sd
            eo, ec = tg - v, tg - vpc
            if cfg.use_huber_loss:
                (lo_, go), (lc, gc) = huber64(eo, f32(cfg.huber_delta)), huber64(ec, f32(cfg.huber_delta))
            else:
                lo_, go, lc, gc = eo ** 2 / 2, eo, ec ** 2 / 2, ec
            w = am if cfg.use_value_active_masks else np.ones(M)
            k = w / w.sum() * f32(cfg.value_loss_coef)
            l, dv = lo_, -(k * go)
            if cfg.use_clipped_value_loss:
                l = np.maximum(lo_, lc)
                to = np.where(lo_ > lc, 1.0, np.where(lc > lo_, 0.0, 0.5))
                ko = np.where(to > 0, k * to, 0.0)          # selected, as torch's masked_fill / where
                kc = np.where((to < 1) & (np.abs(d) <= c), k * (1 - to), 0.0)
                dv = -(ko * go + kc * gc)
            out["dvalues"] = dv
            out["stats"][1] = (w * l).sum() / w.sum()
            out.update(d=d, e_o=eo, e_c=ec, l_o=lo_, l_c=lc)
    return out


def torch_objectives(cfg, logits, values, inp, dtype):
    """The reference's lines as torch ops on `logits` [M, A] and `values` [M] (tensors of `dtype` inside a
    graph, or None to skip that half): {actor: policy_loss - entropy_coef * dist_entropy, critic: value_loss *
    value_loss_coef (what the reference calls backward() on), imp_weights, stats, vn_state, denorm}. A row
    without any available action gets zero logits (uniform: the project's convention, include/lsm_evaluate.h;
    torch's own rounding of -FLT_MAX - logsumexp is not imitated)."""
    import torch
    t = lambda k: torch.tensor(np.asarray(inp[k]), dtype=dtype)
    np_ = lambda x: x.detach().to(torch.float64).numpy()
    out = {"stats": np.full(4, np.nan), "actor": None, "critic": None}
    am = t("active") if inp.get("active") is not None else None
    c = f32(cfg.clip_param)
    if logits is not None:
        x = logits
        if inp.get("avail") is not None:
            av = torch.tensor(np.asarray(inp["avail"]))
            x = logits.clone()
            x[av == 0] = FLT_MIN
            x[(av == 0).all(dim=1)] = 0.0
        act, _ = clamp_actions(inp["actions"], x.shape[1])
        dist = torch.distributions.Categorical(logits=x)
        logp = dist.log_prob(torch.tensor(act))
        ent = dist.entropy()
        imp = torch.exp(logp - t("old"))
        adv = t("adv")
        surr1 = imp * adv
        surr2 = torch.clamp(imp, f32(1.0 - c), f32(1.0 + c)) * adv
        mn = torch.min(surr1, surr2)
        if cfg.use_policy_active_masks:
            policy_loss = (-mn * am).sum() / am.sum()
            dist_entropy = (ent * am).sum() / am.sum()
        else:
            policy_loss, dist_entropy = -mn.mean(), ent.mean()
        out["actor"] = policy_loss - dist_entropy * f32(cfg.entropy_coef)
        out["imp_weights"] = np_(imp)
        out["stats"][[0, 2, 3]] = float(policy_loss.detach()), float(dist_entropy.detach()), float(imp.detach().mean())
    if values is not None:
        vp, ret = t("vpreds"), t("returns")
        vpc = vp + (values - vp).clamp(-c, c)
        tg = ret
        if cfg.use_valuenorm:
            # the scalars as a float32 tensor op takes them (in double they are then the model's too)
            wb, om = f32(cfg.vn_beta), f32(1.0 - float(cfg.vn_beta))
            rm, rms, db = (t("vn_state")[i].clone() for i in range(3))
            with torch.no_grad():
                rm.mul_(wb).add_(ret.mean() * om)
                rms.mul_(wb).add_((ret ** 2).mean() * om)
                db.mul_(wb).add_(1.0 * om)
                dm, dms = rm / db.clamp(min=f32(1e-5)), rms / db.clamp(min=f32(1e-5))
                var = (dms - dm ** 2).clamp(min=f32(1e-2))
            tg = (ret - dm) / torch.sqrt(var)
            out["vn_state"] = np_(torch.stack([rm, rms, db]))
            out["denorm"] = np_(torch.stack([torch.sqrt(var), dm]))
        eo, ec = tg - values, tg - vpc
        if cfg.use_huber_loss:
            dl = f32(cfg.huber_delta)
            hub = lambda e: (abs(e) <= dl).to(dtype) * e ** 2 / 2 + (e > dl).to(dtype) * dl * (abs(e) - dl / 2)
            lo_, lc = hub(eo), hub(ec)
        else:
            lo_, lc = eo ** 2 / 2, ec ** 2 / 2
        l = torch.max(lo_, lc) if cfg.use_clipped_value_loss else lo_
        value_loss = (l * am).sum() / am.sum() if cfg.use_value_active_masks else l.mean()
        out["critic"] = value_loss * f32(cfg.value_loss_coef)
        out["stats"][1] = float(value_loss.detach())
    return out


def model_torch(cfg, inp, dtype, actor=True, critic=True):
    """torch_objectives on leaf logits and values, with autograd to them: {dlogits, dvalues, imp_weights,
    stats, vn_state, denorm} as float64 arrays."""
    import torch
    leaf = lambda k: torch.tensor(np.asarray(inp[k]), dtype=dtype).requires_grad_(True)
    logits, values = (leaf("logits") if actor else None), (leaf("values") if critic else None)
    out = torch_objectives(cfg, logits, values, inp, dtype)
    if actor:
        out.pop("actor").backward()
        out["dlogits"] = logits.grad.to(torch.float64).numpy()
    if critic:
        out.pop("critic").backward()
        out["dvalues"] = values.grad.to(torch.float64).numpy()
    return out


def bound(w64, e32):
    w64 = np.asarray(w64, dtype=np.float64)
    fin = w64[np.isfinite(w64)]
    s = float(np.abs(fin).max()) if fin.size else 0.0
    return 4.0 * e32 + 4.0 * 2.0 ** -23 * s


def tensor_bound(w64, w32):
    """(tolerance, e32) of one output tensor; entries that are NaN in the model are NaN in both."""
    w64, w32 = np.asarray(w64, dtype=np.float64), np.asarray(w32, dtype=np.float64)
    fin = np.isfinite(w64)
    assert (np.isnan(w32) == np.isnan(w64)).all()
    e32 = float(np.abs(w32 - w64)[fin].max()) if fin.any() else 0.0
    return bound(w64, e32), e32
