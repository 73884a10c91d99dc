"""Numpy model of the learner hand-off (include/lsm_learner.h): compute_returns, the advantages and the
minibatch gather, stated operation by operation in float32 as the header gives them. The model and the
fixtures recorded from the reference (tests/golden/returns/) check each other; the HIP kernels are then
compared with both."""
import numpy as np

f32 = np.float32


def dn(x, denorm):
    """x * denorm[0] + denorm[1], two separately rounded float32 operations; x without a normaliser."""
    if denorm is None:
        return x
    return (x * f32(denorm[0])).astype(f32) + f32(denorm[1])


def compute_returns(rewards, value_preds, masks, bad_masks, next_value, denorm, returns, gamma, gae_lambda,
                    use_gae=True, use_proper_time_limits=False):
    """In place on value_preds / returns, [rows][M] float32 (any trailing shape: rows are the first axis)."""
    T = rewards.shape[0]
    g, gl = f32(gamma), f32(gamma * gae_lambda)
    v = value_preds
    if use_gae:
        v[T] = next_value
        gae = np.zeros_like(next_value, dtype=f32)
        for t in range(T - 1, -1, -1):
            m = masks[t + 1]
            delta = (rewards[t] + (g * dn(v[t + 1], denorm)) * m) - dn(v[t], denorm)
            if use_proper_time_limits and denorm is not None:
                gae = delta + (gl * gae) * m
            else:
                gae = delta + (gl * m) * gae
            if use_proper_time_limits:
                gae = gae * bad_masks[t + 1]
            returns[t] = gae + dn(v[t], denorm)
    else:
        returns[T] = next_value
        for t in range(T - 1, -1, -1):
            x = ((returns[t + 1] * g) * masks[t + 1]) + rewards[t]
            if use_proper_time_limits:
                b = bad_masks[t + 1]
                x = x * b + (f32(1) - b) * dn(v[t], denorm)
            returns[t] = x
    assert returns.dtype == f32 and v.dtype == f32


def raw_advantages(returns, value_preds, denorm):
    """returns - dn(value_preds) over the first T rows, float32."""
    return returns[:-1] - dn(value_preds[:-1], denorm)


def advantage_stats(adv, active):
    """float64 (mean, population std, count) over entries whose active mask is non-zero."""
    x = adv.astype(np.float64).copy()
    x[active == 0.0] = np.nan
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return np.array([np.nanmean(x), np.nanstd(x), float(np.count_nonzero(active != 0.0))])


def normalised_advantages(adv, stats):
    return ((adv - f32(stats[0])) / f32(stats[1] + 1e-5)).astype(f32)


def reference_advantages(adv, active):
    """The reference's normalisation (graph_mappo.py:264-268) restated: float32 nanmean / nanstd over the
    active entries, then (adv - mean) / (std + 1e-5) in float32."""
    c = adv.copy()
    c[active == 0.0] = np.nan
    return (adv - np.nanmean(c)) / (np.nanstd(c) + 1e-5)


def mask_bits(words, E):
    """[..., W] uint64 disconnect words -> [..., E] bool."""
    w = np.asarray(words).astype(np.uint64)
    sh = np.arange(64, dtype=np.uint64)
    bits = ((w[..., None] >> sh) & np.uint64(1)).astype(bool)
    return bits.reshape(w.shape[:-1] + (-1,))[..., :E]


def gather_rows(src, indices):
    """dst[b] = src[indices[b]]; an index outside [0, rows) gives a zero row."""
    idx = np.asarray(indices)
    ok = (idx >= 0) & (idx < src.shape[0])
    out = src[np.where(ok, idx, 0)].copy()
    out[~ok] = 0
    return out


def gather_compact_adj(A, masks, indices, N):
    """dst[b][r][c] = (bit r | bit c of masks[i]) ? 0 : A[i // N][r][c], i = indices[b] (a select)."""
    idx = np.asarray(indices)
    E = A.shape[-1]
    ok = (idx >= 0) & (idx < masks.shape[0])
    i = np.where(ok, idx, 0)
    bits = mask_bits(masks[i], E)
    drop = bits[:, :, None] | bits[:, None, :] | ~ok[:, None, None]
    return np.where(drop, f32(0), A[i // N]).astype(f32)
