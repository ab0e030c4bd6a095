"""numpy float64 reference of matgcn_crps_loss / matgcn_crps_loss_grad (include/matgcn.h): the mean CRPS of an ensemble
over the unmasked elements and its gradient w.r.t. every sample, with the (value, sample index) rank rule.  De-scaling,
labels and mask are mc_scores_ref's (float32, one rounding per operation); everything behind them is float64."""
import numpy as np

import mc_scores_ref as M

F32 = np.float32


def ranks(p):
    """(S, ...) -> the 0-based rank of every sample along axis 0, sorted by (value, sample index): a stable argsort"""
    order = np.argsort(p, axis=0, kind="stable")
    r = np.empty_like(order)
    np.put_along_axis(r, order, np.broadcast_to(np.arange(p.shape[0]).reshape((-1,) + (1,) * (p.ndim - 1)), p.shape), axis=0)
    return r


def element_crps(p, l):
    """per element, float64, from the float32 samples p (S, ...) and labels l (...):
    (1/S) sum_s |p_s - l| - (1/S^2) sum_i (2i - S + 1) p_(i)"""
    return M.crps_sorted(np.sort(p, axis=0), l)


def value(samples, y, mean=0.0, std=1.0, null_val=0.0, min_s=1e-4):
    """samples (S, B, out, N, od), y the raw labels (B, out, N, od).  Returns (result (1 + out,) float32 - [over all
    horizons, per horizon], 0 where nothing is kept -, the float64 quotients before rounding, the kept count M)"""
    p = M.descale(samples, mean, std)
    l, mask = M.labels(y, mean, std, null_val, min_s)
    c = np.where(mask, element_crps(p, l), 0.0)
    tot, cnt = c.sum(axis=(0, 2, 3)), mask.sum(axis=(0, 2, 3)).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(cnt > 0, tot / cnt, 0.0)
        total = tot.sum() / cnt.sum() if cnt.sum() > 0 else 0.0
    exact = np.concatenate([[total], per])
    return exact.astype(F32), exact, float(cnt.sum())


def grad(samples, y, mean=0.0, std=1.0, null_val=0.0, min_s=1e-4, upstream=1.0):
    """d result[0] / d samples, float64 (S, B, out, N, od):
    upstream * (std / M) * (sgn(p_s - l) / S - (2 r_s - S + 1) / S^2), 0 on masked elements"""
    p = M.descale(samples, mean, std)
    l, mask = M.labels(y, mean, std, null_val, min_s)
    s = float(p.shape[0])
    m = float(mask.sum())
    if m == 0:
        return np.zeros(p.shape, dtype=np.float64)
    sg = np.sign(p.astype(np.float64) - l.astype(np.float64)[None])
    g = sg / s - (2.0 * ranks(p) - s + 1.0) / (s * s)
    w = float(upstream) * float(F32(std)) / m
    return np.where(mask[None], w * g, 0.0)


def pairwise(samples, y, mean=0.0, std=1.0):
    """per element mean|x - l| - mean|x - x'| / 2 over all S^2 pairs (mc_scores_ref.crps_brute), float64"""
    p = M.descale(samples, mean, std)
    l, _ = M.labels(y, mean, std, float("nan"), -1.0)
    return M.crps_brute(p, l)
