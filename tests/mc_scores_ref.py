"""numpy reference of matgcn_mc_quantiles / matgcn_mc_scores (include/matgcn.h): float32 for the de-scale and the
quantile - each operation one numpy float32 operation, hence one rounding, which is what the kernels promise bit for bit -,
float64 for the score terms.  Also the O(S^2) ensemble CRPS the sorted form is checked against."""
import math

import numpy as np

F32 = np.float32
SCORE_SUMS = 5


def descale(x, mean=0.0, std=1.0):
    """x*std + mean: a float32 product, then a float32 sum"""
    t = np.asarray(x, dtype=F32) * F32(std)
    return t + F32(mean)


def sorted_samples(samples, mean=0.0, std=1.0):
    """(S, ...) -> de-scaled and sorted along the sample axis"""
    return np.sort(descale(samples, mean, std), axis=0)


def level_terms(q, s):
    """(j, j2, g, q as the double of its float) of one level: h = (double)q*(S-1), j = floor(h), g = (float)(h - j)"""
    qd = float(F32(q))
    h = qd * (s - 1)
    j = int(math.floor(h))
    return j, min(j + 1, s - 1), F32(h - j), qd


def quantiles_sorted(xs, probs):
    """(len(probs), ...) float32 from the sorted (S, ...) samples: Q = lo + g*(hi - lo), three float32 roundings"""
    s = xs.shape[0]
    out = np.empty((len(probs),) + xs.shape[1:], dtype=F32)
    for k, q in enumerate(probs):
        j, j2, g, _ = level_terms(q, s)
        lo, hi = xs[j], xs[j2]
        d = hi - lo
        t = g * d
        out[k] = lo + t
        assert d.dtype == F32 and t.dtype == F32
    return out


def quantiles(samples, probs, mean=0.0, std=1.0):
    return quantiles_sorted(sorted_samples(samples, mean, std), probs)


def labels(y, mean=0.0, std=1.0, null_val=0.0, min_s=1e-4):
    """(l float32, mask) of the raw labels y: de-scale, |l| < min_s -> 0, mask = l != null_val (NaN: not isnan)"""
    l = descale(y, mean, std).copy()
    with np.errstate(invalid="ignore"):
        l[np.abs(l) < F32(min_s)] = F32(0.0)
    mask = ~np.isnan(l) if math.isnan(null_val) else (l != F32(null_val))
    return l, mask


def crps_sorted(xs, l):
    """per element: (1/S) sum_i |x(i) - l| - (1/S^2) sum_i (2i - S + 1) x(i), float64"""
    s = xs.shape[0]
    x = xs.astype(np.float64)
    coef = (2.0 * np.arange(s) - s + 1.0).reshape((s,) + (1,) * (xs.ndim - 1))
    return np.abs(x - l.astype(np.float64)[None]).sum(0) / s - (coef * x).sum(0) / (float(s) * float(s))


def crps_brute(x, l):
    """mean|x - l| - mean|x - x'| / 2 over all S^2 pairs, float64; x (S, ...) in any order"""
    x = x.astype(np.float64)
    pair = np.zeros(x.shape[1:], dtype=np.float64)
    for i in range(x.shape[0]):
        pair += np.abs(x - x[i][None]).sum(0)
    s = float(x.shape[0])
    return np.abs(x - l.astype(np.float64)[None]).mean(0) - 0.5 * pair / (s * s)


def score_terms(xs, l, probs):
    """(5 + len(probs), ...) float64 terms [1, CRPS, covered, width, Winkler, pinball per level] of every element, from
    the sorted samples xs (S, ...) and the float32 labels l (...)"""
    q = quantiles_sorted(xs, probs)
    qf, ql = q[0], q[-1]
    ld, qfd, qld = l.astype(np.float64), qf.astype(np.float64), ql.astype(np.float64)
    alpha = 1.0 - (float(F32(probs[-1])) - float(F32(probs[0])))
    c = 2.0 / alpha if alpha != 0.0 else 0.0
    width = qld - qfd
    with np.errstate(invalid="ignore"):
        covered = ((qf <= l) & (l <= ql)).astype(np.float64)
        winkler = (width + c * np.maximum(qfd - ld, 0.0)) + c * np.maximum(ld - qld, 0.0)
        terms = [np.ones_like(ld), crps_sorted(xs, l), covered, width, winkler]
        for k, p in enumerate(probs):
            pd = float(F32(p))
            d = ld - q[k].astype(np.float64)
            terms.append(np.maximum(pd * d, (pd - 1.0) * d))
    return np.stack(terms, 0)


def score_sums(samples, y, probs, mean=0.0, std=1.0, null_val=0.0, min_s=1e-4):
    """samples (S, B, out, N, od), y the raw labels (B, out, N, od).  Returns (sums, abs_sums), both (out, 5 + len(probs))
    float64: the per-horizon sums over the unmasked elements, and the sums of the terms' magnitudes (the scale of the
    summation-order noise)."""
    xs = sorted_samples(samples, mean, std)
    l, mask = labels(y, mean, std, null_val, min_s)
    terms = np.where(mask[None], score_terms(xs, l, probs), 0.0)       # (K, B, out, N, od)
    return terms.sum(axis=(1, 3, 4)).T.copy(), np.abs(terms).sum(axis=(1, 3, 4)).T.copy()
