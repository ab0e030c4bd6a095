"""numpy reference of the sums grouped per (horizon, node) - matgcn_metric_sums_nodes / matgcn_mc_scores_nodes
(include/matgcn.h).  The per-element values come from the references of the per-horizon entry points
(metrics_ref.metric_elements, mc_scores_ref.score_terms); what is added here is the grouping, its sequential rule - entry
[o][n] starts from the stored value (or 0) and takes its terms one add at a time in ascending (b, c) - and, for the scores,
the descriptor: per-node affines (each a float32 product, then a float32 sum), the clamp before the sort, the truth filter."""
import math

import numpy as np

import mc_scores_ref as MC
import metrics_ref as M

F32, F64 = np.float32, np.float64
NAN = float("nan")


def accumulate(terms, start=None):
    """terms (K, B, out, N, od) float64 -> (out, N, K): ``start`` (or 0) + the terms, one add each, ascending (b, c)"""
    k, b, out, n, od = terms.shape
    acc = np.zeros((k, out, n), dtype=F64) if start is None else np.ascontiguousarray(np.moveaxis(start, 2, 0), dtype=F64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(b):
            for c in range(od):
                acc = acc + terms[:, i, :, :, c]
    return np.ascontiguousarray(np.moveaxis(acc, 0, 2))


def metric_terms(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s, label_start=None):
    """(14, B, out, N, od) float64: what one element adds to each of the sums of metrics_ref.metric_sums_ref"""
    l, p, keep = M.metric_elements(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s,
                                   label_start, F32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p - l
        ad, sq, ap = np.abs(d), d * d, np.abs(d / l)
        assert ad.dtype == F32 and sq.dtype == F32 and ap.dtype == F32
        valid, nz = keep & ~np.isnan(l), keep & (l != 0)
        l64, p64 = l.astype(F64), p.astype(F64)
        nan0 = lambda a: np.where(np.isnan(a), 0.0, a)
        terms = [keep, valid] + [np.where(valid, nan0(t.astype(F64)), 0.0) for t in (ad, sq, ap)]
        terms += [nz] + [np.where(nz, nan0(t.astype(F64)), 0.0) for t in (ad, sq, ap)]
        terms += [np.where(keep, t, 0.0) for t in (l64, l64 * l64, p64, p64 * p64, l64 - p64)]
    return np.stack([np.asarray(t, dtype=F64) for t in terms], 0)


def metric_sums_nodes_ref(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s,
                          label_start=None, start=None):
    """(out, N, 14) float64"""
    return accumulate(metric_terms(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s,
                                   label_start), start)


def descale_nodes(x, mean=None, std=None, group_mean=None, group_std=None):
    """x (..., N, od) float32 through the descriptor's affines (None = identity), node axis -2"""
    x = np.asarray(x, dtype=F32)
    for mu, sd in ((mean, std), (group_mean, group_std)):
        if mu is None:
            continue
        mu, sd = (np.asarray(v, dtype=F32).reshape(-1)[:, None] for v in (mu, sd))
        t = x * sd
        x = t + mu
        assert t.dtype == F32 and x.dtype == F32
    return x


def sorted_samples_nodes(samples, mean=None, std=None, group_mean=None, group_std=None, clamp_min=NAN):
    """(S, ..., N, od): de-scaled, clamped from below, sorted along the sample axis"""
    x = descale_nodes(samples, mean, std, group_mean, group_std).copy()
    if not math.isnan(clamp_min):
        x[x < F32(clamp_min)] = F32(clamp_min)
    return np.sort(x, axis=0)


def quantiles_nodes(samples, probs, **scale):
    return MC.quantiles_sorted(sorted_samples_nodes(samples, **scale), probs)


def score_terms_nodes(samples, y, probs, mean=None, std=None, group_mean=None, group_std=None, clamp_min=NAN,
                      truth_min=NAN, null_val=0.0, min_s=1e-4):
    """samples (S, B, out, N, od), y the raw labels (B, out, N, od) -> (5 + levels, B, out, N, od) float64 terms, zeros
    at elements that are left out (l <= truth_min, tested before |l| < min_s -> 0) or masked (l == null_val; NaN: NaN)"""
    xs = sorted_samples_nodes(samples, mean, std, group_mean, group_std, clamp_min)
    l = descale_nodes(y, mean, std, group_mean, group_std).copy()
    with np.errstate(invalid="ignore"):
        keep = np.ones(l.shape, dtype=bool) if math.isnan(truth_min) else (l > F32(truth_min))
        l[np.abs(l) < F32(min_s)] = F32(0.0)
        keep &= ~np.isnan(l) if math.isnan(null_val) else (l != F32(null_val))
    return np.where(keep[None], MC.score_terms(xs, l, probs), 0.0)


def score_sums_nodes(samples, y, probs, start=None, **kw):
    """((out, N, 5 + levels) sums, the same of the terms' magnitudes: the scale of the terms' own rounding noise)"""
    terms = score_terms_nodes(samples, y, probs, **kw)
    return accumulate(terms, start), accumulate(np.abs(terms))
