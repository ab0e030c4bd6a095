"""numpy reference of matgcn_mc_conformity / matgcn_conformal_quantile / matgcn_conformal_coverage (include/matgcn.h).
Sorting, quantiles and the descriptor's affines come from mc_scores_ref / node_metrics_ref; what is added here is the score
s = max(Q_first - l, l - Q_last) - two float32 differences, each one numpy float32 operation, hence one rounding -, NaN at
masked or filtered labels, and the rank rule: per group the k-th smallest valid score, k = max(1, ceil((n + 1) *
coverage)) with the product in float64, +inf where k > n."""
import math

import numpy as np

import mc_scores_ref as MC
import node_metrics_ref as R

F32, F64 = np.float32, np.float64
NAN = float("nan")


def coverage_of(probs):
    """(double)q_last - (double)q_first of the float32 levels: what the Python layer hands to the library"""
    return float(F32(probs[-1])) - float(F32(probs[0]))


def scores_from_band(q_first, l, q_last, keep):
    """float32 scores from float32 band edges and labels; NaN where not ``keep``"""
    q_first, l, q_last = (np.asarray(v, dtype=F32) for v in (q_first, l, q_last))
    with np.errstate(invalid="ignore"):
        below = q_first - l
        above = l - q_last
        s = np.maximum(below, above)
    assert below.dtype == F32 and above.dtype == F32 and s.dtype == F32
    return np.where(keep, s, F32(NAN)).astype(F32)


def labels_nodes(y, mean=None, std=None, group_mean=None, group_std=None, truth_min=NAN, null_val=0.0, min_s=1e-4):
    """(l float32, keep) of the raw labels y (..., N, od): de-scaled, l <= truth_min left out (tested before |l| < min_s ->
    0), masked where l == null_val (NaN: where NaN) - the rules of node_metrics_ref.score_terms_nodes"""
    l = R.descale_nodes(y, mean, std, group_mean, group_std).copy()
    with np.errstate(invalid="ignore"):
        keep = np.ones(l.shape, dtype=bool) if math.isnan(truth_min) else (l > F32(truth_min))
        l[np.abs(l) < F32(min_s)] = F32(0.0)
        keep &= ~np.isnan(l) if math.isnan(null_val) else (l != F32(null_val))
    return l, keep


def conformity(samples, y, probs, mean=None, std=None, group_mean=None, group_std=None, clamp_min=NAN, truth_min=NAN,
               null_val=0.0, min_s=1e-4):
    """samples (S, B, out, N, od), y the raw labels (B, out, N, od) -> (B, out, N, od) float32 scores"""
    xs = R.sorted_samples_nodes(samples, mean, std, group_mean, group_std, clamp_min)
    q = MC.quantiles_sorted(xs, (probs[0], probs[-1]))
    l, keep = labels_nodes(y, mean, std, group_mean, group_std, truth_min, null_val, min_s)
    return scores_from_band(q[0], l, q[1], keep)


def rank(n, coverage):
    return max(1, int(math.ceil(F64(n + 1) * F64(coverage))))


def ranks(n, coverage):
    """``rank`` of every entry of an integer array: the same float64 product and ceil"""
    k = np.ceil((np.asarray(n).astype(F64) + F64(1.0)) * F64(coverage))
    return np.maximum(k, 1.0).astype(np.int64)


def _groups(scores, rows, grouping):
    """the store's first ``rows`` rows as (groups, members): per horizon, or per (horizon, column)"""
    s = np.asarray(scores, dtype=F32)[:rows]
    out = s.shape[1]
    s = s.reshape(rows, out, -1)
    if grouping in (0, "horizon"):
        return np.moveaxis(s, 1, 0).reshape(out, -1), (out,)
    return np.moveaxis(s, 0, -1).reshape(-1, rows), tuple(np.asarray(scores).shape[1:])


def quantile_many(scores, rows, grouping, coverages):
    """[(margin float32, count int32) for every coverage] per group of a store (capacity, out, ...).  np.sort puts NaN
    behind every number, so the first n entries of a sorted group are np.sort(valid) and entry k - 1 its k-th smallest."""
    groups, shape = _groups(scores, rows, grouping)
    ordered = np.sort(groups, axis=1)
    count = (~np.isnan(groups)).sum(1).astype(np.int32)
    result = []
    for coverage in coverages:
        k = ranks(count, coverage)
        picked = ordered[np.arange(len(groups)), np.minimum(k, groups.shape[1]) - 1]
        margin = np.where(k <= count, picked, F32(np.inf)).astype(F32)
        result.append((margin.reshape(shape), count.reshape(shape).copy()))
    return result


def quantile(scores, rows, grouping, coverage):
    """(margin float32, count int32) per group of a store (capacity, out, ...)"""
    return quantile_many(scores, rows, grouping, (coverage,))[0]


def coverage_counts(scores, rows, grouping, margin):
    """(*group shape, 2) int64: [valid scores, valid scores <= margin] per group"""
    groups, shape = _groups(scores, rows, grouping)
    m = np.asarray(margin, dtype=F32).reshape(-1)
    with np.errstate(invalid="ignore"):
        n = (~np.isnan(groups)).sum(1)
        covered = (groups <= m[:, None]).sum(1)
    return np.stack([n, covered], -1).astype(np.int64).reshape(shape + (2,))


def apply_margin(quantiles, margin, grouping, clamp_min=NAN):
    """the band (levels, B, out, N, od) float32 with its outer levels moved by the margin, then held at the clamp"""
    q = np.array(quantiles, dtype=F32)
    m = np.asarray(margin, dtype=F32)
    m = m.reshape(-1, 1, 1) if grouping in (0, "horizon") else m
    with np.errstate(invalid="ignore"):
        q[0] = q[0] - m
        q[-1] = q[-1] + m
    if not math.isnan(clamp_min):
        q[0] = np.maximum(q[0], F32(clamp_min))
        q[-1] = np.maximum(q[-1], F32(clamp_min))
    return q
