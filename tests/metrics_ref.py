"""numpy reference of the loss / metric epilogue (include/matgcn.h: "loss / metric epilogue" and "the evaluator's metric
table"; semantics as oracle/matgcn_oracle.py restates the reference's loss.py and traffic_state_evaluator.py).

Element-wise arithmetic runs in ``dtype`` - float32 like the kernels' (every operation one numpy operation, hence one
rounding), or float64 for the comparison with the two-pass oracle; every sum is float64.

Also the generator of the grid-valued ("exact") inputs of tests/test_loss_metrics_{host,edges}.py and the check of what
makes them exact: every value a small multiple of a power of two, so that no float32 operation on them rounds."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
METRIC_SUMS = 14
METRICS = 10


# ---- geometry -------------------------------------------------------------------------------------------------------
def label_rows(y, out, y_start, od, label_start=None):
    """(B, out, N, od) raw labels: channels y_start .. y_start+od-1 of the first ``out`` rows of the windows
    (B, y_steps, N, F), or - with label_start (B) - rows label_start[b] + o of the series (T, N, F), a row outside the
    series clamped to its first / last row (matgcn_series_violations counts those)."""
    y = np.asarray(y)
    if label_start is None:
        return y[:, :out, :, y_start:y_start + od]
    rows = np.asarray(label_start, dtype=np.int64)[:, None] + np.arange(out, dtype=np.int64)[None]
    return y[np.clip(rows, 0, y.shape[0] - 1)][..., y_start:y_start + od]


def affine(x, mean, std, dtype=F32):
    """x*std + mean in ``dtype``: a product, then a sum; mean / std scalars or one pair per node (axis 2)"""
    mean, std = np.asarray(mean, dtype=dtype).reshape(-1), np.asarray(std, dtype=dtype).reshape(-1)
    shape = (1, 1, -1, 1)
    t = np.asarray(x, dtype=dtype) * std.reshape(shape)
    return t + mean.reshape(shape)


def _nan0(a):
    return np.where(np.isnan(a), 0.0, a)


# ---- loss -----------------------------------------------------------------------------------------------------------
def mae_elements(pred, y, y_start, mean, std, null_val, min_s, label_start=None, dtype=F32):
    """(l, p, mask) of every element: l = y*std + mean, p = pred*std + mean; l := 0 where |l| < min_s;
    mask = l != null_val (NaN null value: not isnan(l))"""
    pred = np.asarray(pred)
    _, out, _, od = pred.shape
    l = affine(label_rows(y, out, y_start, od, label_start), mean, std, dtype).copy()
    p = affine(pred, mean, std, dtype)
    with np.errstate(invalid="ignore"):
        l[np.abs(l) < dtype(min_s)] = dtype(0.0)
        mask = ~np.isnan(l) if math.isnan(null_val) else (l != dtype(null_val))
    return l, p, mask


def mae_ref(pred, y, y_start, mean, std, null_val, min_s, label_start=None, dtype=F32):
    """((1 + out,) float64 [sum(|p-l|*mask) / sum(mask) over all horizons, then per horizon], sum(mask)); NaN terms
    count as 0, a ratio without an unmasked label is 0"""
    l, p, mask = mae_elements(pred, y, y_start, mean, std, null_val, min_s, label_start, dtype)
    with np.errstate(invalid="ignore"):
        term = np.where(mask, _nan0(np.abs(p - l)), 0).astype(F64)
    sa, sc = term.sum(axis=(0, 2, 3)), mask.sum(axis=(0, 2, 3)).astype(F64)
    sa, sc = np.concatenate([[sa.sum()], sa]), np.concatenate([[sc.sum()], sc])
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(sc > 0, sa / sc, 0.0), int(sc[0])


def mae_grad_ref(pred, y, y_start, mean, std, null_val, min_s, upstream=1.0, label_start=None, dtype=F32):
    """d result[0] / d pred = upstream * std * sign(p - l) * mask / sum(mask) in ``dtype`` (sign(NaN) = 0); all zeros
    when nothing is unmasked"""
    l, p, mask = mae_elements(pred, y, y_start, mean, std, null_val, min_s, label_start, dtype)
    count = int(mask.sum())
    if count == 0:
        return np.zeros(p.shape, dtype=dtype)
    with np.errstate(invalid="ignore"):
        d = p - l
        sgn = np.where(d > 0, dtype(1), np.where(d < 0, dtype(-1), dtype(0))).astype(dtype)
    g = (dtype(upstream) * dtype(std)) * sgn * mask.astype(dtype) / dtype(count)
    assert g.dtype == dtype
    return g


# ---- the evaluator's sums and table ------------------------------------------------------------------------------------
def metric_elements(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s, label_start=None,
                    dtype=F32):
    """(l, p, keep): first affine (None = identity), second per-node affine, p := clamp_min where p < clamp_min,
    keep = l > truth_min, l := 0 where |l| < min_s (min_s < 0: off) - in this order; NaN switches clamp / selection off"""
    pred = np.asarray(pred)
    _, out, _, od = pred.shape
    l, p = np.asarray(label_rows(y, out, y_start, od, label_start), dtype=dtype), pred.astype(dtype)
    if mean is not None:
        l, p = affine(l, mean, std, dtype), affine(p, mean, std, dtype)
    if group_mean is not None:
        l, p = affine(l, group_mean, group_std, dtype), affine(p, group_mean, group_std, dtype)
    l, p = l.copy(), p.copy()
    with np.errstate(invalid="ignore"):
        if not math.isnan(clamp_min):
            p[p < dtype(clamp_min)] = dtype(clamp_min)
        keep = np.ones(l.shape, dtype=bool) if math.isnan(truth_min) else (l > dtype(truth_min))
        if min_s >= 0:
            l[np.abs(l) < dtype(min_s)] = dtype(0.0)
    return l, p, keep


def metric_sums_ref(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s, label_start=None,
                    dtype=F32):
    """(out, 14) float64 per-horizon sums over the kept elements: 0 elements, 1 non-NaN labels, 2 sum|d|, 3 sum d^2,
    4 sum|d/l| over those (NaN terms -> 0), 5 labels != 0 (a NaN label is one), 6-8 the same three over those, 9 sum l,
    10 sum l^2, 11 sum p, 12 sum p^2, 13 sum(l - p); d = p - l, d^2 and d/l in ``dtype``, 9-13 from the float64 values"""
    l, p, keep = metric_elements(pred, y, y_start, mean, std, group_mean, group_std, clamp_min, truth_min, min_s,
                                 label_start, dtype)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = p - l
        ad, sq, ap = np.abs(d), d * d, np.abs(d / l)
        assert ad.dtype == dtype and sq.dtype == dtype and ap.dtype == dtype
        valid, nz = keep & ~np.isnan(l), keep & (l != 0)
        l64, p64 = l.astype(F64), p.astype(F64)
        terms = [keep, valid]
        terms += [np.where(valid, _nan0(t.astype(F64)), 0.0) for t in (ad, sq, ap)]
        terms += [nz]
        terms += [np.where(nz, _nan0(t.astype(F64)), 0.0) for t in (ad, sq, ap)]
        terms += [np.where(keep, t, 0.0) for t in (l64, l64 * l64, p64, p64 * p64, l64 - p64)]
        return np.stack([np.asarray(t, dtype=F64).sum(axis=(0, 2, 3)) for t in terms], 1)


def metric_table_ref(sums, swap_r2=False):
    """(2, out, 10) float64: [0] "single" mode (horizon o alone), [1] "average" mode (horizons 0..o); columns MAE, MAPE,
    MSE, RMSE over the non-NaN labels, the same four over the labels != 0 (a ratio over nothing is 0), R2 = 1 -
    sum d^2 / sum (t - mean t)^2 and EVAR = 1 - Var(t - p) / Var(t) with sklearn's conventions for a constant truth
    (1 where the numerator is 0 too, else 0); swap_r2: prediction takes the place of the truth in those two."""
    sums = np.asarray(sums, dtype=F64)
    table = np.empty((2,) + (sums.shape[0], METRICS), dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for mode, s in enumerate((sums, np.cumsum(sums, axis=0))):
            s = s.T
            t = table[mode].T
            for c, (num, den) in enumerate(((2, 1), (4, 1), (3, 1), (None, 1), (6, 5), (8, 5), (7, 5), (None, 5))):
                t[c] = np.sqrt(t[c - 1]) if num is None else np.where(s[den] > 0, s[num] / s[den], 0.0)
            n, res = s[0], s[3]
            s1, s2 = (s[11], s[12]) if swap_r2 else (s[9], s[10])
            ss_tot = np.where(n > 0, s2 - s1 * s1 / n, 0.0)
            var_d = np.where(n > 0, res / n - (s[13] / n) * (s[13] / n), 0.0)
            var_t = np.where(n > 0, ss_tot / n, 0.0)
            t[8] = np.where(ss_tot != 0, 1.0 - res / ss_tot, np.where(res == 0, 1.0, 0.0))
            t[9] = np.where(var_t != 0, 1.0 - var_d / var_t, np.where(var_d == 0, 1.0, 0.0))
    return table


def table_conditioning(sums, swap_r2=False):
    """((2, out) s2 / ssTot, (2, out) (res / n) / varD): by how much the two one-pass differences of metric_table_ref
    magnify a relative rounding error of their operands; inf where the difference is 0, NaN where the sums are"""
    sums = np.asarray(sums, dtype=F64)
    cond = np.empty((2, 2, sums.shape[0]), dtype=F64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for mode, s in enumerate((sums, np.cumsum(sums, axis=0))):
            s = s.T
            n, res = s[0], s[3]
            s1, s2 = (s[11], s[12]) if swap_r2 else (s[9], s[10])
            cond[0, mode] = np.abs(s2 / (s2 - s1 * s1 / n))
            cond[1, mode] = np.abs((res / n) / (res / n - (s[13] / n) * (s[13] / n)))
    return cond[0], cond[1]


# ---- grid-valued inputs ---------------------------------------------------------------------------------------------------
# Raw labels: multiples of 1/16 in [-4, 4]; prediction = label + a multiple of 1/16 in [-1, 1]; the scaler's std 1 or 2 and
# its mean an integer in [-2, 2] (a scalar, or one pair per node); group std 0.5, 1 or 2, group mean an integer in [-2, 2].
# Then l, p, p - l, |p - l| and (p - l)^2 are multiples of 2^-10 far below 2^24 of them: exact in float32, fused or not,
# and every float64 sum of them is exact in any order.
EXACT_MIN_S, EXACT_TRUTH_MIN, EXACT_CLAMP_MIN = 0.125, 1.0, 0.0


def grid_case(seed, b, out, n, od, y_steps=None, y_feat=None, y_start=0, per_node=False, group=False):
    """dict: y (B, y_steps, N, y_feat), pred (B, out, N, od) float32, mean / std (python floats, or float32 (N,) with
    per_node), group_mean / group_std (float32 (N,), or None).  The channels and rows of y that are no labels hold values
    of the same kind, so that reading the wrong one shows."""
    rng = np.random.default_rng(seed)
    y_steps = out if y_steps is None else y_steps
    y_feat = y_start + od if y_feat is None else y_feat
    y = (rng.integers(-64, 65, (b, y_steps, n, y_feat)) / 16.0).astype(F32)
    pred = (y[:, :out, :, y_start:y_start + od] + rng.integers(-16, 17, (b, out, n, od)) / 16.0).astype(F32)
    if per_node:
        mean, std = rng.integers(-2, 3, n).astype(F32), rng.choice([1.0, 2.0], n).astype(F32)
    else:
        mean, std = float(rng.integers(-2, 3)), float(rng.choice([1.0, 2.0]))
    c = dict(y=y, pred=pred, y_start=y_start, mean=mean, std=std, group_mean=None, group_std=None)
    if group:
        c["group_mean"], c["group_std"] = rng.integers(-2, 3, n).astype(F32), rng.choice([0.5, 1.0, 2.0], n).astype(F32)
    return c


def exact_report(c, group=None, label_start=None, step=2.0 ** -5, clamp_min=float("nan"), min_s=-1.0):
    """What makes case ``c`` exact, checked on the reference alone: the float32 and float64 element values (l, p, d,
    |d|, d^2) are equal, l, p, d are multiples of ``step`` (d^2 of its square), and a whole slab's sum of |d| stays below
    2^24 steps (the float32 sums of the loss kernel).  Returns dict(max_l, max_d, equal, slab_steps); NaN / inf elements
    are left out of the maxima and compared as such."""
    pred = c["pred"]
    gm, gs = (c["group_mean"], c["group_std"]) if (c["group_mean"] is not None if group is None else group) else (None, None)
    vals = {}
    for dtype in (F32, F64):
        l, p, _ = metric_elements(pred, c["y"], c["y_start"], c["mean"], c["std"], gm, gs, clamp_min, float("nan"), min_s,
                                  label_start, dtype)
        with np.errstate(invalid="ignore"):
            d = p - l
            vals[dtype] = [l, p, d, np.abs(d), d * d]
    equal = all(np.array_equal(a.astype(F64), b, equal_nan=True) for a, b in zip(vals[F32], vals[F64]))
    l, _, d = vals[F64][0], vals[F64][1], vals[F64][2]
    fin = np.isfinite(l) & np.isfinite(d)
    on_grid = all(bool((np.mod(v[np.isfinite(v)] / q, 1.0) == 0).all())
                  for v, q in zip(vals[F64], (step, step, step, step, step * step)))
    max_l, max_d = float(np.abs(l[fin]).max(initial=0.0)), float(np.abs(d[fin]).max(initial=0.0))
    slab = pred.shape[2] * pred.shape[3]
    return dict(max_l=max_l, max_d=max_d, equal=bool(equal and on_grid), slab_steps=slab * max_d / step)


def assert_exact(c, **kw):
    r = exact_report(c, **kw)
    assert r["equal"], "float32 and float64 element values differ, or leave the grid: %r" % (r,)
    assert r["slab_steps"] < 2.0 ** 24, r
    return r
