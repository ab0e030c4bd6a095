"""numpy statement of the executor's eleven differentiable training objectives and their gradients (include/matgcn.h:
"the executor's training objectives"), in float64 unless asked otherwise.

An objective is a name of ``LOSSES`` -> (family, null value, default delta).  With l = y*std + mean, p = pred*std + mean
(a product, then a sum, in ``dtype``) and d = p - l:

  masked families (mae, mse, rmse, mape and the masked_* names): l := 0 where |l| < MIN_S; an element takes part when its
  label differs from the null value (null value NaN: when it is no NaN).  value = sum of the terms taking part / their
  number; a NaN term adds 0 (and still counts) and has no gradient; nothing taking part gives 0.  rmse is the square root
  of that mean of squares, and where it is 0 every gradient is 0.
  plain means (logcosh, huber, quantile): the mean over every element, NaN included.

Every sum is a float64 numpy sum.  ``grad`` is d value / d pred (the scaled prediction): upstream * std * g / count."""
import math

import numpy as np

import metrics_ref as R

F32, F64 = np.float32, np.float64
NAN = float("nan")
MIN_S = float(np.float32(1e-4))
MASKED = ("mae", "mse", "rmse", "mape")
LOSSES = {
    "mae": ("mae", NAN, 0.0), "mse": ("mse", NAN, 0.0), "rmse": ("rmse", NAN, 0.0), "mape": ("mape", NAN, 0.0),
    "logcosh": ("logcosh", NAN, 0.0), "huber": ("huber", NAN, 1.0), "quantile": ("quantile", NAN, 0.25),
    "masked_mae": ("mae", 0.0, 0.0), "masked_mse": ("mse", 0.0, 0.0), "masked_rmse": ("rmse", 0.0, 0.0),
    "masked_mape": ("mape", 0.0, 0.0),
}


def elements(name, pred, y, y_start, mean, std, label_start=None, dtype=F64):
    """(l, p, d, part) of every element of ``pred`` (B, out, N, od); part: which elements take part in the mean"""
    family, null_val, _ = LOSSES[name]
    pred = np.asarray(pred)
    _, out, _, od = pred.shape
    l = R.affine(R.label_rows(y, out, y_start, od, label_start), mean, std, dtype).copy()
    p = R.affine(pred, mean, std, dtype)
    part = np.ones(l.shape, dtype=bool)
    with np.errstate(invalid="ignore"):
        if family in MASKED:
            l[np.abs(l) < dtype(MIN_S)] = dtype(0.0)
            part = ~np.isnan(l) if math.isnan(null_val) else (l != dtype(null_val))
        d = p - l
    return l, p, d, part


def term_and_slope(family, l, p, d, delta, dtype=F64):
    """(t, g): the term of every element and dt/dp, one numpy operation per arithmetic step, in ``dtype``"""
    one, half, two = dtype(1.0), dtype(0.5), dtype(2.0)
    delta = dtype(delta)
    with np.errstate(all="ignore"):
        sgn = np.where(d > 0, one, np.where(d < 0, -one, dtype(0.0))).astype(dtype)
        a = np.abs(d)
        if family == "mae":
            t, g = a, sgn
        elif family in ("mse", "rmse"):
            t, g = d * d, two * d
        elif family == "mape":
            t, g = np.abs(d / l), sgn / np.abs(l)
        elif family == "logcosh":
            t, g = a + np.log1p(np.exp(-two * a)) - dtype(math.log(2.0)), np.tanh(d)
        elif family == "huber":
            t = np.where(a <= delta, half * a * a, delta * a - half * delta * delta)
            g = np.where(a <= delta, d, delta * sgn)
        elif family == "quantile":
            t = np.where(l >= p, delta * (l - p), (one - delta) * (p - l))
            g = np.where(l >= p, -delta, one - delta) + dtype(0.0) * d
        else:
            raise KeyError(family)
    return t.astype(dtype), g.astype(dtype)


def train_loss_ref(name, pred, y, y_start, mean, std, delta=None, label_start=None, upstream=1.0, dtype=F64):
    """dict: value (the objective over all horizons), horizons (out,), grad (B, out, N, od) = d value / d pred, count.
    Element arithmetic in ``dtype``; sums, quotients and the square root in float64."""
    family, _, default_delta = LOSSES[name]
    delta = default_delta if delta is None else delta
    l, p, d, part = elements(name, pred, y, y_start, mean, std, label_start, dtype)
    t, g = term_and_slope(family, l, p, d, delta, dtype)
    t, g = t.astype(F64), g.astype(F64)
    if family in MASKED:
        live = part & ~np.isnan(t)
        t, g = np.where(live, t, 0.0), np.where(live, g, 0.0)
        cnt_h = part.sum(axis=(0, 2, 3)).astype(F64)
    else:
        cnt_h = np.full(t.shape[1], t.shape[0] * t.shape[2] * t.shape[3], dtype=F64)
    sum_h = t.sum(axis=(0, 2, 3))
    sums, cnts = np.concatenate([[sum_h.sum()], sum_h]), np.concatenate([[cnt_h.sum()], cnt_h])
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = np.where(cnts > 0, sums / cnts, 0.0)
        if family == "rmse":
            vals = np.sqrt(vals)
            g = g / (2.0 * vals[0]) if vals[0] > 0 else np.zeros_like(g)
        grad = (float(upstream) * float(std)) * g / cnts[0] if cnts[0] > 0 else np.zeros_like(g)
    return dict(value=float(vals[0]), horizons=vals[1:], grad=grad, count=int(cnts[0]))


# ---- the same objectives in torch, in the order of operations of the reference's loss.py -----------------------------------
def torch_loss(name, p, l, delta=None):
    """The executor's closure arithmetic on de-scaled torch tensors ``p`` (may require grad) and ``l`` - what a float32
    torch run of the reference computes, operation by operation (mask as a float32 tensor divided by its mean, NaN
    products replaced by 0, torch.mean): the yardstick of the realistic tests and the route the timing tool compares with.
    ``l`` is not modified."""
    import torch
    family, null_val, default_delta = LOSSES[name]
    delta = default_delta if delta is None else delta
    if family == "logcosh":
        return torch.mean(torch.log(torch.cosh(p - l)))
    if family == "huber":
        a = torch.abs(p - l)
        return torch.mean(torch.where(a <= delta, 0.5 * torch.square(a), delta * a - 0.5 * delta * delta))
    if family == "quantile":
        return torch.mean(torch.where(l >= p, delta * (l - p), (1 - delta) * (p - l)))
    l = torch.where(torch.abs(l) < 1e-4, torch.zeros_like(l), l)
    mask = (~torch.isnan(l) if math.isnan(null_val) else l.ne(null_val)).float()
    mask = mask / torch.mean(mask)
    mask = torch.where(torch.isnan(mask), torch.zeros_like(mask), mask)
    if family == "mae":
        t = torch.abs(p - l)
    elif family == "mape":
        t = torch.abs((p - l) / l)
    else:
        t = torch.square(p - l)
    t = t * mask
    v = torch.mean(torch.where(torch.isnan(t), torch.zeros_like(t), t))
    return torch.sqrt(v) if family == "rmse" else v


def torch_closure(name, pred, y, mean, std, dtype, delta=None):
    """(value, d value / d pred) as numpy, of torch_loss on CPU in ``dtype`` after x*std + mean on prediction and label"""
    import torch
    p = torch.tensor(np.asarray(pred), dtype=dtype, requires_grad=True)
    v = torch_loss(name, p * std + mean, torch.tensor(np.asarray(y), dtype=dtype) * std + mean, delta)
    v.backward()
    return v.detach().numpy(), p.grad.numpy()


# ---- grid-valued inputs --------------------------------------------------------------------------------------------------
def grid_case(seed, b, out, n, od, **kw):
    """metrics_ref.grid_case: labels multiples of 1/16 in [-4, 4], prediction = label + a multiple of 1/16 in [-1, 1],
    std 1 or 2, integer mean.  l, p and d are then multiples of 2^-4 below 2^4, d^2 and huber's 0.5 d^2 multiples of 2^-9,
    quantile's 0.25 / 0.75 |d| multiples of 2^-6: no float32 operation rounds, and a float64 sum of 2^31 of them is
    exact in any order."""
    return R.grid_case(seed, b, out, n, od, **kw)


def assert_exact(name, c, delta=None, label_start=None):
    """the condition of the bit-exact tests, on the reference alone: every element value (l, p, d, term; the slope too,
    except mape's quotients) is the same number in float32 and in float64 arithmetic, and the sum of all terms, counted
    in units of the smallest term step 2^-9, stays far below 2^53"""
    family, _, default_delta = LOSSES[name]
    delta = default_delta if delta is None else delta
    vals = {}
    for dtype in (F32, F64):
        l, p, d, part = elements(name, c["pred"], c["y"], c["y_start"], c["mean"], c["std"], label_start, dtype)
        t, g = term_and_slope(family, l, p, d, delta, dtype)
        vals[dtype] = [l, p, d, part] + ([] if family == "mape" else [t, g])
    for a32, a64 in zip(vals[F32], vals[F64]):
        assert a32.dtype in (F32, bool), a32.dtype
        assert np.array_equal(a32.astype(F64), a64.astype(F64), equal_nan=True), "a float32 operation rounds: %s" % name
    if family != "mape":
        t = vals[F64][4]
        fin = np.isfinite(t)
        assert bool((np.mod(t[fin] * 512.0, 1.0) == 0).all()), "terms leave the 2^-9 grid"
        assert float(np.abs(t[fin]).sum()) * 512.0 < 2.0 ** 50
