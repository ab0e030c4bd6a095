"""tests/metrics_ref.py pinned before it judges a kernel (tests/test_loss_metrics_edges.py): against the tables the
reference's own evaluator produced (tests/golden/metrics_small.npz), against the two-pass float64 oracle on random
inputs, against the oracle's masked MAE and float64 autograd through it - and the preconditions of the grid-valued
("exact") inputs, once per generator setting.  No GPU."""
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from helpers import GOLDEN_DIR
from oracle import matgcn_oracle as O

GOLD = np.load(os.path.join(GOLDEN_DIR, "metrics_small.npz"))
NAN = float("nan")
GROUP_COLS = [O.EVAL_METRICS.index(k) for k in ("MAE", "MSE", "RMSE", "R2", "EVAR", "MAPE")]


def _close(got, want, rtol, atol):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same_inf = np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want))
    with np.errstate(invalid="ignore"):
        ok = same_inf | (np.abs(got - want) <= rtol * np.abs(want) + atol)
    return bool(ok.all()), np.argwhere(~ok)[:5].tolist()


def _oracle_table(p, t, mode, min_s=1e-4):
    d = O.evaluator_table(torch.from_numpy(p), torch.from_numpy(t), mode, min_s)
    return np.array([[d["%s@%d" % (m, i + 1)] for m in O.EVAL_METRICS] for i in range(p.shape[1])], dtype=np.float64)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_reproduces_the_golden_evaluator_tables(tag):
    """float32 element arithmetic, as the reference's tensors; the file's tolerance (test_metrics.py)"""
    scaled = tag + "_std" in GOLD
    mean, std = (float(GOLD[tag + "_mean"]), float(GOLD[tag + "_std"])) if scaled else (None, None)
    sums = R.metric_sums_ref(GOLD[tag + "_pred"], GOLD[tag + "_true"], 0, mean, std, None, None, NAN, NAN, 1e-4)
    table = R.metric_table_ref(sums)
    for mode, name in enumerate(("single", "average")):
        ok, where = _close(table[mode], GOLD["%s_%s" % (tag, name)], 2e-5, 1e-9)
        assert ok, (name, where)
    if tag == "a":
        assert np.isinf(table[0][:, 1]).any() and np.isfinite(table[0][:, 5]).all()


def test_reference_reproduces_the_golden_groupstd_table():
    sums = R.metric_sums_ref(GOLD["c_pred"], GOLD["c_true"], 0, None, None, GOLD["c_all_m"], GOLD["c_all_std"], 0.0, 10.0, -1.0)
    ok, where = _close(R.metric_table_ref(sums, swap_r2=True)[0][:, GROUP_COLS], GOLD["c_table"], 2e-5, 1e-9)
    assert ok, where


def _random64(seed, b, out, n, od, y_feat, y_start):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, out + 1, n, y_feat))
    pred = y[:, :out, :, y_start:y_start + od] + 0.3 * rng.standard_normal((b, out, n, od))
    y[0, :, :2, y_start] = 0.0                        # exact zeros: inf MAPE, masked under null value 0
    y[1, 1, 3, y_start] = 5e-5                        # below min_s
    pred[1, 2, 4, 0] = y[1, 2, 4, y_start]            # p == l
    return pred, y


@pytest.mark.parametrize("shape", [(4, 5, 23, 1, 1, 0), (3, 7, 19, 2, 4, 1)])
def test_reference_agrees_with_the_two_pass_oracle_in_float64(shape):
    b, out, n, od, y_feat, y_start = shape
    pred, y = _random64(17, *shape)
    rng = np.random.default_rng(5)
    mean, std = rng.uniform(-1, 1, n), rng.uniform(0.5, 2.0, n)
    sums = R.metric_sums_ref(pred, y, y_start, mean, std, None, None, NAN, NAN, 1e-4, dtype=R.F64)
    table = R.metric_table_ref(sums)
    p = R.affine(pred, mean, std, R.F64)
    t = R.affine(y[:, :out, :, y_start:y_start + od], mean, std, R.F64)
    for mode, name in enumerate(("single", "average")):
        ok, where = _close(table[mode], _oracle_table(p, t, name), 1e-9, 1e-9)
        assert ok, (name, where)
    all_m, all_std = rng.uniform(5.0, 60.0, n), rng.uniform(3.0, 40.0, n)
    sums = R.metric_sums_ref(pred, y, y_start, mean, std, all_m, all_std, 0.0, 10.0, -1.0, dtype=R.F64)
    cols = O.groupstd_table(torch.from_numpy(p), torch.from_numpy(t), all_m, all_std)
    want = np.stack([cols[k] for k in ("MAE", "MSE", "RMSE", "R2", "EVAR", "MAPE")], 1)
    ok, where = _close(R.metric_table_ref(sums, swap_r2=True)[0][:, GROUP_COLS], want, 1e-9, 1e-9)
    assert ok, where


@pytest.mark.parametrize("null_val", [0.0, NAN, 1.875])
def test_mae_reference_agrees_with_the_oracle_and_its_autograd(null_val):
    """loss and MAE@k to 1e-12; the closed-form gradient against float64 autograd through O.masked_mae to 1e-12 (finite
    predictions only: torch propagates 0 * sign(NaN), include/matgcn.h defines 0 there)"""
    out, y_start, od = 5, 1, 2
    pred, y = _random64(23, 4, out, 23, od, 4, y_start)
    mean, std, min_s = 0.75, 1.5, 1e-4
    y[0, :, :2, y_start] = -0.5                        # de-scales to exactly 0
    y[1, 1, 3, y_start] = (5e-5 - mean) / std          # below min_s after de-scaling
    y[2, 0, 5, y_start] = 0.75                         # de-scales to exactly 1.875, the third null value
    y[3, 1, 6, y_start + 1] = NAN                      # a NaN label: masked under the NaN mask, counted under 0 / 2
    got, count = R.mae_ref(pred, y, y_start, mean, std, null_val, min_s, dtype=R.F64)
    tp = (torch.from_numpy(pred) * std + mean).requires_grad_(True)
    tl = torch.from_numpy(y[:, :out, :, y_start:y_start + od]) * std + mean
    want = O.masked_mae(tp, tl, null_val, min_s)
    assert abs(got[0] - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
    for k in range(out):
        w = float(O.masked_mae(tp[:, k], tl[:, k], null_val, min_s))
        assert abs(got[1 + k] - w) <= 1e-12 * abs(w), k
    l, _, mask = R.mae_elements(pred, y, y_start, mean, std, null_val, min_s, dtype=R.F64)
    assert count == int(mask.sum()) and 0 < count < mask.size
    (want * 0.5).backward()
    grad = R.mae_grad_ref(pred, y, y_start, mean, std, null_val, min_s, upstream=0.5, dtype=R.F64)
    # d / d pred = std * d / d p
    assert np.abs(grad - tp.grad.numpy() * std).max() <= 1e-12 * np.abs(grad).max()
    assert (grad[~mask] == 0).all()


def test_all_masked_reference_is_zero():
    y = np.zeros((2, 3, 5, 1), dtype=np.float32)
    pred = np.ones((2, 3, 5, 1), dtype=np.float32)
    got, count = R.mae_ref(pred, y, 0, 0.0, 1.0, 0.0, 1e-4)
    assert count == 0 and (got == 0).all()
    assert (R.mae_grad_ref(pred, y, 0, 0.0, 1.0, 0.0, 1e-4, upstream=4.0) == 0).all()
    assert float(O.masked_mae(torch.from_numpy(pred), torch.from_numpy(y), 0.0)) == 0.0


def test_label_rows_gathers_and_clamps():
    series = np.arange(7 * 2 * 3, dtype=np.float32).reshape(7, 2, 3)
    got = R.label_rows(series, 3, 1, 2, label_start=[0, 4, 6, -1])
    assert np.array_equal(got[0], series[0:3, :, 1:3]) and np.array_equal(got[1], series[4:7, :, 1:3])
    assert np.array_equal(got[2], series[[6, 6, 6]][:, :, 1:3]) and np.array_equal(got[3], series[[0, 0, 1]][:, :, 1:3])


SETTINGS = {          # generator setting -> (grid_case arguments, largest |l| its ranges allow)
    "scalar": (dict(), 10.0),
    "per_node": (dict(per_node=True), 10.0),
    "scalar_group": (dict(group=True), 22.0),
    "per_node_group": (dict(per_node=True, group=True), 22.0),
}


@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_exact_group_preconditions(setting):
    """B = 65, N = 4096: float32 and float64 element values are equal and on the grid, a slab's |d| sum stays far below
    2^24 grid steps; float64 totals do not depend on the order, and a float32 running sum of a slab's |d| is exact."""
    kw, bound = SETTINGS[setting]
    c = R.grid_case(3, 65, 1, 4096, 1, **kw)
    R.assert_exact(c, clamp_min=R.EXACT_CLAMP_MIN, min_s=R.EXACT_MIN_S)     # the clamp and the zeroing stay on the grid
    r = R.assert_exact(c)
    print("%s: max|l| %g, max|d| %g, float32 == float64: %s, slab steps 2^%.1f" % (
        setting, r["max_l"], r["max_d"], r["equal"], np.log2(r["slab_steps"])))
    assert r["max_l"] <= bound and r["max_d"] <= 4.0
    l, p, _ = R.metric_elements(c["pred"], c["y"], 0, c["mean"], c["std"], c["group_mean"], c["group_std"], NAN, NAN, -1.0)
    ad = np.abs(p - l).reshape(-1)
    perm = np.random.default_rng(1).permutation(ad.size)
    total = float(ad.astype(np.float64).sum())
    assert float(ad[perm].astype(np.float64).sum()) == total
    assert float(sum(float(ad[k::256].astype(np.float64).sum()) for k in range(256))) == total
    slab = ad[:4096]
    assert float(np.cumsum(slab, dtype=np.float32)[-1]) == float(slab.astype(np.float64).sum())


def test_exact_group_preconditions_large_offset():
    """scaler mean 4096, std 1: outside the integer range of the generator, still exact"""
    c = R.grid_case(4, 3, 6, 257, 1)
    c["mean"], c["std"] = 4096.0, 1.0
    r = R.assert_exact(c, min_s=R.EXACT_MIN_S)
    print("offset 4096: max|l| %g, max|d| %g, float32 == float64: %s" % (r["max_l"], r["max_d"], r["equal"]))
    assert 4092.0 <= r["max_l"] <= 4100.0 and r["max_d"] <= 1.0
