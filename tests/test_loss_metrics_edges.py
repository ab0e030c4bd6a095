"""The loss / metric kernels (section 9 of csrc/matgcn_kernels.hip: k_mae_partial / k_mae_final, k_mae_grad,
k_metric_partial / k_metric_accumulate / k_metric_table) at their block, channel and mask edges, against the plain
numpy reference of tests/metrics_ref.py (pinned on the host by tests/test_loss_metrics_host.py).

Two groups of inputs.

EXACT: every value sits on a dyadic grid (metrics_ref.grid_case), so no float32 operation of the kernels rounds and
every float64 sum is exact in any order - each test asserts that on its own reference before it launches.  Then
  * sums 0-3, 5-7, 9-13 of matgcn_metric_sums are bit-equal to the reference; sums 4 and 8 add one float32 quotient of
    exact operands per term: |got - want| <= 2^-22 * want (a correctly rounded quotient is within 2^-24, the factor 4
    covers a division of up to 2.5 ulp), inf == inf where a zero label meets d != 0;
  * matgcn_masked_mae is bit-equal to float32(sum / count), in the total and per horizon;
  * matgcn_masked_mae_grad is within 1 float32 ulp of the closed form and exactly 0 where it is 0;
  * matgcn_metric_table against the reference's table of the same sums: 1e-12 relative in columns 0-7; R2 within
    1e-15 * s2 / ssTot and EVAR within 1e-15 * (s2 / ssTot + (res / n) / varD) - the one-pass differences s2 - s1^2 / n
    and res / n - (s13 / n)^2 magnify the float64 rounding of their operands by exactly these factors, and EVAR is a
    ratio of both differences -, exact where a difference is 0 (sklearn's constant-truth convention);
  * against the two-pass float64 oracle on the float64 de-scaled inputs: 1e-9 in every column whose sums are exact;
    the two MAPE columns carry the float32 quotients and get their 2^-22.
REALISTIC: continuous data under Baltimore's scaler with per-tract group statistics (tests/golden/
make_metrics_golden.py), held to the tolerances of the existing tests of these entry points: 2e-5 relative + 1e-9 per
table entry, 2e-6 relative for the loss and each MAE@k, 1e-6 max-normalised for the gradient with exact zeros at
masked elements.  The kernel may fuse its float32 de-scale where numpy does not, so no element is left within an ulp's
reach of a threshold (see _realistic)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import metrics_ref as R
from helpers import max_norm_err
from oracle import matgcn_oracle as O

pytestmark = pytest.mark.gpu

NAN = float("nan")
EXACT_COLS = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13]
QUOT_COLS = [4, 8]
QUOT_TOL = 2.0 ** -22
MAPE_COLS = [1, 5]
GROUP_KEYS = ("MAE", "MSE", "RMSE", "R2", "EVAR", "MAPE")
GROUP_COLS = [O.EVAL_METRICS.index(k) for k in GROUP_KEYS]
UPSTREAM = 4.0          # a power of two keeps upstream * std exact


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


# ---- shapes of the exact group -----------------------------------------------------------------------------------------
def _shape(b=3, out=6, n=257, od=1, y_steps=None, y_feat=None, y_start=0):
    return (b, out, n, od, out if y_steps is None else y_steps, y_start + od if y_feat is None else y_feat, y_start)


SHAPES = {"base": _shape()}
# N * od across the 256-thread block (the slab loop of k_mae_partial / k_metric_partial, the idx split of k_mae_grad)
for _n, _od in ((1, 1), (63, 1), (255, 1), (256, 1), (171, 3), (128, 2), (1039, 1)):
    SHAPES["n%d_od%d" % (_n, _od)] = _shape(n=_n, od=_od)      # B*out*N*od a multiple of 256 at N = 256 and (128, 2) only
SHAPES["n4096_b2"] = _shape(b=2, n=4096)
# channels: labels in the middle of the feature axis, at its end, and alone
SHAPES["od2_feat5_start2"] = _shape(od=2, y_feat=5, y_start=2)
SHAPES["od3_start1_last"] = _shape(od=3, y_feat=4, y_start=1)
SHAPES["od1_feat1"] = _shape(od=1, y_feat=1)
# horizons up to the limit of 64, label windows as long as the horizon and longer
for _out in (1, 24, 63, 64):
    SHAPES["out%d" % _out] = _shape(out=_out)
    SHAPES["out%d_steps%d" % (_out, _out + 2)] = _shape(out=_out, y_steps=_out + 2)
SHAPES["b1"] = _shape(b=1)
SHAPES["b65"] = _shape(b=65)
SHAPES["b65_out64_n171_od3"] = _shape(b=65, out=64, n=171, od=3, y_steps=66, y_feat=4, y_start=1)
SHAPE_IDS = list(SHAPES)


@functools.lru_cache(maxsize=None)
def _case(name, per_node=False, group=False):
    b, out, n, od, y_steps, y_feat, y_start = SHAPES[name]
    c = R.grid_case(SHAPE_IDS.index(name) + 1, b, out, n, od, y_steps, y_feat, y_start, per_node=per_node, group=group)
    R.assert_exact(c, clamp_min=R.EXACT_CLAMP_MIN, min_s=R.EXACT_MIN_S)
    return c


def _base(seed=101, **kw):
    """a fresh base-shape case the semantic tests plant values in; scalar scaler fixed by the caller"""
    return R.grid_case(seed, *SHAPES["base"][:4], **kw)


# ---- comparisons ----------------------------------------------------------------------------------------------------
def _same(a, b):
    """equal, NaN == NaN, inf == inf of the same sign"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _assert_sums(got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = np.argwhere(~_same(got[:, EXACT_COLS], want[:, EXACT_COLS]))
    assert bad.size == 0, ("exact sums differ at (horizon, index into EXACT_COLS)", bad[:5].tolist(),
                           got[bad[0][0]].tolist(), want[bad[0][0]].tolist())
    g, w = got[:, QUOT_COLS], want[:, QUOT_COLS]
    with np.errstate(invalid="ignore"):
        ok = _same(g, w) | (np.abs(g - w) <= QUOT_TOL * w)
    assert ok.all(), ("quotient sums", np.argwhere(~ok)[:5].tolist(), g[~ok][:5], w[~ok][:5])


def _assert_table(got, want, sums, swap, rtol=1e-12, mape_rtol=1e-12, mode=None):
    """device table against the reference's table of the same sums (module docstring); mode: (out, 10) tables of that
    mode alone"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    tol = np.zeros_like(want)
    tol[..., :8] = rtol * np.abs(want[..., :8])
    tol[..., MAPE_COLS] = mape_rtol * np.abs(want[..., MAPE_COLS])
    cond_t, cond_d = R.table_conditioning(sums, swap)
    cond_t, cond_d = (np.where(np.isfinite(c), c, 0.0) for c in (cond_t, cond_d))
    if mode is not None:
        cond_t, cond_d = cond_t[mode], cond_d[mode]
    tol[..., 8], tol[..., 9] = 1e-15 * cond_t, 1e-15 * (cond_t + cond_d)
    with np.errstate(invalid="ignore"):
        ok = _same(got, want) | (np.abs(got - want) <= np.where(np.isfinite(tol), tol, 0.0))
    assert ok.all(), ("table (mode, horizon, metric)", np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


def _assert_oracle(got, want, cond=None):
    """(out, 10) or (out, 6 group columns with ``cols``) against the two-pass oracle: 1e-9, the MAPE columns 2^-22
    relative, R2 / EVAR of an ill-conditioned case within ``cond`` = (out, 2) bounds instead"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    tol = 1e-9 * np.maximum(1.0, np.abs(want))
    tol[:, MAPE_COLS] = QUOT_TOL * np.abs(want[:, MAPE_COLS]) + 1e-9
    if cond is not None:
        tol[:, 8:10] = cond
    with np.errstate(invalid="ignore"):
        ok = _same(got, want) | (np.abs(got - want) <= np.where(np.isfinite(tol), tol, 0.0))
    assert ok.all(), ("oracle (horizon, metric)", np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


def _oracle_eval(p64, l64, mode, min_s):
    d = O.evaluator_table(torch.from_numpy(p64), torch.from_numpy(l64), mode, min_s)
    return np.array([[d["%s@%d" % (m, i + 1)] for m in O.EVAL_METRICS] for i in range(p64.shape[1])], dtype=np.float64)


def _oracle_group(p64, l64, gm, gs, s_small):
    """the oracle's re-transform table spread over the ten-metric layout (the columns it does not have: NaN)"""
    cols = O.groupstd_table(torch.from_numpy(p64), torch.from_numpy(l64), gm, gs, s_small)
    t = np.full((p64.shape[1], 10), NAN)
    for k, c in zip(GROUP_KEYS, GROUP_COLS):
        t[:, c] = cols[k]
    return t


def _descaled64(c, label_start=None):
    pred = c["pred"]
    lab = R.label_rows(c["y"], pred.shape[1], c["y_start"], pred.shape[3], label_start)
    return R.affine(pred, c["mean"], c["std"], R.F64), R.affine(lab, c["mean"], c["std"], R.F64)


ROUTES = {      # name -> (group affine, clamp_min, truth_min, min_s, swap_r2)
    "evaluator": (False, NAN, NAN, R.EXACT_MIN_S, False),
    "groupstd": (True, R.EXACT_CLAMP_MIN, R.EXACT_TRUTH_MIN, -1.0, True),
    "all": (True, R.EXACT_CLAMP_MIN, R.EXACT_TRUTH_MIN, R.EXACT_MIN_S, False),
}


def _sums_both(c, route, label_start=None, sums=None, ref=True):
    """(device sums, reference sums, swap_r2) of case c through ops.metric_sums"""
    from multistgraph_amd import ops
    group, clamp, truth, min_s, swap = ROUTES[route]
    gm, gs = (c["group_mean"], c["group_std"]) if group else (None, None)
    ls = None if label_start is None else _dev(np.asarray(label_start, dtype=np.int32))
    got = ops.metric_sums(_dev(c["pred"]), _dev(c["y"]), c["y_start"], c["mean"], c["std"], gm, gs, clamp_min=clamp,
                          truth_min=truth, min_s=min_s, label_start=ls, sums=sums)
    want = R.metric_sums_ref(c["pred"], c["y"], c["y_start"], c["mean"], c["std"], gm, gs, clamp, truth, min_s,
                             label_start) if ref else None
    return got, want, swap


def _check_route(c, route, label_start=None):
    from multistgraph_amd import ops
    got, want, swap = _sums_both(c, route, label_start)
    _assert_sums(_host(got), want)
    for sw in (swap, not swap):
        _assert_table(_host(ops.metric_table(got, swap_r2=sw)), R.metric_table_ref(_host(got), sw), _host(got), sw)
    return got, want


def _loss_both(c, null_val=0.0, min_s=R.EXACT_MIN_S, label_start=None):
    from multistgraph_amd import ops
    ls = None if label_start is None else _dev(np.asarray(label_start, dtype=np.int32))
    got = ops.masked_mae_device(_dev(c["pred"]), _dev(c["y"]), c["y_start"], c["mean"], c["std"], null_val, min_s, ls)
    want, count = R.mae_ref(c["pred"], c["y"], c["y_start"], c["mean"], c["std"], null_val, min_s, label_start)
    return _host(got), want, count


def _assert_loss_exact(c, **kw):
    got, want, count = _loss_both(c, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape
    print("loss %r reference %r count %d" % (got[0], want[0], count))
    assert np.array_equal(got, want.astype(np.float32)), (got, want.astype(np.float32))
    return got, want, count


def _grad_both(c, null_val=0.0, min_s=R.EXACT_MIN_S, label_start=None, upstream=UPSTREAM):
    from multistgraph_amd import ops
    ls = None if label_start is None else _dev(np.asarray(label_start, dtype=np.int32))
    p = _dev(c["pred"]).requires_grad_(True)
    loss = ops.masked_mae_loss(p, _dev(c["y"]), c["y_start"], c["mean"], c["std"], null_val, min_s, ls)
    (loss * upstream).backward()
    want = R.mae_grad_ref(c["pred"], c["y"], c["y_start"], c["mean"], c["std"], null_val, min_s, upstream, label_start)
    return _host(p.grad), want, float(loss.detach())


def _assert_grad_exact(c, **kw):
    got, want, loss = _grad_both(c, **kw)
    assert got.dtype == np.float32 and got.shape == want.shape and np.isfinite(got).all()
    zero = want == 0
    assert (got[zero] == 0).all(), "a gradient at a masked or p == l element"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("gradient: worst error %.3g ulp" % float((err / np.spacing(np.abs(want)).astype(np.float64))[~zero].max(initial=0.0)))
    assert (err <= np.spacing(np.abs(want))).all()
    return got, want, loss


def _violations(reset=1):
    from multistgraph_amd import _lib
    cnt = C.c_int64()
    _lib.check(_lib.load().matgcn_series_violations(C.byref(cnt), reset), "matgcn_series_violations")
    return int(cnt.value)


# ---- the exact group over the shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_exact_loss(name, lib_built):
    c = _case(name)
    got, want, count = _assert_loss_exact(c)
    assert 0 < count and (count < c["pred"].size or c["pred"].size < 1000)     # zero labels occur on the grid: the mask is at work
    again, _, _ = _loss_both(c)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("name", SHAPE_IDS)
def test_exact_gradient(name, lib_built):
    c = _case(name)
    got, want, loss = _assert_grad_exact(c)
    assert np.float32(loss) == np.float32(R.mae_ref(c["pred"], c["y"], c["y_start"], c["mean"], c["std"], 0.0, R.EXACT_MIN_S)[0][0])
    assert c["pred"].size < 1000 or ((want == 0).any() and (want > 0).any() and (want < 0).any())
    assert np.array_equal(got, _grad_both(c)[0])


@pytest.mark.parametrize("name", SHAPE_IDS)
def test_exact_metric_sums(name, lib_built):
    """all three routes of the kernel's element pipeline; scalar and per-node first affine alternate over the shapes"""
    c = _case(name, per_node=SHAPE_IDS.index(name) % 2 == 1, group=True)
    for route in ROUTES:
        got, _ = _check_route(c, route)
        assert torch.equal(got, _sums_both(c, route, ref=False)[0])


@pytest.mark.parametrize("route", ["single", "average", "groupstd"])
@pytest.mark.parametrize("name", SHAPE_IDS)
def test_exact_tables_match_the_two_pass_oracle(name, route, lib_built):
    from multistgraph_amd import ops
    c = _case(name, per_node=SHAPE_IDS.index(name) % 2 == 1, group=True)
    p64, l64 = _descaled64(c)
    if route == "groupstd":
        got, _, swap = _sums_both(c, "groupstd", ref=False)
        want = _oracle_group(p64, l64, c["group_mean"].astype(np.float64), c["group_std"].astype(np.float64), R.EXACT_TRUTH_MIN)
        have = _host(ops.metric_table(got, swap_r2=swap))[0]
        have[:, [k for k in range(10) if k not in GROUP_COLS]] = NAN
        empty = _host(got)[:, 0] == 0              # nothing kept at N = 1: the oracle's means over nothing are NaN,
        want[empty] = have[empty]                  # the device's table (checked against the reference's) says 0
    else:
        got, _, swap = _sums_both(c, "evaluator", ref=False)
        want = _oracle_eval(p64, l64, route, R.EXACT_MIN_S)
        have = _host(ops.metric_table(got, swap_r2=swap))[0 if route == "single" else 1]
    _assert_oracle(have, want)


# ---- semantic edges, exact group ------------------------------------------------------------------------------------------
def _scalar(c, mean, std):
    c["mean"], c["std"] = float(mean), float(std)
    return c


@pytest.mark.parametrize("null_val", [0.0, NAN, 2.0])
def test_null_values(null_val, lib_built):
    """null value 0, NaN (with NaN labels) and 2.0: loss, MAE@k and gradient.  A NaN label under null value 0 counts in
    the mask and contributes 0, as O.masked_mae has it."""
    c = _scalar(_base(), 1, 2)
    y = c["y"]
    y[0, 1, 10:20, 0] = NAN
    y[2, 3, 200:257, 0] = NAN
    y[1, 2, 5:9, 0] = 0.5                      # de-scales to exactly 2.0
    y[1, 4, 0, 0] = -0.5                       # and to exactly 0
    R.assert_exact(c, min_s=R.EXACT_MIN_S)
    l, _, mask = R.mae_elements(c["pred"], y, 0, 1.0, 2.0, null_val, R.EXACT_MIN_S)
    assert (l[1, 2, 5:9, 0] == 2.0).all() and l[1, 4, 0, 0] == 0.0
    assert mask[0, 1, 10:20, 0].all() != math.isnan(null_val)
    assert mask[1, 2, 5:9, 0].all() != (null_val == 2.0) and mask[1, 4, 0, 0] != (null_val == 0.0)
    got, want, count = _assert_loss_exact(c, null_val=null_val)
    _assert_grad_exact(c, null_val=null_val)
    tp, tl = torch.from_numpy(c["pred"]).double() * 2 + 1, torch.from_numpy(y).double() * 2 + 1
    assert abs(want[0] - float(O.masked_mae(tp, tl, null_val, R.EXACT_MIN_S))) <= 1e-12 * want[0]
    if null_val == 0.0:
        assert count == int((l != 0).sum()) and count > int((np.nan_to_num(l, nan=0.0) != 0).sum())


def test_min_s_boundary(lib_built):
    """labels that de-scale to exactly +-0.0625 are zeroed (and masked under null value 0), +-0.125 are kept - the test is
    `<` -, -0.0 is masked; the same in the metric sums, where sum 5 leaves the zeroed ones out"""
    c = _scalar(_base(), 0, 1)
    y, pred = c["y"], c["pred"]
    spots = {0.0625: (0, 0, 3), -0.0625: (0, 1, 255), 0.125: (1, 2, 256), -0.125: (1, 3, 0), -0.0: (2, 5, 100)}
    for v, (b, o, n) in spots.items():
        y[b, o, n, 0] = v
        pred[b, o, n, 0] = v + 0.5
    R.assert_exact(c, min_s=R.EXACT_MIN_S)
    l, _, mask = R.mae_elements(pred, y, 0, 0.0, 1.0, 0.0, R.EXACT_MIN_S)
    for v, at in spots.items():
        assert mask[at][0] == (abs(v) == 0.125) and l[at][0] == (v if abs(v) == 0.125 else 0.0)
    _assert_loss_exact(c)
    got, want, _ = _assert_grad_exact(c)
    for v, at in spots.items():
        assert (got[at][0] != 0) == (abs(v) == 0.125)
    dev, ref = _check_route(c, "evaluator")
    off = R.metric_sums_ref(pred, y, 0, 0.0, 1.0, None, None, NAN, NAN, -1.0)
    zeroed = (np.abs(y[..., 0]) == 0.0625).sum(axis=(0, 2))                       # with the zeroing off they are labels != 0
    assert (off[:, 5] - ref[:, 5]).tolist() == zeroed.tolist() and zeroed[0] >= 1 and zeroed[1] >= 1


def test_all_masked(lib_built):
    """one horizon without an unmasked label: MAE@k = 0, the masked_* columns 0, no gradient over that slab; the whole
    batch masked: loss 0.0 and an all-zero, finite gradient"""
    from multistgraph_amd import ops
    c = _scalar(_base(), 0, 2)
    c["y"][:, 2] = 0.0
    R.assert_exact(c, min_s=R.EXACT_MIN_S)
    got, want, count = _assert_loss_exact(c)
    assert got[1 + 2] == 0.0 and got[0] > 0 and (got[[1, 2, 4, 5, 6]] > 0).all()
    grad, _, _ = _assert_grad_exact(c)
    assert (grad[:, 2] == 0).all() and (grad[:, 3] != 0).any()
    dev, ref = _check_route(c, "evaluator")
    table = _host(ops.metric_table(dev))
    assert ref[2, 5] == 0 and (table[0, 2, 4:8] == 0).all() and (table[0, 3, 4:8] > 0).all()
    assert np.isinf(table[0, 2, 1]) and table[0, 2, 0] > 0       # the plain MAPE of zero labels is inf, the plain MAE is not 0
    c["y"][:] = 0.0
    got, want, count = _assert_loss_exact(c)
    assert count == 0 and (got == 0).all()
    grad, _, loss = _assert_grad_exact(c)
    assert loss == 0.0 and (grad == 0).all()


def test_metric_sums_with_nan_and_inf(lib_built):
    """NaN labels: left out of sum 1, counted in sum 5, sums 9 / 10 / 13 NaN and with them R2 / EVAR, in reference and
    device alike; one NaN and one inf prediction under finite labels"""
    from multistgraph_amd import ops
    c = _scalar(_base(), 1, 2)
    c["y"][1, 2, 7:12, 0] = NAN
    c["pred"][0, 3, 40, 0] = NAN
    c["pred"][2, 4, 256, 0] = float("inf")
    c["y"][2, 4, 256, 0] = 1.0
    R.assert_exact(c, min_s=R.EXACT_MIN_S)
    dev, ref = _check_route(c, "evaluator")
    got = _host(dev)
    n = 3 * 257
    assert got[2, 0] == n and got[2, 1] == n - 5 and np.isnan(got[2, [9, 10, 13]]).all() and np.isfinite(got[2, [2, 3, 11, 12]]).all()
    zeros = int((R.metric_elements(c["pred"], c["y"], 0, 1.0, 2.0, None, None, NAN, NAN, R.EXACT_MIN_S)[0][:, 2] == 0).sum())
    assert got[2, 5] == n - zeros                                 # a NaN label is a label != 0
    assert np.isnan(got[3, [11, 12, 13]]).all() and np.isfinite(got[3, [2, 3, 9, 10]]).all()
    assert np.isinf(got[4, [2, 3, 6, 7, 11, 12]]).all() and got[4, 13] == -np.inf
    table = _host(ops.metric_table(dev))
    assert np.isnan(table[0, 2, 8:]).all() and np.isnan(table[1, 2:, 8:]).all() and np.isfinite(table[0, :2, 8:]).all()
    assert np.isfinite(table[0, 2, [0, 2, 3, 4, 5, 6, 7]]).all()


def test_thresholds(lib_built):
    """a label exactly at truth_min is left out (the test is `>`), the next grid value kept; a prediction of -1/16 is
    clamped to 0, one of exactly 0 is not touched; min_s = -1 switches the zeroing off (the groupstd_table route)"""
    from multistgraph_amd import ops
    c = _scalar(_base(), 0, 1)
    y, pred = c["y"], c["pred"]
    y[0, 0, :, 0] = np.where(np.arange(257) % 2 == 0, 1.0, 1.0625)
    y[1, 1, 0:4, 0] = [0.0625, -0.0625, 0.03125, 2.0]
    pred[2, 2, 0:3, 0] = [-0.0625, 0.0, -0.0]
    y[2, 2, 0:3, 0] = 2.0
    R.assert_exact(c, clamp_min=R.EXACT_CLAMP_MIN)
    c["group_mean"], c["group_std"] = np.zeros(257, np.float32), np.ones(257, np.float32)
    only = {"truth": (NAN, R.EXACT_TRUTH_MIN, -1.0), "clamp": (R.EXACT_CLAMP_MIN, NAN, -1.0), "off": (NAN, NAN, -1.0)}
    ref = {}
    for k, (clamp, truth, min_s) in only.items():
        dev = ops.metric_sums(_dev(pred), _dev(y), 0, 0.0, 1.0, clamp_min=clamp, truth_min=truth, min_s=min_s)
        ref[k] = R.metric_sums_ref(pred, y, 0, 0.0, 1.0, None, None, clamp, truth, min_s)
        _assert_sums(_host(dev), ref[k])
    for route in ROUTES:
        _check_route(c, route)
    l, p, keep = R.metric_elements(pred, y, 0, 0.0, 1.0, None, None, R.EXACT_CLAMP_MIN, R.EXACT_TRUTH_MIN, -1.0)
    assert not keep[0, 0, 0::2, 0].any() and keep[0, 0, 1::2, 0].all()
    assert p[2, 2, 0, 0] == 0.0 and p[2, 2, 1, 0] == 0.0
    assert ref["clamp"][2, 11] > ref["off"][2, 11] and ref["truth"][0, 0] < ref["off"][0, 0]
    on = R.metric_sums_ref(pred, y, 0, 0.0, 1.0, None, None, NAN, NAN, R.EXACT_MIN_S)
    assert ref["off"][1, 5] >= on[1, 5] + 3                      # +-1/16 and 1/32 stay labels != 0 with the zeroing off


def test_constant_labels(lib_built):
    """a horizon of constant labels: ssTot == 0, sklearn's convention - R2 = EVAR = 1 where p == l, 0 where not; the same
    with swap_r2 and a constant prediction"""
    from multistgraph_amd import ops
    c = _scalar(_base(), 0, 1)
    y, pred = c["y"], c["pred"]
    y[:, 1], pred[:, 1] = 2.0, 2.0
    y[:, 2] = 2.0
    pred[:, 3] = 1.5
    y[:, 4], pred[:, 4] = -3.0, -3.0
    R.assert_exact(c)
    dev, _ = _check_route(c, "evaluator")
    plain, swapped = _host(ops.metric_table(dev))[0], _host(ops.metric_table(dev, swap_r2=True))[0]
    assert plain[1, 8:].tolist() == [1.0, 1.0] and plain[2, 8:].tolist() == [0.0, 0.0] and plain[4, 8:].tolist() == [1.0, 1.0]
    assert swapped[3, 8:].tolist() == [0.0, 0.0] and swapped[1, 8:].tolist() == [1.0, 1.0]
    assert 0 < plain[0, 8] < 1 and 0 < plain[0, 9] < 1
    p64, l64 = _descaled64(c)
    _assert_oracle(plain, _oracle_eval(p64, l64, "single", R.EXACT_MIN_S))


def test_large_offset(lib_built):
    """scaler mean 4096, std 1: s2 - s1^2 / n loses 22 bits, where the one-pass variance is most fragile.  Still on the
    grid (asserted), so the sums are exact; R2 / EVAR against the two-pass oracle within the conditioned bound"""
    from multistgraph_amd import ops
    c = _scalar(_base(), 4096, 1)
    r = R.assert_exact(c, min_s=R.EXACT_MIN_S)
    assert r["max_l"] >= 4092
    dev, _ = _check_route(c, "evaluator")
    p64, l64 = _descaled64(c)
    cond_t, cond_d = R.table_conditioning(_host(dev))
    print("s2 / ssTot %.3g" % cond_t.max())
    assert cond_t.min() > 1e6
    for mode, name in enumerate(("single", "average")):
        bound = 1e-15 * np.stack([cond_t[mode], cond_t[mode] + cond_d[mode]], 1)
        _assert_oracle(_host(ops.metric_table(dev))[mode], _oracle_eval(p64, l64, name, R.EXACT_MIN_S), cond=bound)


AFFINES = ["scalar", "per_node", "scalar_mean_vector_std", "per_node_group", "n1_vectors"]


@pytest.mark.parametrize("kind", AFFINES)
def test_affine_routes_through_the_evaluator(kind, lib_built):
    """every way ops.metric_sums takes the first affine (scalars, vectors, one of each: the broadcast branch; a one-entry
    vector at N = 1), with and without the group affine, through DeviceEvaluator.collect_scaled and groupstd_table"""
    from multistgraph_amd.evaluator import ALLOWED_METRICS, DeviceEvaluator, groupstd_table
    b, out, n, od = (3, 6, 1, 1) if kind == "n1_vectors" else (3, 6, 257, 2)
    c = R.grid_case(55, b, out, n, od, y_feat=od + 1, y_start=1, per_node=kind != "scalar", group=True)
    if kind == "scalar_mean_vector_std":
        c["mean"] = 1.0
    if kind == "n1_vectors":
        assert c["mean"].shape == (1,) and c["group_std"].shape == (1,)
        f = np.float32
        c["mean"], c["std"], c["group_mean"], c["group_std"] = (np.array([v], f) for v in (1.0, 2.0, 1.0, 0.5))
        off = c["pred"] - c["y"][:, :out, :, 1:2]
        c["y"][..., 1] = np.abs(c["y"][..., 1]) + 2.0             # every label ends above truth_min: (2y + 1) / 2 + 1 >= 3.5
        c["pred"] = c["y"][:, :out, :, 1:2] + off
    R.assert_exact(c)
    pd, yd = _dev(c["pred"]), _dev(c["y"])
    sums = R.metric_sums_ref(c["pred"], c["y"], 1, c["mean"], c["std"], None, None, NAN, NAN, R.EXACT_MIN_S)
    want = R.metric_table_ref(sums)
    for mode, name in enumerate(("single", "average")):
        ev = DeviceEvaluator({"metrics": list(ALLOWED_METRICS), "evaluator_mode": name, "min_s": R.EXACT_MIN_S})
        ev.collect_scaled(pd, yd, 1, c["mean"], c["std"])
        _assert_table(ev.table().numpy(), want[mode], sums, False, mape_rtol=QUOT_TOL, mode=mode)
        res = ev.evaluate()
        assert res["RMSE@%d" % out] == float(ev.table()[out - 1, 3]) and len(res) == 10 * out
    gsum = R.metric_sums_ref(c["pred"], c["y"], 1, c["mean"], c["std"], c["group_mean"], c["group_std"], 0.0, 1.0, -1.0)
    gwant = R.metric_table_ref(gsum, True)[0]
    assert gsum[:, 0].min() > 0
    cols, dsums = groupstd_table(pd, yd, c["group_mean"], c["group_std"], 1, c["mean"], c["std"], s_small=1.0)
    _assert_sums(_host(dsums), gsum)
    have = np.full((out, 10), NAN)
    for k, col in zip(GROUP_KEYS, GROUP_COLS):
        have[:, col] = cols[k].numpy()
    gwant[:, [k for k in range(10) if k not in GROUP_COLS]] = NAN
    _assert_table(have, gwant, gsum, True, mape_rtol=QUOT_TOL, mode=0)


def test_accumulate_over_unequal_batches(lib_built):
    """one collect of B = 69 against streaming collects of B = 1, 65, 3 over the same samples: the same sums, bit for
    bit - through ops.metric_sums, DeviceEvaluator(streaming=True) and the sums= argument of groupstd_table; and the
    non-streaming evaluator: the mean of the batches' tables, an inf MAPE among them"""
    from multistgraph_amd import ops
    from multistgraph_amd.evaluator import ALLOWED_METRICS, DeviceEvaluator, groupstd_table
    c = _scalar(R.grid_case(77, 69, 6, 257, 1, group=True), 1, 1)
    R.assert_exact(c)
    pred, y = c["pred"], c["y"]
    gm, gs = c["group_mean"], c["group_std"]
    # the quotient sums too are exact in any order here: every finite |d / l| is a float32 of at least 2^-9, its last bit
    # at or above 2^-32, and a horizon's sum stays below 2^53 of those
    for elements in (R.metric_elements(pred, y, 0, 1.0, 1.0, None, None, NAN, NAN, R.EXACT_MIN_S),
                     R.metric_elements(pred, y, 0, 1.0, 1.0, gm, gs, 0.0, 1.0, -1.0)):
        l, p, keep = elements
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.abs((p - l) / l)[keep]
        q = q[np.isfinite(q) & (q > 0)]
        assert q.min() >= 2.0 ** -9 and 69 * 257 * float(q.max()) / 2.0 ** -32 < 2.0 ** 53
    parts = [slice(0, 1), slice(1, 66), slice(66, 69)]
    pd, yd = _dev(pred), _dev(y)
    whole = ops.metric_sums(pd, yd, 0, 1.0, 1.0, min_s=R.EXACT_MIN_S)
    _assert_sums(_host(whole), R.metric_sums_ref(pred, y, 0, 1.0, 1.0, None, None, NAN, NAN, R.EXACT_MIN_S))
    run = None
    for s in parts:
        run = ops.metric_sums(pd[s], yd[s], 0, 1.0, 1.0, min_s=R.EXACT_MIN_S, sums=run)
    assert torch.equal(run, whole)
    cfg = {"metrics": list(ALLOWED_METRICS), "evaluator_mode": "average", "min_s": R.EXACT_MIN_S}
    one, st, sep = DeviceEvaluator(cfg), DeviceEvaluator(cfg, streaming=True), DeviceEvaluator(cfg)
    one.collect_scaled(pd, yd, 0, 1.0, 1.0)
    for s in parts:
        st.collect_scaled(pd[s], yd[s], 0, 1.0, 1.0)
        sep.collect_scaled(pd[s], yd[s], 0, 1.0, 1.0)
    assert torch.equal(st.table(), one.table()) and torch.equal(st.table(), ops.metric_table(whole)[1].cpu())
    _, gwhole = groupstd_table(pd, yd, gm, gs, 0, 1.0, 1.0, s_small=1.0)
    grun, cols = None, None
    for s in parts:
        cols, grun = groupstd_table(pd[s], yd[s], gm, gs, 0, 1.0, 1.0, s_small=1.0, sums=grun)
    _assert_sums(_host(gwhole), R.metric_sums_ref(pred, y, 0, 1.0, 1.0, gm, gs, 0.0, 1.0, -1.0))
    assert torch.equal(grun, gwhole)
    assert torch.equal(cols["MAE"], groupstd_table(pd, yd, gm, gs, 0, 1.0, 1.0, s_small=1.0)[0]["MAE"])
    tables = [R.metric_table_ref(R.metric_sums_ref(pred[s], y[s], 0, 1.0, 1.0, None, None, NAN, NAN, R.EXACT_MIN_S))[1]
              for s in parts]
    with np.errstate(invalid="ignore"):
        want = np.mean(tables, 0)
    assert np.isinf(want[:, 1]).any() and np.isfinite(want[:, 5]).all()
    got = sep.table().numpy()
    with np.errstate(invalid="ignore"):
        ok = _same(got, want) | (np.abs(got - want) <= np.where(np.isin(np.arange(10), MAPE_COLS), QUOT_TOL, 1e-12) * np.abs(want))
    assert ok.all(), (np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


def test_label_start_gathers_what_the_windows_hold(lib_built):
    """loss, gradient and metric sums gathered from a (T, N, F) series equal the materialised windows bit for bit - starts
    at 0, at exactly T - out, duplicated and overlapping -, and the range counter stays 0; one start past the end: the
    metric kernel clamps the rows into the series (by design: nothing is read outside) and counts them"""
    from multistgraph_amd import ops
    t_steps, out, n, od, feat, y_start = 40, 6, 257, 2, 4, 1
    rng = np.random.default_rng(31)
    series = (rng.integers(-64, 65, (t_steps, n, feat)) / 16.0).astype(np.float32)
    starts = np.array([0, t_steps - out, 5, 5, 7], dtype=np.int32)
    windows = np.stack([series[s:s + out] for s in starts], 0)
    pred = (windows[..., y_start:y_start + od] + rng.integers(-16, 17, (5, out, n, od)) / 16.0).astype(np.float32)
    cw = dict(y=windows, pred=pred, y_start=y_start, mean=-1.0, std=2.0, group_mean=None, group_std=None)
    cs = dict(cw, y=series)
    R.assert_exact(cw)
    _violations()
    lw, _, _ = _assert_loss_exact(cw)
    ls, _, _ = _assert_loss_exact(cs, label_start=starts)
    assert np.array_equal(lw, ls)
    gw, _, _ = _assert_grad_exact(cw)
    gs, _, _ = _assert_grad_exact(cs, label_start=starts)
    assert np.array_equal(gw, gs)
    sw, _ = _check_route(cw, "evaluator")
    ss, _ = _check_route(cs, "evaluator", label_start=starts)
    assert torch.equal(sw, ss)
    assert _violations() == 0
    bad = starts.copy()
    bad[3] = t_steps - 2                       # rows T-2, T-1, then four past the end: clamped to T-1
    assert np.array_equal(R.label_rows(series, out, 0, feat, bad)[3, 2:], np.broadcast_to(series[-1], (4, n, feat)))
    sb, _ = _check_route(cs, "evaluator", label_start=bad)
    assert not torch.equal(sb, ss) and _violations() > 0
    assert _violations() == 0


def test_run_to_run(lib_built):
    """the three entry points twice on one input: fixed summation order, identical bits (continuous data)"""
    from multistgraph_amd import ops
    rng = np.random.default_rng(8)
    y = _dev(rng.standard_normal((3, 8, 1039, 3)).astype(np.float32))
    pred = _dev(rng.standard_normal((3, 6, 1039, 2)).astype(np.float32))
    a, b = (ops.masked_mae_device(pred, y, 1, 14.41, 29.3, 0.0) for _ in range(2))
    assert torch.equal(a, b)
    grads = []
    for _ in range(2):
        p = pred.clone().requires_grad_(True)
        ops.masked_mae_loss(p, y, 1, 14.41, 29.3, 0.0).backward()
        grads.append(p.grad)
    assert torch.equal(grads[0], grads[1]) and float(grads[0].abs().max()) > 0
    a, b = (ops.metric_sums(pred, y, 1, 14.41, 29.3) for _ in range(2))
    assert torch.equal(a, b) and torch.equal(ops.metric_table(a), ops.metric_table(b))


def test_host_refusals(lib_built):
    """what the host refuses before any launch"""
    from multistgraph_amd import ops
    from multistgraph_amd._lib import MatgcnError
    y = torch.zeros(2, 66, 5, 3, device="cuda:0")
    pred = torch.zeros(2, 6, 5, 2, device="cuda:0")
    series, starts = torch.zeros(40, 5, 3, device="cuda:0"), torch.zeros(2, dtype=torch.int32, device="cuda:0")
    entries = [lambda p, yy, ys, **kw: ops.masked_mae_device(p, yy, ys, 0.0, 1.0, **kw),
               lambda p, yy, ys, **kw: ops.masked_mae_loss(p, yy, ys, 0.0, 1.0, **kw),
               lambda p, yy, ys, **kw: ops.metric_sums(p, yy, ys, **kw)]
    for call in entries:
        call(pred, y, 1)                                                   # the valid call goes through
        call(pred, series, 1, label_start=starts)
        with pytest.raises(MatgcnError):
            call(torch.zeros(2, 65, 5, 2, device="cuda:0"), y, 1)           # out = 65
        with pytest.raises(MatgcnError):
            call(pred, y, 2)                                               # y_start + od > y_feat
        with pytest.raises(MatgcnError):
            call(pred, y[:, :5].contiguous(), 1)                           # y_steps < out
        with pytest.raises(MatgcnError):
            call(pred.double(), y, 1)                                      # a float64 pred
        with pytest.raises(MatgcnError):
            call(pred, series, 1, label_start=starts.cpu())                # a CPU label_start
    with pytest.raises(MatgcnError):
        ops.metric_sums(pred, y, 1, sums=torch.zeros(6, 13, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(MatgcnError):
        ops.metric_sums(pred, y, 1, sums=torch.zeros(7, 14, dtype=torch.float64, device="cuda:0"))


# ---- the realistic group -----------------------------------------------------------------------------------------------------
MEAN, STD = 14.41, 29.3        # Baltimore's flow statistics, as tests/golden/make_metrics_golden.py


def _realistic(seed, b, out, n, od, y_start):
    """Continuous data as make_metrics_golden.py draws them, the planted elements of its case "a" placed well inside
    each side of every threshold, and every other element moved out of an ulp's reach of one: the raw label + 1 where
    the de-scaled |l| is in [5e-5, 2e-4] or the re-transformed l within 1e-3 relative of truth_min = 10, the raw
    prediction + 1 where the re-transformed p is within 1e-3 of clamp_min = 0 or |p - l| < 1e-3 (the sign of p - l is a
    threshold for the gradient).  Asserted on the reference: none remain."""
    rng = np.random.default_rng(seed)
    y_feat = y_start + od
    y = rng.standard_normal((b, out + 1, n, y_feat)).astype(np.float32)
    pred = (y[:, :out, :, y_start:] + 0.3 * rng.standard_normal((b, out, n, od))).astype(np.float32)
    gm, gs = rng.uniform(5.0, 60.0, n).astype(np.float32), rng.uniform(3.0, 40.0, n).astype(np.float32)
    planted = np.zeros(pred.shape, dtype=bool)
    plants = {(0, 0, 0, 0): 0.0, (0, 1, n - 1, od - 1): 2e-5, (1, 0, n // 2, 0): -2e-5, (1, 2, 0, od - 1): 4e-4}
    for (pb, po, pn, pc), v in plants.items():
        y[pb, po, pn, y_start + pc] = np.float32((v - MEAN) / STD)
        planted[pb, po, pn, pc] = True
    pred[1, 3, 1 % n, 0] = y[1, 3, 1 % n, y_start]                        # p == l, bit for bit
    planted[1, 3, 1 % n, 0] = True

    def state():
        l, p, _ = R.metric_elements(pred, y, y_start, MEAN, STD, None, None, NAN, NAN, -1.0)
        l2, p2, _ = R.metric_elements(pred, y, y_start, MEAN, STD, gm, gs, NAN, NAN, -1.0)
        near_l = ((np.abs(l) >= 5e-5) & (np.abs(l) <= 2e-4)) | (np.abs(l2 - 10.0) <= 1e-2)
        near_p = (np.abs(p2) <= 1e-3) | (np.abs(p - l) < 1e-3)
        return l, near_l & ~planted, near_p & ~planted

    for _ in range(3):
        l, near_l, near_p = state()
        if not (near_l.any() or near_p.any()):
            break
        y[:, :out, :, y_start:][near_l] += np.float32(1.0)
        pred[near_p] += np.float32(1.0)
    l, near_l, near_p = state()
    assert not near_l.any() and not near_p.any()
    for at, v in plants.items():
        assert abs(float(l[at]) - v) <= 1e-5, (at, float(l[at]))           # well inside: 5e-5 and 2e-4 are 3e-5 and more away
    return dict(y=y, pred=pred, y_start=y_start, mean=MEAN, std=STD, group_mean=gm, group_std=gs), planted


@pytest.mark.parametrize("shape", [(3, 12, 257, 1, 0), (5, 24, 171, 3, 1), (2, 24, 1039, 1, 0), (2, 24, 4096, 1, 0)],
                         ids=lambda s: "b%d_out%d_n%d_od%d" % s[:4])
def test_realistic(shape, lib_built):
    from multistgraph_amd import ops
    from multistgraph_amd.evaluator import ALLOWED_METRICS, DeviceEvaluator, groupstd_table
    c, planted = _realistic(13, *shape)
    pred, y, y_start = c["pred"], c["y"], c["y_start"]
    out = pred.shape[1]
    pd, yd = _dev(pred), _dev(y)
    # the loss and each MAE@k: 2e-6 relative (test_model_gpu.py)
    got = _host(ops.masked_mae_device(pd, yd, y_start, MEAN, STD, 0.0, 1e-4))
    want, count = R.mae_ref(pred, y, y_start, MEAN, STD, 0.0, 1e-4)
    print("loss %r reference %r, worst relative %.3g" % (got[0], want[0], float((np.abs(got - want) / want).max())))
    assert count == pred.size - 3 and (np.abs(got - want) <= 2e-6 * np.abs(want)).all()
    # the gradient: 1e-6 max-normalised, exact zeros at masked elements
    p = pd.clone().requires_grad_(True)
    (ops.masked_mae_loss(p, yd, y_start, MEAN, STD, 0.0, 1e-4) * UPSTREAM).backward()
    grad = _host(p.grad)
    gwant = R.mae_grad_ref(pred, y, y_start, MEAN, STD, 0.0, 1e-4, UPSTREAM)
    _, _, mask = R.mae_elements(pred, y, y_start, MEAN, STD, 0.0, 1e-4)
    err = max_norm_err(grad, gwant)
    print("gradient max-normalised error %.3g" % err)
    assert err <= 1e-6 and (grad[~mask] == 0).all() and (~mask).sum() == 3 and grad[1, 3, 1 % pred.shape[2], 0] == 0
    # the evaluator's table and the re-transform table: 2e-5 relative + 1e-9 per entry (test_metrics.py)

    def close(have, ref):
        with np.errstate(invalid="ignore"):
            ok = _same(have, ref) | (np.abs(have - ref) <= 2e-5 * np.abs(ref) + 1e-9)
        assert ok.all(), (np.argwhere(~ok)[:5].tolist(), have[~ok][:5], ref[~ok][:5])

    table = R.metric_table_ref(R.metric_sums_ref(pred, y, y_start, MEAN, STD, None, None, NAN, NAN, 1e-4))
    assert np.isinf(table[0][:2, 1]).all() and np.isfinite(table[0][:, 5]).all()
    for mode, name in enumerate(("single", "average")):
        ev = DeviceEvaluator({"metrics": list(ALLOWED_METRICS), "evaluator_mode": name})
        ev.collect_scaled(pd, yd, y_start, MEAN, STD)
        close(ev.table().numpy(), table[mode])
    gref = R.metric_table_ref(R.metric_sums_ref(pred, y, y_start, MEAN, STD, c["group_mean"], c["group_std"], 0.0, 10.0, -1.0),
                              True)[0]
    cols, _ = groupstd_table(pd, yd, c["group_mean"], c["group_std"], y_start, MEAN, STD)
    close(np.stack([cols[k].numpy() for k in GROUP_KEYS], 1), gref[:, GROUP_COLS])
