"""The executor's training objectives on the device (csrc/matgcn_loss.hip: k_loss_partial / k_loss_final / k_loss_grad
behind matgcn_loss / matgcn_loss_grad) against the numpy reference of tests/train_loss_ref.py, which the host tests pin to
the reference's own loss functions (tests/test_train_loss_host.py).

EXACT: every value sits on a dyadic grid (train_loss_ref.grid_case), so no float32 operation rounds and every sum is exact
in any order - each test asserts that on its own reference before it launches (train_loss_ref.assert_exact).  Then for
MAE, MSE, RMSE (NaN and 0 null value), HUBER (delta 1) and QUANTILE (delta 0.25) result[0] and every result[1 + k] are
bit-equal to float32 of the float64 reference, the gradient is within 1 float32 ulp of the closed form and exactly 0 where
that is 0.  MAPE adds one quotient per term: 2^-22 relative (the project's quotient allowance), inf == inf.
REALISTIC: the fixture's continuous inputs and one larger draw (B = 5, out = 24, N = 403) under Baltimore's scaler.  The
error against the float64 reference is at most twice the gap of a float32 torch CPU run of the reference's arithmetic on
the same inputs (for the fixture: the reference's own recorded run), with a floor of 2^-22 relative; the same bar for the
gradient, max-normalised, with exact zeros at masked elements.  Both runs start from the same float32 de-scaled values,
so the rounding of x*std + mean is common to them; what remains on our side is one float32 rounding of the result,
2^-24.  result[1 + k] is the objective of the slab [:, k] alone and is held to the same rule with its own yardstick: the
float32 torch run on that slab (one label near 0 moves a horizon's MAPE far more than it moves the total's).
The logcosh case with |d| up to 5000 uses a power-of-two std and mean 0, so that the de-scale is exact and the case is
about log(cosh) alone: the float32 torch run is inf there, its gap is no number, and the floor is the bar.
The figures this file prints are recorded in DESIGN.md section 5b."""
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest
import torch

import train_loss_ref as R
from helpers import GOLDEN_DIR, Case, max_norm_err

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -22
UPSTREAM = 4.0          # a power of two keeps upstream * std exact
EXACT_NAMES = ("mae", "masked_mae", "mse", "masked_mse", "rmse", "masked_rmse", "huber", "quantile")
MAPE_NAMES = ("mape", "masked_mape")
ELEVEN = tuple(R.LOSSES)
ZERO_FREE = ("mape", "logcosh", "huber", "quantile")
GOLD = np.load(os.path.join(GOLDEN_DIR, "train_loss_small.npz"))
MEAN, STD = float(GOLD["mean"]), float(GOLD["std"])


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """The models and autograd nodes of the end-to-end tests die in reference cycles.  Collect them when the module is
    done and hand torch's cached blocks back: otherwise their device memory is freed at a moment of the collector's
    choosing, in the middle of a later module that watches which address the caching allocator hands out."""
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _run(name, c, label_start=None, delta=None, upstream=UPSTREAM):
    """((1 + out,) values, gradient, the autograd scalar) of case c through ops.train_loss_device / ops.train_loss"""
    from multistgraph_amd import ops
    ls = None if label_start is None else _dev(np.asarray(label_start, dtype=np.int32))
    y = _dev(c["y"])
    p = _dev(c["pred"]).requires_grad_(True)
    full = ops.train_loss_device(p.detach(), y, c["y_start"], c["mean"], c["std"], name, delta, ls)
    loss = ops.train_loss(p, y, c["y_start"], c["mean"], c["std"], name, delta, ls)
    (loss * upstream).backward()
    full = _host(full)
    assert full.dtype == F32 and _same(full[0], _host(loss)).all()
    return full, _host(p.grad), loss.detach()


def _ref(name, c, label_start=None, delta=None, upstream=UPSTREAM):
    r = R.train_loss_ref(name, c["pred"], c["y"], c["y_start"], c["mean"], c["std"], delta, label_start, upstream)
    r["values"] = np.concatenate([[r["value"]], r["horizons"]])
    return r


# ---- EXACT ----------------------------------------------------------------------------------------------------------------
def _shape(b=3, out=6, n=257, od=1, y_steps=None, y_feat=None, y_start=0):
    return (b, out, n, od, out if y_steps is None else y_steps, y_start + od if y_feat is None else y_feat, y_start)


SHAPES = {"base": _shape()}
# N * od across the 256-thread block (the slab loop of k_loss_partial, the index split of k_loss_grad); B * out * N * od is a
# multiple of 256 at N = 256 only: every other shape has a partial last block in the gradient
for _n, _od in ((1, 1), (255, 1), (256, 1), (171, 3)):
    SHAPES["n%d_od%d" % (_n, _od)] = _shape(n=_n, od=_od)
# label channels in the middle of the feature axis and at its end
SHAPES["od2_feat5_start2"] = _shape(od=2, y_feat=5, y_start=2)
SHAPES["od3_feat4_start1"] = _shape(n=171, od=3, y_feat=4, y_start=1)
# horizons up to the limit of 64 (k_loss_final's one wave), label windows as long as the horizon and longer
for _out in (1, 24, 64):
    SHAPES["out%d" % _out] = _shape(out=_out, n=65)
    SHAPES["out%d_steps%d" % (_out, _out + 2)] = _shape(out=_out, n=65, y_steps=_out + 2)
SHAPES["b1"] = _shape(b=1)
SHAPES["b65"] = _shape(b=65, n=65)
SHAPE_IDS = list(SHAPES)


@functools.lru_cache(maxsize=None)
def _grid(shape_name, nan_labels):
    b, out, n, od, y_steps, y_feat, y_start = SHAPES[shape_name]
    c = R.grid_case(SHAPE_IDS.index(shape_name) + 1, b, out, n, od, y_steps=y_steps, y_feat=y_feat, y_start=y_start)
    if nan_labels:          # NaN labels for the kinds that mask them, in label rows and channels and outside them
        rng = np.random.default_rng(7)
        c = dict(c, y=c["y"].copy())
        c["y"].reshape(-1)[rng.integers(0, c["y"].size, max(1, c["y"].size // 50))] = NAN
    return c


def _case_for(name, shape_name):
    return _grid(shape_name, R.LOSSES[name][0] in R.MASKED and not name.startswith("masked_"))


def _assert_exact_values(name, got, want):
    if name in MAPE_NAMES:
        with np.errstate(invalid="ignore"):
            ok = _same(got, want["values"]) | (np.abs(got - want["values"]) <= FLOOR * np.abs(want["values"]))
        assert ok.all(), (name, got, want["values"])
    else:
        assert np.array_equal(got, want["values"].astype(F32)), (name, got, want["values"].astype(F32))


def _assert_exact_grad(name, got, want):
    g = want["grad"]
    assert got.dtype == F32 and got.shape == g.shape
    zero = g == 0
    assert (got[zero] == 0).all(), "%s: a gradient where the reference has none" % name
    with np.errstate(invalid="ignore"):
        err = np.abs(got.astype(F64) - g)
        tol = FLOOR * np.abs(g) if name in MAPE_NAMES else np.spacing(np.abs(g).astype(F32)).astype(F64)
        ok = _same(got, g.astype(F32)) | (err <= tol)
    assert ok.all(), (name, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], g[~ok][:5])


@pytest.mark.parametrize("shape_name", SHAPE_IDS)
def test_exact(shape_name, lib_built):
    for name in EXACT_NAMES + MAPE_NAMES:
        c = _case_for(name, shape_name)
        R.assert_exact(name, c)
        want = _ref(name, c)
        got, grad, _ = _run(name, c)
        _assert_exact_values(name, got, want)
        _assert_exact_grad(name, grad, want)
        if name not in MAPE_NAMES:
            assert np.isfinite(got).all() and want["count"] > 0


def test_label_start_gathers_what_the_windows_hold(lib_built):
    """value and gradient gathered from a (T, N, F) series equal the materialised windows bit for bit - starts at 0, at
    exactly T - out (the last valid one), duplicated and overlapping - and match the reference"""
    t_steps, out, n, od, feat, y_start = 40, 6, 257, 2, 4, 1
    rng = np.random.default_rng(31)
    series = (rng.integers(-64, 65, (t_steps, n, feat)) / 16.0).astype(F32)
    starts = np.array([0, t_steps - out, 5, 5, 7], dtype=np.int32)
    windows = np.stack([series[s:s + out] for s in starts], 0)
    pred = (windows[..., y_start:y_start + od] + rng.integers(-16, 17, (5, out, n, od)) / 16.0).astype(F32)
    cw = dict(y=windows, pred=pred, y_start=y_start, mean=-1.0, std=2.0)
    cs = dict(cw, y=series)
    for name in EXACT_NAMES + MAPE_NAMES:
        R.assert_exact(name, cw)
        want = _ref(name, cs, label_start=starts)
        assert np.array_equal(want["values"], _ref(name, cw)["values"], equal_nan=True)
        vw, gw, _ = _run(name, cw)
        vs, gs, _ = _run(name, cs, label_start=starts)
        assert _same(vw, vs).all() and _same(gw, gs).all(), name
        _assert_exact_values(name, vs, want)
        _assert_exact_grad(name, gs, want)


# ---- semantics --------------------------------------------------------------------------------------------------------------
def _base(seed=101, **kw):
    return R.grid_case(seed, *SHAPES["base"][:4], **kw)


def test_all_masked(lib_built):
    c = _base()
    c = dict(c, y=np.zeros_like(c["y"]), mean=0.0, std=2.0)
    for name in ("masked_mae", "masked_mse", "masked_rmse", "masked_mape"):
        got, grad, _ = _run(name, c)
        assert (got == 0).all() and (grad == 0).all(), name
    c = dict(c, y=np.full_like(c["y"], NAN))
    for name in ("mae", "mse", "rmse", "mape"):
        got, grad, _ = _run(name, c)
        assert (got == 0).all() and (grad == 0).all(), name


def test_nan_label_under_an_unmasked_kind(lib_built):
    c = _base()
    c = dict(c, y=c["y"].copy())
    c["y"][1, 2, 5, 0] = NAN
    for name in ("logcosh", "huber", "quantile"):
        got, _, _ = _run(name, c)
        fin = np.ones(got.shape, dtype=bool)
        fin[[0, 3]] = False                       # the total and horizon 2
        assert np.isnan(got[~fin]).all() and np.isfinite(got[fin]).all(), (name, got)


def test_rmse_zero_gives_a_zero_gradient(lib_built):
    c = _base()
    c = dict(c, pred=c["y"][:, :, :, :1].copy())
    for name in ("rmse", "masked_rmse"):
        got, grad, _ = _run(name, c)
        assert (got == 0).all() and (grad == 0).all(), name     # torch: 0 / 0 = NaN


def test_unmasked_zero_label_under_mape_is_inf(lib_built):
    c = _base()
    c = dict(c, y=c["y"].copy(), pred=c["pred"].copy(), mean=0.0, std=2.0)
    c["y"][0, 1, 4, 0], c["pred"][0, 1, 4, 0] = 0.0, 0.5        # d != 0 over l == 0
    c["y"][0, 3, 9, 0], c["pred"][0, 3, 9, 0] = 0.0, 0.0        # 0 / 0: a NaN term, counts 0
    keep = np.abs(c["y"]) > 0
    keep[0, 1, 4, 0] = keep[0, 3, 9, 0] = True
    c["y"][~keep] = 1.0                                         # no other zero label
    got, grad, _ = _run("mape", c)
    want = _ref("mape", c)
    assert got[0] == INF and got[2] == INF and np.isfinite(got[[1, 3, 4, 5, 6]]).all()
    assert _same(got, want["values"].astype(F32))[[0, 2]].all()
    assert grad[0, 3, 9, 0] == 0.0 and np.isinf(grad[0, 1, 4, 0])
    got, grad, _ = _run("masked_mape", c)                       # the same labels masked: finite
    assert np.isfinite(got).all() and grad[0, 1, 4, 0] == 0.0 and grad[0, 3, 9, 0] == 0.0


def test_min_s_zeroes_and_masks(lib_built):
    """|l| < 1e-4 becomes 0: the masked_* names leave the element out, the NaN-null names keep it with l = 0"""
    b, out, n = 2, 3, 40
    y = np.full((b, out, n, 1), 2.0, dtype=F32)
    pred = np.full((b, out, n, 1), 3.0, dtype=F32)
    y[0, 0, :5, 0] = 5e-5               # below min_s: d becomes 3 instead of 3 - 5e-5
    y[1, 2, 7, 0] = 2e-4                # above: stays
    c = dict(y=y, pred=pred, y_start=0, mean=0.0, std=1.0)
    total = b * out * n
    got, grad, _ = _run("masked_mae", c)
    want = ((total - 6) * 1.0 + (3.0 - float(F32(2e-4)))) / (total - 5)
    assert abs(got[0] - want) <= 2e-7 * want and (grad[0, 0, :5] == 0).all() and grad[1, 2, 7, 0] > 0
    got, grad, _ = _run("mae", c)
    want = ((total - 6) * 1.0 + 5 * 3.0 + (3.0 - float(F32(2e-4)))) / total
    assert abs(got[0] - want) <= 2e-7 * want and (grad[0, 0, :5] > 0).all()
    got, _, _ = _run("mse", c)
    want = ((total - 6) * 1.0 + 5 * 9.0 + (3.0 - float(F32(2e-4))) ** 2) / total
    assert abs(got[0] - want) <= 2e-7 * want


def _raw_calls(name, c, fill):
    """matgcn_loss / matgcn_loss_grad on caller buffers pre-filled with ``fill``: (values, gradient, scratch)"""
    from multistgraph_amd import _lib, ops
    lib = _lib.load()
    pred, y = _dev(c["pred"]), _dev(c["y"])
    b, out, n, od = pred.shape
    desc = ops.train_loss_desc(name, c["mean"], c["std"])
    need = C.c_size_t()
    _lib.check(lib.matgcn_loss_bytes(b, out, C.byref(need)), "matgcn_loss_bytes")
    scratch = torch.full((need.value // 8,), fill, dtype=torch.float64, device=pred.device)
    result = torch.full((1 + out,), fill, dtype=torch.float32, device=pred.device)
    d_pred = torch.full_like(pred, fill)
    up = torch.full((1,), UPSTREAM, dtype=torch.float32, device=pred.device)
    stream = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    geo = (b, out, n, od, int(y.shape[1]), int(y.shape[3]), c["y_start"])
    _lib.check(lib.matgcn_loss(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), None, *geo, C.byref(desc),
                               C.c_void_p(scratch.data_ptr()), need.value, C.c_void_p(result.data_ptr()), stream),
               "matgcn_loss")
    _lib.check(lib.matgcn_loss_grad(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), None, *geo, C.byref(desc),
                                    C.c_void_p(scratch.data_ptr()), need.value, C.c_void_p(up.data_ptr()),
                                    C.c_void_p(d_pred.data_ptr()), stream), "matgcn_loss_grad")
    return _host(result), _host(d_pred), _host(scratch)


def _realistic_case(seed, b, out, n, zeros):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, out, n, 1)).astype(F32)
    pred = (y + 0.3 * rng.standard_normal((b, out, n, 1))).astype(F32)
    if zeros:
        y[0, :, :3, 0] = F32(-MEAN / STD)
        y[1, 2, 5, 0] = F32((5e-5 - MEAN) / STD)
        pred[1, 3, 7, 0] = y[1, 3, 7, 0]
    return dict(y=y, pred=pred, y_start=0, mean=MEAN, std=STD)


def test_run_to_run_and_dirty_buffers(lib_built):
    """two consecutive calls give equal bits (continuous data, every name), and neither NaN nor another finite filling of
    the caller's scratch, result and gradient buffers reaches a result"""
    for name in ELEVEN:
        c = _realistic_case(3, 5, 7, 301, name not in ZERO_FREE)
        v1, g1, _ = _run(name, c)
        v2, g2, _ = _run(name, c)
        assert np.array_equal(v1, v2) and np.array_equal(g1, g2), name
        rv, rg, rs = _raw_calls(name, c, NAN)
        assert np.array_equal(rv, v1) and np.array_equal(rg, g1), name
        assert np.isfinite(rv).all() and np.isfinite(rg).all() and np.isfinite(rs).all(), name
        rv, rg, _ = _raw_calls(name, c, 7.5)
        assert np.array_equal(rv, v1) and np.array_equal(rg, g1), name


# ---- REALISTIC ------------------------------------------------------------------------------------------------------------
def _bar(gap):
    return max(2.0 * gap, FLOOR) if np.isfinite(gap) else FLOOR


def _check_realistic(tag, name, c, v32, g32, delta=None):
    want = _ref(name, c, delta=delta, upstream=1.0)
    got, grad, _ = _run(name, c, delta=delta, upstream=1.0)
    v64, g64 = want["value"], want["grad"]
    with np.errstate(invalid="ignore", over="ignore"):
        gap_v = abs(float(v32) - v64) / abs(v64)
        fin = np.isfinite(g32)
        gmax = np.abs(g64).max()
        gap_g = float(np.abs(g32.astype(F64) - g64)[fin].max() / gmax) if fin.all() or name.startswith("masked_") else NAN
        # horizon k alone is the same objective on the slab [:, k]: the same float32 torch run on that slab is its yardstick
        h32 = np.array([float(R.torch_closure(name, c["pred"][:, k:k + 1], c["y"][:, k:k + 1], c["mean"], c["std"],
                                              torch.float32, delta)[0]) for k in range(c["pred"].shape[1])])
        gap_h = np.abs(h32 - want["horizons"]) / np.abs(want["horizons"])
    err_v = abs(float(got[0]) - v64) / abs(v64)
    err_h = np.abs(got[1:].astype(F64) - want["horizons"]) / np.abs(want["horizons"])
    err_g = float(np.abs(grad.astype(F64) - g64).max() / gmax)
    print("TRAIN-LOSS-GAP %s %-11s value: torch32 gap %.3g ours %.3g | horizons: worst gap %.3g ours %.3g | gradient: "
          "torch32 gap %.3g ours %.3g" % (tag, name, gap_v, err_v, np.nanmax(gap_h), err_h.max(), gap_g, err_g))
    assert np.isfinite(got).all() and np.isfinite(grad).all()
    assert err_v <= _bar(gap_v), (name, err_v, gap_v)
    bars = np.array([_bar(g) for g in gap_h])
    assert (err_h <= bars).all(), (name, err_h, gap_h)
    assert err_g <= _bar(gap_g), (name, err_g, gap_g)
    assert (grad[g64 == 0] == 0).all()


@pytest.mark.parametrize("name", ELEVEN)
def test_realistic_fixture(name, lib_built):
    """the reference's own recorded float32 run is the yardstick"""
    pred, y = (GOLD["pred"], GOLD["y"]) if name in ZERO_FREE else (GOLD["pred_z"], GOLD["y_z"])
    c = dict(y=y, pred=pred, y_start=0, mean=MEAN, std=STD)
    _check_realistic("fixture", name, c, GOLD[name + "_value32"], GOLD[name + "_grad32"])


@pytest.mark.parametrize("name", ELEVEN)
def test_realistic_larger_draw(name, lib_built):
    c = _realistic_case(41, 5, 24, 403, name not in ZERO_FREE)
    v32, g32 = R.torch_closure(name, c["pred"], c["y"], MEAN, STD, torch.float32)
    _check_realistic("b5_out24_n403", name, c, v32, g32)


def test_logcosh_far_past_the_range_of_cosh(lib_built):
    rng = np.random.default_rng(43)
    y = rng.uniform(-1.0, 1.0, (5, 24, 403, 1)).astype(F32)
    pred = (y + rng.uniform(-2.44, 2.44, y.shape)).astype(F32)
    c = dict(y=y, pred=pred, y_start=0, mean=0.0, std=2048.0)
    d = (pred.astype(F64) - y.astype(F64)) * 2048.0
    assert 4900.0 < np.abs(d).max() <= 5000.0 and (np.abs(d) < 1.0).any()
    v32, g32 = R.torch_closure("logcosh", pred, y, 0.0, 2048.0, torch.float32)
    assert np.isinf(v32)                                        # the reference's form in float32
    _check_realistic("d5000", "logcosh", c, v32, g32)


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _model(c, **extra):
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd.model import MultiATGCN
    dev = torch.device("cuda:0")
    cfg = dict(c.config("cuda:0"), hip_deterministic=True, **extra)
    m = MultiATGCN(cfg, dict(c.data_feature, scaler=syn.PlainScaler(MEAN, STD))).to(dev).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    return m, dev


def _grads(m):
    return {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}


def _labels_with_zeros(c):
    y = torch.from_numpy(c.y).clone()
    y[0, :, :3, 0] = -MEAN / STD
    return y


@pytest.mark.parametrize("name", ["huber", "masked_mse"])
def test_calculate_loss_trains_on_the_configured_objective(name, lib_built):
    """hip_train_loss = name: calculate_loss(batch).backward() against the same model's HIP prediction fed through the
    torch statement of that objective by autograd (the executor closure's route); the suite's 1e-4"""
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_train_loss=name)
    y = _labels_with_zeros(c)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": y.to(dev)}
    loss = m.calculate_loss(batch)
    assert loss.requires_grad
    loss.backward()
    got = _grads(m)
    m.zero_grad(set_to_none=True)
    sc = m._scaler
    want_loss = R.torch_loss(name, sc.inverse_transform(m.predict(batch)), sc.inverse_transform(batch["y"][..., 0:1]))
    want_loss.backward()
    want = _grads(m)
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-4 * abs(float(want_loss.detach()))
    bad = {k: max_norm_err(_host(got[k]), _host(want[k])) for k in want
           if float(want[k].abs().max()) > 0 and max_norm_err(_host(got[k]), _host(want[k])) > 1e-4}
    assert not bad, bad
    assert all(float(got[k].abs().max()) <= 1e-6 for k in want if float(want[k].abs().max()) == 0)
    with torch.no_grad():
        assert torch.equal(m.calculate_loss(batch), loss.detach())
        assert torch.equal(m.train_loss(batch, name), loss.detach())


@pytest.mark.parametrize("name", ["huber", "masked_mse"])
def test_resident_series_batch_gives_the_window_batch_bits(name, lib_built):
    from multistgraph_amd import windows as W
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_train_loss=name)
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 40
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, c.feat)).astype(F32)
    series[rng.random(series.shape) < 0.02] = F32(-MEAN / STD)
    starts = W.valid_label_starts(steps, rel, 24)
    pick = starts[rng.permutation(len(starts))[:c.b]].astype(np.int32)
    pick[-1] = starts[-1]                                        # the last valid start
    x, y = W.gather_windows(series, pick, rel, c.out)
    win = {"X": torch.from_numpy(x).to(dev), "y": torch.from_numpy(y).to(dev)}
    res = {"series": torch.from_numpy(series).to(dev), "label_start": torch.from_numpy(pick).to(dev), "rel_steps": rel}
    with torch.no_grad():
        a, b = m.calculate_loss(win), m.calculate_loss(res)
        assert torch.equal(a, b) and torch.isfinite(a)
        assert torch.equal(m.train_loss(res, name), a)
        assert not torch.equal(m.train_loss(res, "quantile", 0.9), a)
    la = m.calculate_loss(win)
    la.backward()
    ga = _grads(m)
    m.zero_grad(set_to_none=True)
    lb = m.calculate_loss(res)
    lb.backward()
    gb = _grads(m)
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(la.detach(), a)
    bad = {k: max_norm_err(_host(gb[k]), _host(ga[k])) for k in ga
           if float(ga[k].abs().max()) > 0 and max_norm_err(_host(gb[k]), _host(ga[k])) > 1e-4}
    assert not bad, bad


def test_default_leaves_calculate_loss_as_it_is(lib_built):
    """hip_train_loss = "none" is the model built without the key: loss and gradients bit for bit"""
    c = Case("tiny_multi_uni_c2")
    y = _labels_with_zeros(c)
    out = []
    for extra in ({}, {"hip_train_loss": "none"}):
        m, dev = _model(c, **extra)
        batch = {"X": torch.from_numpy(c.x).to(dev), "y": y.to(dev)}
        loss = m.calculate_loss(batch)
        loss.backward()
        out.append((loss.detach().clone(), _grads(m)))
    (l0, g0), (l1, g1) = out
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert any(float(g0[k].abs().max()) > 0 for k in g0)


def test_device_only(lib_built):
    """a scaler that is not affine has no device route: refused, like the other device-only methods"""
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_train_loss="huber")

    class Cubic:
        def inverse_transform(self, d):
            return d * d * d
    m._scaler = Cubic()
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            m.train_loss(batch, "mse")
        with pytest.raises(NotImplementedError):
            m.calculate_loss(batch)
