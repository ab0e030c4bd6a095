"""Conformal calibration on the GPU - matgcn_mc_conformity, matgcn_conformal_quantile, matgcn_conformal_coverage - against
the numpy reference (conformal_ref.py), and the surface above them: ops, evaluator.ConformalCalibrator,
MultiATGCN.calibrate_mc / predict_interval(calibrator=).

Bounds: none.  Scores and margins are compared with the reference bit for bit - np.array_equal after adding 0.0 to both
sides (only the sign of a zero is open; NaN equals NaN), counts exactly - and runs with each other on int32 views.  The
reference itself is held to the coverage promise in tests/test_conformal_host.py.
Shapes.  Scores: S = 2, 3, 32, 33, 257 (P = S and P > S, the 64- and 32-element tiles); geometries (B, out, N, od): one
element, a plain small one, 130 elements per row (three 64-wide tiles, the last with 2), Baltimore's 403 nodes.  Selection:
rows 1, 2, 255 .. 257 (around one histogram's worth), 1025; cols 1, 63 .. 65 (around the 64 columns of a workgroup), 403."""
import ctypes as C

import numpy as np
import pytest
import torch

import conformal_ref as CR
import mc_scores_ref as MC
import node_metrics_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = np.float32
PROBS = (0.05, 0.5, 0.95)
GEOMETRIES = ((1, 1, 1, 1), (3, 6, 21, 1), (2, 3, 65, 2), (2, 2, 403, 1))
GUARD = 256
POISON = 12345.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a + F32(0.0), b + F32(0.0), equal_nan=True)


# ---- scores -------------------------------------------------------------------------------------------------------------
def _samples(kind, s, geometry):
    rng = np.random.default_rng(1000 * s + 7 * sum(geometry))
    if kind == "normal":
        return rng.standard_normal((s,) + geometry).astype(F32)
    if kind == "ties":
        return (rng.integers(-3, 4, (s,) + geometry) / 2.0).astype(F32)
    return np.broadcast_to(rng.standard_normal(geometry).astype(F32), (s,) + geometry).copy()      # constant


def _real_scale(n):
    rng = np.random.default_rng(n)
    return dict(mean=rng.uniform(-2, 2, n).astype(F32), std=rng.uniform(0.5, 4, n).astype(F32),
                group_mean=rng.uniform(0, 3, n).astype(F32), group_std=rng.uniform(0.5, 2, n).astype(F32),
                clamp_min=0.0, truth_min=0.25, null_val=NAN, min_s=-1.0)


IDENTITY = dict(null_val=0.0, min_s=1e-4)


def _labels(x, geometry, on_band):
    """raw labels (B, out + 1, N, od + 1), scored channels y[:, :out, :, 1:]: random ones, tiny, zero and NaN ones and -
    ``on_band``, identity scale - ones exactly on Q_first, exactly on Q_last and inside the band"""
    b, out, n, od = geometry
    rng = np.random.default_rng(sum(geometry) + x.shape[0])
    y = (2.0 * rng.standard_normal((b, out + 1, n, od + 1))).astype(F32)
    core = y[:, :out, :, 1:]
    pick = rng.random(core.shape)
    if on_band:
        q = MC.quantiles(x, (PROBS[0], PROBS[-1]))
        mid = (q[0] + q[1]) * F32(0.5)
        for lo, hi, val in ((0.0, 0.15, q[0]), (0.15, 0.30, q[1]), (0.30, 0.50, mid)):
            sel = (pick >= lo) & (pick < hi)
            core[sel] = val[sel]
    core[(pick >= 0.50) & (pick < 0.55)] = 3e-5
    core[(pick >= 0.55) & (pick < 0.60)] = 0.0
    core[(pick >= 0.60) & (pick < 0.65)] = np.nan
    return y


def _guarded_scores(ops, xd, yd, geometry, **kw):
    """ops.mc_conformity into a poisoned buffer between two guards: every element written, no guard touched"""
    e = int(np.prod(geometry))
    flat = torch.full((GUARD + e + GUARD,), POISON, dtype=torch.float32, device="cuda:0")
    out = flat[GUARD:GUARD + e].view(geometry)
    got = ops.mc_conformity(xd, yd, PROBS, y_start=1, out=out, **kw)
    assert got.data_ptr() == out.data_ptr()
    assert bool((flat[:GUARD] == POISON).all()) and bool((flat[GUARD + e:] == POISON).all()), "a guard was written"
    assert not bool((out == POISON).any()), "an element was not written"
    return out


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=["x".join(map(str, g)) for g in GEOMETRIES])
@pytest.mark.parametrize("s", [2, 3, 32, 33, 257])
def test_scores_against_the_reference(s, geometry, lib_built):
    from multistgraph_amd import ops
    b, out, n, od = geometry
    zeros = negatives = nans = 0
    for kind in ("normal", "ties", "constant"):
        x = _samples(kind, s, geometry)
        xd = _dev(x)
        for name, kw in (("identity", IDENTITY), ("real", _real_scale(n))):
            y = _labels(x, geometry, on_band=name == "identity")
            want = CR.conformity(x, y[:, :out, :, 1:], PROBS, **kw)
            got = _guarded_scores(ops, xd, _dev(y), geometry, **kw)
            assert _same(_host(got), want), (kind, name, np.argwhere(~((_host(got) == want) | np.isnan(want)))[:5])
            assert torch.equal(_bits(ops.mc_conformity(xd, _dev(y), PROBS, y_start=1, **kw)), _bits(got))
            if name == "identity":
                zeros += int((want == 0).sum())
                negatives += int((want < 0).sum())
                nans += int(np.isnan(want).sum())
    if b * out * n * od > 100:
        assert zeros > 0 and negatives > 0 and nans > 0      # labels on the band's edge, inside it, masked


@pytest.mark.parametrize("s", [3, 257])
def test_scores_from_the_series(s, lib_built):
    """label_start rows give the bits of window labels"""
    from multistgraph_amd import ops
    geometry = b, out, n, od = (3, 6, 21, 1)
    rng = np.random.default_rng(s)
    series = rng.standard_normal((40, n, 3)).astype(F32)
    series[rng.random(series.shape) < 0.1] = 0.0
    x = _samples("normal", s, geometry)
    xd, sd = _dev(x), _dev(series)
    starts = np.array([0, 17, 40 - out], dtype=np.int32)
    windows = np.stack([series[t:t + out] for t in starts], 0)
    for kw in (IDENTITY, _real_scale(n)):
        a = ops.mc_conformity(xd, sd, PROBS, y_start=2, label_start=_dev(starts), **kw)
        w = ops.mc_conformity(xd, _dev(windows), PROBS, y_start=2, **kw)
        assert torch.equal(_bits(a), _bits(w))
        assert _same(_host(a), CR.conformity(x, windows[..., 2:], PROBS, **kw))
    with pytest.raises(Exception):
        ops.mc_conformity(xd, sd, (0.5,), y_start=2, label_start=_dev(starts))      # one level is no band


# ---- selection ------------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 255, 256, 257, 1025)
COLS = (1, 63, 64, 65, 403)
KINDS = ("continuous", "grid", "equal", "zeros", "inf", "nan_group", "single")
COVERAGES = (0.5, 0.8, 0.9, 1.0)


def _store(kind, rows, out, cols):
    """(2 * rows, out, cols): the scores in rows 0 .. rows - 1, behind them NaN-free garbage below every score - read, it
    would change every count and every margin"""
    rng = np.random.default_rng(rows * 1000 + cols * 10 + out)
    shape = (rows, out, cols)
    if kind == "grid":
        s = (rng.integers(-4, 5, shape) / 4.0).astype(F32)
    elif kind == "equal":
        s = np.full(shape, 1.5, dtype=F32)
    elif kind == "zeros":
        s = rng.choice(np.array([0.0, -0.0, 0.0, -0.0, 1e-40, -1e-40, 0.5, -0.5], dtype=F32), shape)
    else:
        s = rng.standard_normal(shape).astype(F32)
    if kind in ("continuous", "grid", "inf"):
        s[rng.random(shape) < 0.1] = np.nan
    if kind == "inf":
        pick = rng.random(shape)
        s[pick < 0.05] = np.inf
        s[pick > 0.95] = -np.inf
    if kind == "nan_group":
        s[:, 0, :] = np.nan
    if kind == "single":
        s[:, out - 1, :] = np.nan
        s[rows - 1, out - 1, cols - 1] = 0.75
    tail = (-1e30 - rng.random(shape) * 1e30).astype(F32)
    return np.concatenate([s, tail], 0)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_selection_against_the_reference(rows, cols, lib_built):
    from multistgraph_amd import ops
    for out in (1, 3):
        for kind in KINDS:
            store = _store(kind, rows, out, cols)
            sd = _dev(store)
            for grouping in ("horizon", "element"):
                wants = CR.quantile_many(store, rows, grouping, COVERAGES)
                for coverage, (want_m, want_c) in zip(COVERAGES, wants):
                    what = (kind, out, grouping, coverage)
                    margin, count = ops.conformal_quantile(sd, rows, grouping, coverage)
                    assert margin.dtype == torch.float32 and count.dtype == torch.int32
                    assert np.array_equal(_host(count), want_c), what
                    assert _same(_host(margin), want_m), (what, _host(margin).ravel()[:4], want_m.ravel()[:4])
                    opened = CR.ranks(want_c, coverage) > want_c                      # where k > n
                    assert np.isposinf(_host(margin))[opened].all(), what
                    if kind != "inf":      # (a +inf score can be the k-th smallest)
                        assert np.array_equal(np.isposinf(_host(margin)), opened), what
                    again, count2 = ops.conformal_quantile(sd, rows, grouping, coverage)
                    assert torch.equal(_bits(again), _bits(margin)) and torch.equal(count2, count), what
            if kind == "nan_group":
                m, c = ops.conformal_quantile(sd, rows, "element", 0.5)
                assert bool(torch.isinf(m[0]).all()) and int(c[0].sum()) == 0
            if kind == "single":
                m, c = ops.conformal_quantile(sd, rows, "horizon", 0.5)
                assert int(c[out - 1]) == 1 and float(m[out - 1]) == 0.75      # n = 1, k = 1


def test_selection_takes_the_store_as_the_calibrator_shapes_it(lib_built):
    """(rows, out, N, od): element margins come back as (out, N, od); a wrong row count or grouping is refused"""
    from multistgraph_amd import ops
    store = _store("continuous", 9, 2, 6).reshape(18, 2, 3, 2)
    sd = _dev(store)
    m, c = ops.conformal_quantile(sd, 9, "element", 0.8)
    assert tuple(m.shape) == (2, 3, 2) == tuple(c.shape)
    assert _same(_host(m), CR.quantile(store, 9, 1, 0.8)[0])
    m0, _ = ops.conformal_quantile(sd, 9, 0, 0.8)
    assert tuple(m0.shape) == (2,)
    for bad in (dict(rows=0), dict(rows=19), dict(grouping="node"), dict(coverage=0.0), dict(coverage=NAN)):
        kw = dict(rows=9, grouping="element", coverage=0.8)
        kw.update(bad)
        with pytest.raises(Exception):
            ops.conformal_quantile(sd, **kw)


# ---- coverage counts ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("rows", ROWS)
def test_coverage_counts(rows, cols, lib_built):
    from multistgraph_amd import ops
    cuts = sorted({0, rows // 3, rows - rows // 4, rows})
    for out in (1, 3):
        for kind in KINDS:
            store = _store(kind, rows, out, cols)
            sd = _dev(store)
            for grouping in ("horizon", "element"):
                what = (kind, out, grouping)
                margin, count = ops.conformal_quantile(sd, rows, grouping, 0.8)
                whole = ops.conformal_coverage(sd, rows, grouping, margin)
                assert whole.dtype == torch.int64 and tuple(whole.shape) == tuple(margin.shape) + (2,)
                assert np.array_equal(_host(whole), CR.coverage_counts(store, rows, grouping, _host(margin))), what
                assert torch.equal(whole[..., 0], count.long()), what
                # a score equal to the margin is covered: at least k of the n valid ones are
                k = CR.ranks(_host(count), 0.8)
                covered = _host(whole[..., 1])
                finite = np.isfinite(_host(margin))
                assert (covered[finite] >= k[finite]).all() and (covered <= _host(count)).all(), what
                run = None
                for lo, hi in zip(cuts[:-1], cuts[1:]):
                    run = ops.conformal_coverage(sd[lo:hi], hi - lo, grouping, margin, counts=run)
                assert torch.equal(run, whole), what
                assert torch.equal(ops.conformal_coverage(sd, rows, grouping, margin), whole), what
    with pytest.raises(Exception):
        ops.conformal_coverage(sd, rows, "element", torch.zeros(7, device="cuda:0"))      # not a margin per group


# ---- the calibrator ---------------------------------------------------------------------------------------------------------
def _calibration_batch(geometry, s=9, seed=0):
    b, out, n, od = geometry
    rng = np.random.default_rng(seed + sum(geometry))
    x = rng.standard_normal((s,) + geometry).astype(F32)
    y = (1.5 * rng.standard_normal((b, out + 1, n, od + 1))).astype(F32)
    y[:, :out, :, 1:][rng.random(geometry) < 0.1] = np.nan
    return x, y


@pytest.mark.parametrize("grouping", ["horizon", "element"])
def test_calibrator_batches_and_growth(grouping, lib_built):
    """B = 6 at once, three batches of 2, and a store growing 2 -> 4 -> 8 rows: the same store, margin and counts"""
    from multistgraph_amd.evaluator import ConformalCalibrator
    geometry = b, out, n, od = (6, 3, 65, 2)
    x, y = _calibration_batch(geometry)
    gm, gs = np.linspace(0.0, 2.0, n).astype(F32), np.linspace(0.5, 1.5, n).astype(F32)
    kw = dict(probs=(0.25, 0.5, 0.75), grouping=grouping, group_mean=gm, group_std=gs, s_small=0.25)
    xd, yd = _dev(x), _dev(y)
    whole = ConformalCalibrator({}, **kw)
    whole.collect_samples(xd, yd, 1, 0.5, 2.0)
    assert tuple(whole._store.shape) == (256, out, n, od) and whole._rows == 6
    pieces, small = ConformalCalibrator({}, **kw), ConformalCalibrator({}, capacity=2, **kw)
    for lo in (0, 2, 4):
        for cal in (pieces, small):
            cal.collect_samples(xd[:, lo:lo + 2].contiguous(), yd[lo:lo + 2], 1, 0.5, 2.0)
    small.collect_samples(xd[:, :2].contiguous(), yd[:2], 1, 0.5, 2.0)                # rows 6, 7: the store is full at 8
    assert tuple(small._store.shape) == (8, out, n, od) and small._rows == 8
    assert torch.equal(_bits(small._store[6:8]), _bits(small._store[0:2]))
    want = CR.conformity(x, y[:, :out, :, 1:], kw["probs"], mean=0.5, std=2.0, group_mean=gm, group_std=gs, clamp_min=0.0,
                         truth_min=0.25, null_val=NAN, min_s=-1.0)
    for cal in (whole, pieces, small):
        assert _same(_host(cal._store[:6]), want)
        assert torch.equal(_bits(cal._store[:6]), _bits(whole._store[:6]))
    small._rows = 6
    want_m, want_c = CR.quantile(want, 6, grouping, CR.coverage_of(kw["probs"]))
    for cal in (whole, pieces, small):
        margin, count = cal.fit()
        assert _same(_host(margin), want_m) and np.array_equal(_host(count), want_c)
        assert tuple(margin.shape) == ((out,) if grouping == "horizon" else (out, n, od))
    with pytest.raises(ValueError):
        whole.collect_samples(xd, yd, 1, 0.5, 3.0)                                   # another scale than the first batch's
    # the test split, streamed: coverage of the calibration rows themselves is at least k / n in every finite group
    for lo in (0, 2, 4):
        pieces.collect_test_samples(xd[:, lo:lo + 2].contiguous(), yd[lo:lo + 2], 1, 0.5, 2.0)
    whole.collect_test_samples(xd, yd, 1, 0.5, 2.0)
    assert torch.equal(pieces._test_counts, whole._test_counts)
    assert np.array_equal(_host(whole._test_counts), CR.coverage_counts(want, 6, grouping, want_m))
    table, result = whole.coverage_table(), whole.evaluate()
    assert tuple(table.shape) == tuple(want_m.shape) and table.dtype == torch.float64
    counts = CR.coverage_counts(want, 6, grouping, want_m).reshape(out, -1, 2).sum(1)
    inf = np.isinf(want_m).reshape(out, -1).sum(1)
    for o in range(out):
        assert result["PICP@%d" % (o + 1)] == counts[o, 1] / counts[o, 0]
        assert result["INF_MARGINS@%d" % (o + 1)] == inf[o]
    # a checkpoint: the state loaded into a fresh calibrator applies the same margin
    fresh = ConformalCalibrator({})
    fresh.load_state_dict(whole.state_dict())
    band = torch.sort(torch.randn(3, 2, out, n, od, device="cuda:0"), 0).values
    assert torch.equal(_bits(fresh.apply(band)), _bits(whole.apply(band)))


def test_calibrator_apply(lib_built):
    from multistgraph_amd.evaluator import ConformalCalibrator
    out, n, od = 2, 3, 1
    band = _dev(np.sort(np.random.default_rng(1).uniform(0.5, 3.0, (3, 4, out, n, od)).astype(F32), 0))
    for grouping, margin in (("horizon", np.array([0.75, np.inf], dtype=F32)),
                             ("element", np.array([[[0.75], [-0.125], [np.inf]], [[4.0], [0.0], [1e-3]]], dtype=F32))):
        for clamp in (NAN, 0.0):
            cal = ConformalCalibrator({}, grouping=grouping)
            cal.margin, cal.clamp_min = _dev(margin), clamp
            got = cal.apply(band)
            assert got.data_ptr() != band.data_ptr() and torch.equal(got[1], band[1])            # a copy; inner level kept
            want = CR.apply_margin(_host(band), margin, grouping, clamp)
            assert np.array_equal(_host(got), want)
            m = np.broadcast_to(margin.reshape(-1, 1, 1) if grouping == "horizon" else margin, (out, n, od))
            assert np.isposinf(_host(got)[2][:, np.isinf(m)]).all()                                # an infinite margin stays
            low = _host(got)[0][:, np.isinf(m)]
            assert (low == 0).all() if clamp == 0.0 else np.isneginf(low).all()
            if clamp == 0.0:
                assert float(got[0].min()) >= 0.0 and bool((got[0] == 0).any())
        with pytest.raises(ValueError):
            cal.apply(band[:2])


# ---- the model surface --------------------------------------------------------------------------------------------------
def _tiny_model(batch):
    from helpers import Case
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    assert c.feat == 2
    dev = torch.device("cuda:0")
    cfg = c.config("cuda:0")
    cfg["batch_size"] = batch
    model = MultiATGCN(cfg, c.data_feature).to(dev).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    return c, model


def _tiny_batches(c, batch):
    """the same ``batch`` windows as a window batch and as a resident-series batch, and the windows' labels"""
    from multistgraph_amd import windows as W
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, 2)).astype(F32)
    series[rng.random(series.shape) < 0.05] = 0.0
    pick = W.valid_label_starts(steps, rel, 24)[:batch].astype(np.int32)
    xw, yw = W.gather_windows(series, pick, rel, c.out)
    return {"X": _dev(xw), "y": _dev(yw)}, {"series": _dev(series), "label_start": _dev(pick)}, yw


def test_predict_interval_and_calibrate_mc(lib_built):
    from multistgraph_amd import ops
    from multistgraph_amd.evaluator import ConformalCalibrator
    batch, s, seed = 3, 8, 11
    c, model = _tiny_model(batch)
    wb, sb, yw = _tiny_batches(c, batch)
    levels = (0.25, 0.5, 0.75)      # coverage 0.5: k = ceil(4 * 0.5) = 2 <= n = 3 (0.05 / 0.95 would give k = 4 > n)
    # without a calibrator: what it was - the quantiles of predict_mc's samples
    mean, std, band = model.predict_interval(wb, samples=s, probs=levels, seed=seed)
    m0, s0, kept = model.predict_mc(wb, samples=s, seed=seed, keep_samples=True)
    assert torch.equal(_bits(band), _bits(ops.mc_quantiles(kept, levels)))
    assert torch.equal(_bits(mean), _bits(m0)) and torch.equal(_bits(std), _bits(s0))
    none = model.predict_interval(wb, samples=s, probs=levels, seed=seed, calibrator=None)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(none, (mean, std, band)))

    fitted = {}
    for grouping in ("horizon", "element"):
        cals = []
        for b in (wb, sb):
            cal = ConformalCalibrator({}, probs=levels, grouping=grouping)
            with pytest.raises(ValueError):
                model.predict_interval(b, samples=s, probs=levels, seed=seed, calibrator=cal)      # not fitted
            assert torch.equal(model.calibrate_mc(b, cal, samples=s, seed=seed), kept)
            cal.fit()
            cals.append(cal)
        win, ser = cals
        assert torch.equal(_bits(win._store[:batch]), _bits(ser._store[:batch]))
        assert torch.equal(_bits(win.margin), _bits(ser.margin)) and torch.equal(win.count, ser.count)
        scores = CR.conformity(_host(kept), yw[:, :c.out, :, :1], levels, mean=0.0, std=1.0, null_val=0.0, min_s=1e-4)
        assert _same(_host(win._store[:batch]), scores)
        margin, count = CR.quantile(scores, batch, grouping, CR.coverage_of(levels))
        assert _same(_host(win.margin), margin) and np.array_equal(_host(win.count), count)
        # the calibrated band is apply() of the uncalibrated one, from both kinds of batch
        got = model.predict_interval(wb, samples=s, probs=levels, seed=seed, calibrator=win)
        assert torch.equal(_bits(got[2]), _bits(win.apply(band))) and torch.equal(_bits(got[0]), _bits(mean))
        from_series = model.predict_interval(sb, samples=s, probs=levels, seed=seed, calibrator=ser)
        assert torch.equal(_bits(from_series[2]), _bits(got[2]))
        assert _same(_host(got[2]), CR.apply_margin(_host(band), margin, grouping))
        fitted[grouping] = (win, got[2], scores, margin, count)
        # counted as a test batch: the calibration rows against their own margin
        model.calibrate_mc(sb, win, samples=s, seed=seed, test=True)
        assert np.array_equal(_host(win._test_counts), CR.coverage_counts(scores, batch, grouping, margin))

    # per element, every group with k <= n: exactly the labels the margin covers lie inside the calibrated band
    win, cband, scores, margin, count = fitted["element"]
    lo, hi = _host(cband[0]), _host(cband[-1])
    l, keep = CR.labels_nodes(yw[:, :c.out, :, :1], mean=0.0, std=1.0, null_val=0.0, min_s=1e-4)
    assert np.array_equal(keep, ~np.isnan(scores)) and keep.sum() > 0.8 * keep.size
    finite = np.broadcast_to(np.isfinite(margin), l.shape) & keep
    assert finite.sum() > 0 and (count[np.isfinite(margin)] >= 2).all()
    # A label whose score IS the margin sits on the calibrated edge up to the rounding of Q -+ m (fl(Q - fl(Q - l)) need
    # not be l): within 2^-22 of the larger operand there it counts as on the edge; everywhere else the test is exact.
    with np.errstate(invalid="ignore"):
        covered = scores <= margin
        tol = 2.0 ** -22 * np.maximum(np.maximum(np.abs(lo), np.abs(hi)), np.abs(l) + np.abs(margin))
        edge = np.abs(scores.astype(np.float64) - margin) <= tol
        inside = (lo <= l) & (l <= hi)
        near = (lo - tol <= l) & (l <= hi + tol)
    off = finite & ~edge
    assert np.array_equal(inside[off], covered[off]) and off.sum() > 0.5 * finite.sum()
    assert near[finite & covered].all()                                             # every covered label, edge ones included
    assert covered[finite].sum() >= 2 * np.isfinite(margin).sum()                   # k = 2 labels of every finite group

    # a calibrator for other levels or another scale is refused
    win = fitted["horizon"][0]
    with pytest.raises(ValueError):
        model.predict_interval(wb, samples=s, probs=(0.05, 0.5, 0.95), seed=seed, calibrator=win)
    with pytest.raises(ValueError):
        model.predict_interval(wb, samples=s, probs=levels, seed=seed, clamp_min=0.0, calibrator=win)
    gm, gs = np.zeros(c.n, dtype=F32), np.ones(c.n, dtype=F32)
    with pytest.raises(ValueError):
        model.predict_interval(wb, samples=s, probs=levels, seed=seed, group_mean=gm, group_std=gs, calibrator=win)
    # the re-transformed route: a calibrator on that scale, fitted and applied
    group = ConformalCalibrator({}, probs=levels, grouping="element", group_mean=gm + 1.0, group_std=gs * 2.0)
    model.calibrate_mc(wb, group, samples=s, seed=seed)
    group.fit()
    kw = dict(group_mean=gm + 1.0, group_std=gs * 2.0, clamp_min=0.0)
    plain = model.predict_interval(wb, samples=s, probs=levels, seed=seed, **kw)[2]
    got = model.predict_interval(wb, samples=s, probs=levels, seed=seed, calibrator=group, **kw)[2]
    assert torch.equal(_bits(got), _bits(group.apply(plain))) and float(got[0].min()) >= 0.0
    want = CR.conformity(_host(kept), yw[:, :c.out, :, :1], levels, mean=0.0, std=1.0, group_mean=gm + 1.0,
                         group_std=gs * 2.0, clamp_min=0.0, null_val=NAN, min_s=-1.0)
    assert _same(_host(group._store[:batch]), want)
