"""matgcn_mc_quantiles / matgcn_mc_scores on the GPU against the numpy reference (mc_scores_ref.py), and the surface above
them: ops.mc_quantiles / mc_scores, ProbabilisticEvaluator, MultiATGCN.predict_interval / score_mc.

Bounds: quantiles np.array_equal after adding 0.0 to both sides (every operation is one float32 rounding on both sides; only
the sign of a zero is left open).  Count and covered sums exact.  Every other sum within 1e-10 of the sum of its terms'
magnitudes: each term is defined bit for bit up to the order of its own S-term fp64 sums (relative 2^-53 * S at worst), and
the terms of a horizon are then added in another order than numpy's - fp64 summation-order noise only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import mc_scores_ref as R

pytestmark = pytest.mark.gpu

SAMPLES = (1, 2, 3, 31, 32, 33, 100, 257, 1024)
GEOMETRIES = ((1, 1, 1, 1), (3, 6, 21, 1), (2, 3, 65, 2), (2, 2, 403, 1))
KINDS = ("normal", "ties", "constant", "ascending", "descending")
LEVELS = (0.0, 0.05, 0.5, 0.95, 1.0)
PROBS = (0.05, 0.5, 0.95)
SCALE = dict(mean=-1.25, std=3.5)
NAN = float("nan")
SUM_TOL = 1e-10
GUARD = 256


def _dev():
    return torch.device("cuda:0")


def _samples(kind, s, geometry, seed=0):
    rng = np.random.default_rng(1000 * s + 7 * sum(geometry) + seed)
    x = rng.standard_normal((s,) + geometry).astype(np.float32)
    if kind == "ties":
        x = np.round(x, 1).astype(np.float32)
    elif kind == "constant":
        x = np.broadcast_to(x[:1], x.shape).copy()
    elif kind == "ascending":
        x = np.sort(x, axis=0)
    elif kind == "descending":
        x = np.sort(x, axis=0)[::-1].copy()
    return x


def _raw_labels(geometry, seed, on_quantiles=None, nans=False):
    """raw labels (B, out + 1, N, od + 1): the scored channels are y[:, :out, :, 1:] (y_start = 1).  About 10 % are 0, a
    few are tiny (|l| < min_s), a few sit exactly on the outer quantiles (identity scale only), a few are NaN."""
    b, out, n, od = geometry
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, out + 1, n, od + 1)).astype(np.float32)
    core = y[:, :out, :, 1:]
    pick = rng.random(core.shape)
    if on_quantiles is not None:
        core[pick < 0.30] = on_quantiles[0][pick < 0.30]
        core[pick < 0.15] = on_quantiles[1][pick < 0.15]
    core[(pick >= 0.30) & (pick < 0.40)] = 0.0
    core[(pick >= 0.40) & (pick < 0.45)] = 3e-5
    if nans:
        core[(pick >= 0.45) & (pick < 0.55)] = np.nan
    return y


def _check_sums(got, want, mag, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, 0], want[:, 0]), "%s: count" % (what,)
    assert np.array_equal(got[:, 2], want[:, 2]), "%s: covered" % (what,)
    err = np.abs(got - want)
    assert (err <= SUM_TOL * mag).all(), "%s: worst error %.3e of %.3e" % (what, err.max(), mag.max())


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("s", SAMPLES)
def test_quantiles_and_scores_against_the_reference(s, geometry, lib_built):
    from multistgraph_amd.ops import mc_quantiles, mc_scores
    dev = _dev()
    b, out, n, od = geometry
    for kind in KINDS:
        x = _samples(kind, s, geometry)
        xd = torch.from_numpy(x).to(dev)
        what = (kind, s, geometry)
        sorted_by_scale = {}
        # ---- quantiles, identity scale and a real one
        for scale in (dict(mean=0.0, std=1.0), SCALE):
            xs = sorted_by_scale[scale["std"]] = R.sorted_samples(x, **scale)
            want = R.quantiles_sorted(xs, LEVELS)
            first = mc_quantiles(xd, LEVELS, **scale)
            assert tuple(first.shape) == (len(LEVELS),) + geometry and first.dtype == torch.float32
            got = first.cpu().numpy()
            assert np.array_equal(got + 0.0, want + 0.0), what
            assert np.array_equal(got[0] + 0.0, xs[0] + 0.0) and np.array_equal(got[-1] + 0.0, xs[-1] + 0.0), what
            assert torch.equal(mc_quantiles(xd, LEVELS, **scale).view(torch.int32), first.view(torch.int32)), what
        # ---- scores: identity scale, null value 0, labels on the outer quantiles
        q = R.quantiles_sorted(sorted_by_scale[1.0], PROBS)
        y = _raw_labels(geometry, 11 + s, on_quantiles=(q[0], q[-1]))
        core = y[:, :out, :, 1:]
        want, mag = R.score_sums(x, core, PROBS)
        yd = torch.from_numpy(y).to(dev)
        got = mc_scores(xd, yd, PROBS, y_start=1)
        _check_sums(got, want, mag, what)
        assert torch.equal(got, mc_scores(xd, yd, PROBS, y_start=1)), what
        if kind == "constant":      # the interval is one point and the labels on it are inside: <= on both ends
            l, mask = R.labels(core)
            assert want[:, 2].sum() == (mask & (l == q[0])).sum()
        # ---- scores: de-scaled, NaN null value and NaN labels
        y = _raw_labels(geometry, 13 + s, nans=True)
        want, mag = R.score_sums(x, y[:, :out, :, 1:], PROBS, null_val=NAN, **SCALE)
        got = mc_scores(xd, torch.from_numpy(y).to(dev), PROBS, y_start=1, null_val=NAN, **SCALE)
        _check_sums(got, want, mag, what + ("nan",))


def test_labels_on_the_interval_ends_are_covered(lib_built):
    """every label exactly on Q_first or Q_last: all covered"""
    from multistgraph_amd.ops import mc_scores
    geometry, s = (2, 3, 65, 2), 33
    x = _samples("normal", s, geometry) + np.float32(4.0)      # away from the null value 0
    q = R.quantiles(x, PROBS)
    y = np.where(np.random.default_rng(3).random(geometry) < 0.5, q[0], q[-1]).astype(np.float32)
    got = mc_scores(torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev()), PROBS).cpu().numpy()
    assert np.array_equal(got[:, 0], np.full(3, 2 * 65 * 2.0)) and np.array_equal(got[:, 2], got[:, 0])


@pytest.mark.parametrize("probs", [LEVELS, (0.5,), (0.01, 0.1, 0.25, 0.4, 0.6, 0.75, 0.9, 0.99)], ids=["alpha0", "one", "eight"])
def test_other_level_sets(probs, lib_built):
    """alpha = 0 (levels 0 and 1 as the interval): the Winkler sum is the width sum; one level; eight levels"""
    from multistgraph_amd.ops import mc_scores
    geometry, s = (2, 3, 65, 2), 100
    x = _samples("normal", s, geometry)
    y = _raw_labels(geometry, 5)
    want, mag = R.score_sums(x, y[:, :3, :, 1:], probs, **SCALE)
    got = mc_scores(torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev()), probs, y_start=1, **SCALE)
    _check_sums(got, want, mag, probs)
    if probs == LEVELS:
        assert torch.equal(got[:, 4], got[:, 3])


@pytest.mark.parametrize("s", [3, 257])
def test_series_labels_equal_window_labels(s, lib_built):
    from multistgraph_amd.ops import mc_scores
    dev = _dev()
    geometry = b, out, n, od = (3, 6, 21, 1)
    rng = np.random.default_rng(s)
    series = rng.standard_normal((40, n, 3)).astype(np.float32)
    series[rng.random(series.shape) < 0.1] = 0.0
    starts = np.array([0, 17, 40 - out], dtype=np.int32)
    windows = np.stack([series[t:t + out] for t in starts], 0)
    xd = torch.from_numpy(_samples("ties", s, geometry)).to(dev)
    a = mc_scores(xd, torch.from_numpy(series).to(dev), PROBS, y_start=2, label_start=torch.from_numpy(starts).to(dev), **SCALE)
    w = mc_scores(xd, torch.from_numpy(windows).to(dev), PROBS, y_start=2, **SCALE)
    assert torch.equal(a, w) and float(a[:, 0].sum()) > 0


def test_accumulation(lib_built):
    from multistgraph_amd.ops import mc_scores
    dev = _dev()
    geometry, s = (2, 3, 65, 2), 33
    xa, xb = (torch.from_numpy(_samples("normal", s, geometry, seed)).to(dev) for seed in (1, 2))
    ya, yb = (torch.from_numpy(_raw_labels(geometry, seed)).to(dev) for seed in (3, 4))
    a = mc_scores(xa, ya, PROBS, y_start=1, **SCALE)
    b = mc_scores(xb, yb, PROBS, y_start=1, **SCALE)
    both = mc_scores(xb, yb, PROBS, y_start=1, sums=a.clone(), **SCALE)
    assert torch.equal(both, a + b)
    twice = mc_scores(xa, ya, PROBS, y_start=1, sums=a.clone(), **SCALE)
    assert torch.equal(twice[:, 0], 2 * a[:, 0]) and torch.equal(twice, a + a)
    with pytest.raises(Exception):
        mc_scores(xa, ya, PROBS, y_start=1, sums=torch.zeros(3, 5, dtype=torch.float64, device=dev))


def _guarded(n, dtype, dev):
    """n elements of NaN to be written, GUARD elements of NaN behind them that must stay"""
    return torch.full((n + GUARD,), NAN, dtype=dtype, device=dev)


def _untouched(buf, n):
    return bool(torch.isnan(buf[n:]).all())


@pytest.mark.parametrize("s,geometry", [(33, (2, 3, 65, 2)), (1024, (3, 6, 21, 1)), (257, (2, 2, 403, 1))])
def test_prefilled_buffers_and_guards(s, geometry, lib_built):
    """scratch and outputs full of NaN: the same results, and nothing behind the outputs or the scratch is written"""
    from multistgraph_amd import _lib
    from multistgraph_amd.ops import mc_quantiles, mc_scores
    lib, dev = _lib.load(), _dev()
    b, out, n, od = geometry
    elems = b * out * n * od
    x = torch.from_numpy(_samples("ties", s, geometry)).to(dev)
    y = torch.from_numpy(_raw_labels(geometry, 21)).to(dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    levels = (C.c_float * len(LEVELS))(*LEVELS)
    q = _guarded(len(LEVELS) * elems, torch.float32, dev)
    _lib.check(lib.matgcn_mc_quantiles(C.c_void_p(x.data_ptr()), s, elems, levels, len(LEVELS), SCALE["mean"], SCALE["std"],
                                       C.c_void_p(q.data_ptr()), stream), "matgcn_mc_quantiles")
    want = mc_quantiles(x, LEVELS, **SCALE)
    assert torch.equal(q[:len(LEVELS) * elems].view(torch.int32), want.reshape(-1).view(torch.int32)) and _untouched(q, want.numel())

    need = C.c_size_t(0)
    _lib.check(lib.matgcn_mc_scores_bytes(b, out, n, od, s, len(PROBS), C.byref(need)), "matgcn_mc_scores_bytes")
    cols = 5 + len(PROBS)
    scratch = _guarded(need.value // 8, torch.float64, dev)
    sums = _guarded(out * cols, torch.float64, dev)
    probs = (C.c_float * len(PROBS))(*PROBS)
    _lib.check(lib.matgcn_mc_scores(C.c_void_p(x.data_ptr()), s, C.c_void_p(y.data_ptr()), None, b, out, n, od, out + 1, od + 1,
                                    1, SCALE["mean"], SCALE["std"], 0.0, 1e-4, probs, len(PROBS),
                                    C.c_void_p(scratch.data_ptr()), need.value, C.c_void_p(sums.data_ptr()), 0, stream),
               "matgcn_mc_scores")
    want = mc_scores(x, y, PROBS, y_start=1, **SCALE)
    assert torch.equal(sums[:out * cols].reshape(out, cols), want) and not torch.isnan(want).any()
    assert _untouched(sums, out * cols) and _untouched(scratch, need.value // 8)
    assert not torch.isnan(scratch[:need.value // 8]).any()      # every partial is written, none is left over


# ---- the model surface ---------------------------------------------------------------------------------------------------
OUT = 6


def _model(nodes, batch, scaler=None, **flags):
    """a synthetic model of `nodes` nodes through the plugin class (closed-form parameters, synthetic inputs, the host graph
    prep's static supports); rnn_units < 64 is padded to the kernels' 64 channels by the class"""
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd.model import MultiATGCN
    dev = _dev()
    seed = 3
    df = syn.make_data_feature(nodes, seed, "DC", ext_dim=1, scaler=scaler)
    cfg = dict(input_window=24, output_window=OUT, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
               adjtype="multi", adpadj="unidirection", cheb_order=2, embed_dim_node=20, embed_dim_adj=20, rnn_units=64,
               num_layers=2, device=dev, batch_size=batch, start_dim=0, end_dim=1)
    cfg.update(flags)
    shapes = syn.param_shapes(nodes, out_steps=OUT, feat_in=2, k_total=syn.k_total_for("multi", "unidirection", 2), **flags)
    model = MultiATGCN(cfg, df).to(dev).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.closed_form_state(shapes, seed).items()})
    x, y = syn.make_batch_arrays(batch, nodes, OUT, seed, feat=2)
    return model, torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)


@pytest.mark.parametrize("flags", [{}, {"rnn_units": 32}], ids=["h64", "h32"])
def test_predict_interval(flags, lib_built):
    nodes, batch, s = 48, 3, 33
    model, x, _ = _model(nodes, batch, **flags)
    mean, std, q = model.predict_interval({"X": x}, samples=s, probs=LEVELS, seed=5)
    mean2, std2, kept = model.predict_mc({"X": x}, samples=s, seed=5, keep_samples=True)
    assert torch.equal(mean.view(torch.int32), mean2.view(torch.int32))
    assert torch.equal(std.view(torch.int32), std2.view(torch.int32))
    assert tuple(q.shape) == (len(LEVELS), batch, OUT, nodes, 1)
    want = R.quantiles(kept.cpu().numpy(), LEVELS)
    assert np.array_equal(q.cpu().numpy() + 0.0, want + 0.0)
    assert float((q[-1] - q[0]).min()) >= 0 and float((q[-1] - q[0]).max()) > 0
    assert model._dropout_counter == 0


def test_predict_interval_from_the_series(lib_built):
    from multistgraph_amd import windows as W
    nodes, batch, s = 48, 3, 8
    model, _, _ = _model(nodes, batch)
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, nodes, 2)).astype(np.float32)
    pick = W.valid_label_starts(steps, rel, 24)[:batch].astype(np.int32)
    sb = {"series": torch.from_numpy(series).to(_dev()), "label_start": torch.from_numpy(pick).to(_dev())}
    xw, yw = W.gather_windows(series, pick, rel, OUT)
    wb = {"X": torch.from_numpy(xw).to(_dev()), "y": torch.from_numpy(yw).to(_dev())}
    a, b = model.predict_interval(sb, samples=s, seed=2), model.predict_interval(wb, samples=s, seed=2)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(model.score_mc(sb, samples=s, probs=PROBS, seed=2), model.score_mc(wb, samples=s, probs=PROBS, seed=2))


def test_score_mc_and_the_evaluator_over_two_batches(lib_built):
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd.evaluator import ProbabilisticEvaluator
    nodes, batch, s = 48, 3, 33
    model, x, y = _model(nodes, batch, scaler=syn.PlainScaler(SCALE["mean"], SCALE["std"]))
    x2, y2 = x.flip(0).contiguous(), (0.5 * y).flip(0).contiguous()
    y2[0, :, :5, 0] = -SCALE["mean"] / SCALE["std"]      # a few labels that de-scale to (almost) 0: masked
    ev = ProbabilisticEvaluator({"min_s": 1e-4}, probs=PROBS)
    sums = None
    kept = []
    for seed, (xb, yb) in enumerate(((x, y), (x2, y2))):
        batch_d = {"X": xb, "y": yb}
        sums = model.score_mc(batch_d, samples=s, probs=PROBS, seed=seed, sums=sums)
        k = model.predict_mc(batch_d, samples=s, seed=seed, keep_samples=True)[2]
        ev.collect_samples(k, yb, model.start_dim, SCALE["mean"], SCALE["std"])
        kept.append(k.cpu().numpy())
    want, mag = R.score_sums(np.concatenate(kept, 1), torch.cat([y, y2], 0)[..., :1].cpu().numpy(), PROBS, **SCALE)
    _check_sums(sums, want, mag, "score_mc")
    assert torch.equal(ev._sums, sums) and float(sums[:, 0].sum()) < 2 * batch * OUT * nodes     # some labels are masked
    table = ev.table()
    assert tuple(table.shape) == (OUT, 4 + len(PROBS))
    assert torch.equal(table, (sums[:, 1:] / sums[:, :1]).cpu())
    got = sums.cpu().numpy()
    res = ev.evaluate()
    assert set(res) == {"%s@%d" % (c, i) for c in ev.columns for i in range(1, OUT + 1)}
    assert res["PICP@1"] == got[0, 2] / got[0, 0] == want[0, 2] / want[0, 0] and 0.0 <= res["PICP@1"] <= 1.0
    ev.clear()
    with pytest.raises(RuntimeError):
        ev.table()
    # a horizon without an unmasked label reports NaN
    ev.collect_samples(torch.from_numpy(kept[0]).to(_dev()), torch.zeros_like(y), 0, None, None)
    assert np.isnan(ev.table().numpy()).all()

    class _Log:
        def inverse_transform(self, data):
            return torch.exp(data)
    model._scaler = _Log()
    with pytest.raises(NotImplementedError):
        model.score_mc({"X": x, "y": y}, samples=4, probs=PROBS, seed=1)
