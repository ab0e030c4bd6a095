"""The per-node evaluation entry points on the GPU - matgcn_metric_sums_nodes, matgcn_metric_table_rows,
matgcn_mc_scores_nodes, matgcn_mc_quantiles_scaled - against the numpy reference (node_metrics_ref.py), and the surface
above them: ops, evaluator.NodeEvaluator, MultiATGCN.collect_node_metrics / score_mc_nodes / predict_interval.

Bounds.
  * Metric sums, grid-valued inputs (metrics_ref.grid_case: no float32 operation rounds, every float64 sum is exact): what
    tests/test_loss_metrics_edges.py holds the per-horizon sums to - sums 0-3, 5-7, 9-13 bit-equal to the reference, sums 4
    and 8 (one float32 quotient per term) within 2^-22 of it, inf == inf.
  * Scores: what tests/test_mc_scores.py holds the per-horizon sums to - count and covered exact, every other sum within
    1e-10 of the sum of its terms' magnitudes (the terms' own S-term fp64 sums; the order the terms are added in is the
    reference's here).
  * Quantiles: np.array_equal after adding 0.0 to both sides (only the sign of a zero is open).
  * Streaming, repetition, dirty buffers, window against series batches: torch.equal.
Shapes (B, out, N, od): one element; a plain small one; 130 elements per row (three 64-wide tiles, the last with 2); od = 3
with node 21's channels across the 64-element tile border; more batch rows than a wave; the 64-horizon limit; Baltimore's 403
nodes.  S = 1, 33, 257, 1024 covers the three tile widths (64, 32, 16 elements)."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as M
import node_metrics_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
GEOMETRIES = ((1, 1, 1, 1), (3, 6, 21, 1), (2, 3, 65, 2), (2, 2, 22, 3), (65, 2, 5, 1), (2, 64, 3, 1), (2, 2, 403, 1))
GEOMETRY_IDS = ["x".join(map(str, g)) for g in GEOMETRIES]
EXACT_COLS = [0, 1, 2, 3, 5, 6, 7, 9, 10, 11, 12, 13]
QUOT_COLS = [4, 8]
QUOT_TOL = 2.0 ** -22
SUM_TOL = 1e-10
PROBS = (0.05, 0.5, 0.95)
GUARD = 256
# descriptor routes of the metric sums: (per-node first affine, group affine, clamp_min, truth_min, min_s, swap_r2)
ROUTES = {
    "scalar": (False, False, NAN, NAN, M.EXACT_MIN_S, False),
    "pernode": (True, False, NAN, NAN, M.EXACT_MIN_S, False),
    "groupstd": (False, True, M.EXACT_CLAMP_MIN, M.EXACT_TRUTH_MIN, -1.0, True),
    "all": (True, True, M.EXACT_CLAMP_MIN, M.EXACT_TRUTH_MIN, M.EXACT_MIN_S, False),
}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _equal_nan(a, b):
    """torch.equal with NaN == NaN"""
    return a.shape == b.shape and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def _same(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _violations(reset=1):
    from multistgraph_amd import _lib
    cnt = C.c_int64()
    _lib.check(_lib.load().matgcn_series_violations(C.byref(cnt), reset), "matgcn_series_violations")
    return int(cnt.value)


# ---- metric sums ----------------------------------------------------------------------------------------------------------
def _grid(geometry, per_node, seed=0):
    """a grid case with labels in the middle of the feature axis and a spare label row; node 0's labels below every
    truth_min, the last node's all NaN, a few more NaN (N >= 3)"""
    b, out, n, od = geometry
    c = M.grid_case(100 + seed + sum(geometry), b, out, n, od, y_steps=out + 1, y_feat=od + 2, y_start=1, per_node=per_node,
                    group=True)
    M.assert_exact(c, clamp_min=M.EXACT_CLAMP_MIN, min_s=M.EXACT_MIN_S)
    if n >= 3:
        rng = np.random.default_rng(seed)
        core = c["y"][:, :out, :, 1:1 + od]
        core[rng.random(core.shape) < 0.05] = np.nan
        core[:, :, 0, :] = -4.0
        core[:, :, n - 1, :] = np.nan
    return c


def _metric_kw(c, route):
    per_node, group, clamp, truth, min_s, _ = ROUTES[route]
    assert per_node == (np.ndim(c["mean"]) == 1)
    gm, gs = (c["group_mean"], c["group_std"]) if group else (None, None)
    return dict(mean=c["mean"], std=c["std"], group_mean=gm, group_std=gs, clamp_min=clamp, truth_min=truth, min_s=min_s)


def _metric_ref(c, kw, label_start=None, start=None):
    return R.metric_sums_nodes_ref(c["pred"], c["y"], c["y_start"], kw["mean"], kw["std"], kw["group_mean"], kw["group_std"],
                                   kw["clamp_min"], kw["truth_min"], kw["min_s"], label_start, start)


def _assert_metric_sums(got, want):
    got, want = np.asarray(got).reshape(-1, 14), np.asarray(want).reshape(-1, 14)
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = np.argwhere(~_same(got[:, EXACT_COLS], want[:, EXACT_COLS]))
    assert bad.size == 0, ("exact sums differ at (row, index into EXACT_COLS)", bad[:5].tolist(), got[bad[0][0]].tolist(),
                           want[bad[0][0]].tolist())
    g, w = got[:, QUOT_COLS], want[:, QUOT_COLS]
    with np.errstate(invalid="ignore"):
        ok = _same(g, w) | (np.abs(g - w) <= QUOT_TOL * w)
    assert ok.all(), ("quotient sums", np.argwhere(~ok)[:5].tolist(), g[~ok][:5], w[~ok][:5])


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=GEOMETRY_IDS)
def test_metric_sums_per_node_against_the_reference(geometry, lib_built):
    from multistgraph_amd import ops
    b, out, n, od = geometry
    for route, (per_node, *_rest) in ROUTES.items():
        c = _grid(geometry, per_node)
        kw = _metric_kw(c, route)
        got = ops.metric_sums_nodes(_dev(c["pred"]), _dev(c["y"]), c["y_start"], **kw)
        assert tuple(got.shape) == (out, n, 14) and got.dtype == torch.float64
        want = _metric_ref(c, kw)
        _assert_metric_sums(_host(got), want)
        if n >= 3:
            assert (want[:, n - 1, 1] == 0).all()                                     # the last node: no valid label
            if route in ("groupstd", "all"):
                assert (want[:, 0] == 0).all() and (_host(got)[:, 0] == 0).all()      # node 0: nothing kept
                assert want[..., 0].sum() > 0
            else:
                assert (want[:, n - 1, 0] == b * od).all()


def test_metric_sums_per_node_from_the_series(lib_built):
    """label_start rows, one of them past the end: clamped and counted"""
    from multistgraph_amd import ops
    geometry = b, out, n, od = (3, 6, 21, 1)
    c = _grid(geometry, True, seed=9)
    series = M.grid_case(77, 1, 40, n, od, y_feat=od + 2, y_start=1)["y"][0]
    starts = np.array([0, 17, 40 - out + 2], dtype=np.int32)
    c = dict(c, y=series)
    kw = _metric_kw(c, "all")
    _violations()
    got = ops.metric_sums_nodes(_dev(c["pred"]), _dev(series), 1, label_start=_dev(starts), **kw)
    assert _violations() > 0 and _violations() == 0
    _assert_metric_sums(_host(got), _metric_ref(c, kw, label_start=starts))


# ---- tables ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(3, 6, 21, 1), (2, 64, 3, 1), (2, 2, 403, 1)], ids=lambda g: "x".join(map(str, g)))
def test_metric_table_rows_against_metric_table(geometry, lib_built):
    from multistgraph_amd import ops
    b, out, n, od = geometry
    c = _grid(geometry, True, seed=3)
    kw = _metric_kw(c, "all")
    pred, y = _dev(c["pred"]), _dev(c["y"])
    horizon = ops.metric_sums(pred, y, c["y_start"], **kw)
    nodes = ops.metric_sums_nodes(pred, y, c["y_start"], **kw)
    empty = torch.zeros(1, 14, dtype=torch.float64, device="cuda:0")
    for swap in (False, True):
        # fold = 1 on (out, 1, 14) sums: the bits of the "single" table, a row of zero sums included
        for sums in (horizon, empty):
            rows = ops.metric_table_rows(sums.reshape(-1, 1, 14), 1, swap)
            assert _equal_nan(rows, ops.metric_table(sums, swap_r2=swap)[0])
        # folded over the horizons / over the nodes: the table of the sums folded on the host, added in ascending index
        per_node = torch.zeros(n, 14, dtype=torch.float64, device="cuda:0")
        for o in range(out):
            per_node = per_node + nodes[o]
        per_horizon = torch.zeros(out, 14, dtype=torch.float64, device="cuda:0")
        for k in range(n):
            per_horizon = per_horizon + nodes[:, k]
        assert _equal_nan(ops.metric_table_rows(nodes, out, swap), ops.metric_table_rows(per_node, 1, swap))
        assert _equal_nan(ops.metric_table_rows(nodes.transpose(0, 1).contiguous(), n, swap),
                          ops.metric_table_rows(per_horizon, 1, swap))
        table = ops.metric_table_rows(nodes, 1, swap)
        assert tuple(table.shape) == (out * n, 10)
        want = M.metric_table_ref(_host(nodes).reshape(-1, 14), swap)[0]
        err = np.abs(_host(table)[:, :8] - want[:, :8])
        assert (_same(_host(table)[:, :8], want[:, :8]) | (err <= 1e-12 * np.abs(want[:, :8]))).all()
    with pytest.raises(Exception):
        ops.metric_table_rows(nodes, 5)      # 5 divides none of the row counts
    with pytest.raises(Exception):
        ops.metric_table_rows(nodes, 0)


# ---- scores ---------------------------------------------------------------------------------------------------------------
def _samples(s, geometry, seed=0):
    return np.random.default_rng(1000 * s + 7 * sum(geometry) + seed).standard_normal((s,) + geometry).astype(np.float32)


def _raw_labels(geometry, seed, nans=False):
    """raw labels (B, out + 1, N, od + 1), scored channels y[:, :out, :, 1:]: about 10 % are 0, a few tiny, a few NaN"""
    b, out, n, od = geometry
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, out + 1, n, od + 1)).astype(np.float32)
    core = y[:, :out, :, 1:]
    pick = rng.random(core.shape)
    core[pick < 0.10] = 0.0
    core[(pick >= 0.10) & (pick < 0.15)] = 3e-5
    if nans:
        core[(pick >= 0.15) & (pick < 0.25)] = np.nan
    return y


def _score_cases(geometry, y):
    """name -> keyword arguments of ops.mc_scores_nodes / node_metrics_ref.score_sums_nodes"""
    n = geometry[2]
    rng = np.random.default_rng(n)
    pm, ps = rng.uniform(-2, 2, n).astype(np.float32), rng.uniform(0.5, 4, n).astype(np.float32)
    gm, gs = rng.uniform(0, 3, n).astype(np.float32), rng.uniform(0.5, 2, n).astype(np.float32)
    core = y[:, :geometry[1], :, 1:]
    group = dict(mean=-1.25, std=3.5, group_mean=gm, group_std=gs)
    hit = R.descale_nodes(core, **group)
    hit = hit[~np.isnan(hit)]
    truth = float(np.sort(hit)[hit.size // 3]) if hit.size else 0.0      # a value a label hits exactly: it is left out
    return {
        "scalar": dict(mean=-1.25, std=3.5),
        "pernode": dict(mean=pm, std=ps),
        # clamp at 0 under this scale: about two samples in three collapse onto 0
        "clamp": dict(mean=-1.25, std=3.5, clamp_min=0.0, null_val=NAN, min_s=0.05),
        "groupstd": dict(clamp_min=0.0, truth_min=truth, null_val=NAN, min_s=-1.0, **group),
        "all": dict(mean=pm, std=ps, group_mean=gm, group_std=gs, clamp_min=0.0, truth_min=0.25, null_val=0.0, min_s=0.05),
    }


def _check_scores(got, want, mag, what):
    got = _host(got)
    assert got.shape == want.shape and got.dtype == np.float64, what
    assert np.array_equal(got[..., 0], want[..., 0]), "%s: count" % (what,)
    assert np.array_equal(got[..., 2], want[..., 2]), "%s: covered" % (what,)
    err = np.abs(got - want)
    assert (err <= SUM_TOL * mag).all(), "%s: worst error %.3e of %.3e" % (what, err.max(), mag.max())


SCORE_RUNS = [(33, g) for g in GEOMETRIES] + [(1, (2, 3, 65, 2)), (257, (2, 3, 65, 2)), (257, (2, 2, 22, 3)),
                                              (1024, (1, 1, 1, 1)), (1024, (3, 6, 21, 1))]


@pytest.mark.parametrize("s,geometry", SCORE_RUNS, ids=["S%d-%s" % (s, "x".join(map(str, g))) for s, g in SCORE_RUNS])
def test_scores_per_node_against_the_reference(s, geometry, lib_built):
    from multistgraph_amd import ops
    b, out, n, od = geometry
    x = _samples(s, geometry)
    with_nan, finite = _raw_labels(geometry, 11 + s, nans=True), _raw_labels(geometry, 11 + s)
    xd = _dev(x)
    for name, kw in _score_cases(geometry, with_nan).items():
        # NaN labels where the NaN null value masks them (under null value 0 a NaN label counts, and its terms are NaN)
        y = with_nan if np.isnan(kw.get("null_val", 0.0)) else finite
        want, mag = R.score_sums_nodes(x, y[:, :out, :, 1:], PROBS, **kw)
        assert not np.isnan(want).any()
        got = ops.mc_scores_nodes(xd, _dev(y), PROBS, y_start=1, **kw)
        assert tuple(got.shape) == (out, n, 5 + len(PROBS))
        _check_scores(got, want, mag, (name, s, geometry))
        if name == "clamp" and s >= 33 and b * out * n * od > 1:
            q = R.quantiles_nodes(x, PROBS, **{k: v for k, v in kw.items() if k in ("mean", "std", "clamp_min")})
            assert (q[0] == 0).mean() > 0.9 and (q[1] == 0).any()      # whole lower halves sit on the clamp
        if name == "groupstd" and want[..., 0].sum() > 10:
            assert want[..., 0].sum() < np.isfinite(y[:, :out, :, 1:]).sum()


@pytest.mark.parametrize("s", [3, 257])
def test_scores_per_node_from_the_series(s, lib_built):
    """label_start rows equal window labels bit for bit; a start past the end is clamped and counted"""
    from multistgraph_amd import ops
    geometry = b, out, n, od = (3, 6, 21, 1)
    rng = np.random.default_rng(s)
    series = rng.standard_normal((40, n, 3)).astype(np.float32)
    series[rng.random(series.shape) < 0.1] = 0.0
    kw = _score_cases(geometry, np.zeros((b, out + 1, n, 2), dtype=np.float32))["all"]
    x = _samples(s, geometry)
    xd, sd = _dev(x), _dev(series)
    starts = np.array([0, 17, 40 - out], dtype=np.int32)
    windows = np.stack([series[t:t + out] for t in starts], 0)
    _violations()
    a = ops.mc_scores_nodes(xd, sd, PROBS, y_start=2, label_start=_dev(starts), **kw)
    assert _violations() == 0
    assert torch.equal(a, ops.mc_scores_nodes(xd, _dev(windows), PROBS, y_start=2, **kw)) and float(a[..., 0].sum()) > 0
    starts[2] += 2
    got = ops.mc_scores_nodes(xd, sd, PROBS, y_start=2, label_start=_dev(starts), **kw)
    assert _violations() > 0 and _violations() == 0
    want, mag = R.score_sums_nodes(x, M.label_rows(series, out, 2, od, starts), PROBS, **kw)
    _check_scores(got, want, mag, ("series", s))


# ---- streaming and repetition -----------------------------------------------------------------------------------------
def test_streaming_gives_the_bits_of_one_call(lib_built):
    """B = 69 at once against accumulating calls over 1, 65 and 3 of the same samples, random finite inputs"""
    from multistgraph_amd import ops
    geometry = b, out, n, od = (69, 2, 5, 2)
    rng = np.random.default_rng(69)
    pred = _dev(rng.standard_normal(geometry).astype(np.float32))
    y = _dev(rng.standard_normal((b, out + 1, n, od + 1)).astype(np.float32))
    x = _dev(_samples(33, geometry))
    gm, gs = _dev(rng.uniform(0, 3, n).astype(np.float32)), _dev(rng.uniform(0.5, 2, n).astype(np.float32))
    mkw = dict(mean=14.41, std=29.3, group_mean=gm, group_std=gs, clamp_min=0.0, truth_min=6.0, min_s=-1.0)
    skw = dict(null_val=NAN, **mkw)
    whole_m = ops.metric_sums_nodes(pred, y, 1, **mkw)
    whole_s = ops.mc_scores_nodes(x, y, PROBS, y_start=1, **skw)
    assert float(whole_m[..., 0].sum()) > 0 and float(whole_s[..., 0].sum()) > 0
    assert not torch.isnan(whole_m).any() and not torch.isnan(whole_s).any()
    run_m = run_s = None
    for lo, hi in ((0, 1), (1, 66), (66, 69)):
        run_m = ops.metric_sums_nodes(pred[lo:hi], y[lo:hi], 1, sums=run_m, **mkw)
        run_s = ops.mc_scores_nodes(x[:, lo:hi].contiguous(), y[lo:hi], PROBS, y_start=1, sums=run_s, **skw)
    assert torch.equal(run_m, whole_m) and torch.equal(run_s, whole_s)
    for _ in range(2):
        assert torch.equal(ops.metric_sums_nodes(pred, y, 1, **mkw), whole_m)
        assert torch.equal(ops.mc_scores_nodes(x, y, PROBS, y_start=1, **skw), whole_s)
    with pytest.raises(Exception):
        ops.metric_sums_nodes(pred, y, 1, sums=torch.zeros(out, n, 13, dtype=torch.float64, device="cuda:0"))
    with pytest.raises(Exception):
        ops.mc_scores_nodes(x, y, PROBS, y_start=1, sums=torch.zeros(out, 8, dtype=torch.float64, device="cuda:0"))


# ---- consistency with the per-horizon entry points ------------------------------------------------------------------------
@pytest.mark.parametrize("geometry", [(3, 6, 21, 1), (2, 2, 22, 3), (2, 2, 403, 1)], ids=lambda g: "x".join(map(str, g)))
def test_rows_added_over_the_nodes_are_the_per_horizon_sums(geometry, lib_built):
    from multistgraph_amd import ops
    b, out, n, od = geometry
    # random inputs: the counts
    rng = np.random.default_rng(n)
    pred = _dev(rng.standard_normal(geometry).astype(np.float32))
    y = _dev(_raw_labels(geometry, 5, nans=True))
    x = _dev(_samples(33, geometry))
    mkw = dict(mean=-1.25, std=3.5, min_s=0.05)
    nodes, horizon = ops.metric_sums_nodes(pred, y, 1, **mkw), ops.metric_sums(pred, y, 1, **mkw)
    for col in (0, 1, 5):
        assert torch.equal(nodes[..., col].sum(1), horizon[:, col])
    nodes = ops.mc_scores_nodes(x, y, PROBS, y_start=1, mean=-1.25, std=3.5)
    horizon = ops.mc_scores(x, y, PROBS, y_start=1, mean=-1.25, std=3.5)
    assert torch.equal(nodes[..., 0].sum(1), horizon[:, 0]) and float(horizon[:, 0].sum()) > 0
    # grid inputs: every partial sum is exact, so every column
    c = _grid(geometry, False, seed=5)
    kw = _metric_kw(c, "scalar")
    nodes = _host(ops.metric_sums_nodes(_dev(c["pred"]), _dev(c["y"]), 1, **kw)).sum(1)
    assert _same(nodes, _host(ops.metric_sums(_dev(c["pred"]), _dev(c["y"]), 1, **kw))).all()
    # S = 32 and levels 1/4, 1/2, 3/4 on grid samples: quantiles, CRPS (divisions by 32 and 1024), Winkler (2 / alpha = 4)
    # and pinball terms are all exact
    xg = (rng.integers(-64, 65, (32,) + geometry) / 16.0).astype(np.float32)
    yg = np.nan_to_num(c["y"], nan=0.0)
    nodes = ops.mc_scores_nodes(_dev(xg), _dev(yg), (0.25, 0.5, 0.75), y_start=1, mean=float(c["mean"]), std=float(c["std"]))
    horizon = ops.mc_scores(_dev(xg), _dev(yg), (0.25, 0.5, 0.75), y_start=1, mean=float(c["mean"]), std=float(c["std"]))
    assert torch.equal(nodes.sum(1), horizon) and float(horizon[:, 4].abs().sum()) > 0


# ---- quantiles on the re-transformed scale ------------------------------------------------------------------------------
@pytest.mark.parametrize("s,geometry", [(1, (2, 2, 22, 3)), (33, (2, 3, 65, 2)), (33, (2, 2, 22, 3)), (257, (2, 2, 403, 1)),
                                        (1024, (1, 1, 1, 1)), (1024, (3, 6, 21, 1))])
def test_quantiles_scaled(s, geometry, lib_built):
    from multistgraph_amd import ops
    levels = (0.0, 0.05, 0.5, 0.95, 1.0)
    n = geometry[2]
    x = _samples(s, geometry)
    xd = _dev(x)
    plain = ops.mc_quantiles(xd, levels, mean=-1.25, std=3.5)
    assert torch.equal(ops.mc_quantiles_scaled(xd, levels, mean=-1.25, std=3.5), plain)
    rng = np.random.default_rng(n)
    kw = dict(mean=rng.uniform(-2, 2, n).astype(np.float32), std=rng.uniform(0.5, 4, n).astype(np.float32),
              group_mean=rng.uniform(-1, 1, n).astype(np.float32), group_std=rng.uniform(0.5, 2, n).astype(np.float32),
              clamp_min=0.0)
    got = ops.mc_quantiles_scaled(xd, levels, **kw)
    assert tuple(got.shape) == (len(levels),) + geometry and got.dtype == torch.float32
    want = R.quantiles_nodes(x, levels, **kw)
    assert np.array_equal(_host(got) + 0.0, want + 0.0) and (want >= 0).all()
    assert s < 33 or n < 21 or (want[0] == 0).any()      # the clamp is at work
    assert torch.equal(_bits(ops.mc_quantiles_scaled(xd, levels, **kw)), _bits(got))
    # any leading axes: (S, E / (N od), N, od)
    flat = ops.mc_quantiles_scaled(xd.reshape(s, -1, n, geometry[3]), levels, **kw)
    assert torch.equal(_bits(flat.reshape(got.shape)), _bits(got))


# ---- dirty buffers --------------------------------------------------------------------------------------------------------
def _guarded(n, dev):
    return torch.full((n + GUARD,), NAN, dtype=torch.float64, device=dev)


@pytest.mark.parametrize("s,geometry", [(33, (2, 3, 65, 2)), (1024, (3, 6, 21, 1)), (257, (2, 2, 22, 3))])
def test_prefilled_buffers_and_guards(s, geometry, lib_built):
    """scratch and sums full of NaN before a non-accumulating call: the same bits, nothing written behind either"""
    from multistgraph_amd import _lib, ops
    lib, dev = _lib.load(), torch.device("cuda:0")
    b, out, n, od = geometry
    x, y = _dev(_samples(s, geometry)), _dev(_raw_labels(geometry, 21))
    pred = x[0].contiguous()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gm = torch.linspace(0.0, 2.0, n, device=dev)
    gs = torch.linspace(0.5, 1.5, n, device=dev)
    mean, std = torch.tensor([-1.25], device=dev), torch.tensor([3.5], device=dev)
    sc = _lib.MetricScale()
    sc.mean, sc.std, sc.per_node, sc.mean2, sc.std2 = mean.data_ptr(), std.data_ptr(), 0, gm.data_ptr(), gs.data_ptr()
    sc.clamp_min, sc.truth_min, sc.min_s = 0.0, 0.5, -1.0
    kw = dict(mean=-1.25, std=3.5, group_mean=gm, group_std=gs, clamp_min=0.0, truth_min=0.5, min_s=-1.0)

    need = C.c_size_t(1)
    _lib.check(lib.matgcn_metric_sums_nodes_bytes(b, out, n, od, C.byref(need)), "matgcn_metric_sums_nodes_bytes")
    scratch = _guarded(need.value // 8, dev)
    sums = _guarded(out * n * 14, dev)
    _lib.check(lib.matgcn_metric_sums_nodes(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), None, b, out, n, od, out + 1,
                                            od + 1, 1, C.byref(sc), C.c_void_p(scratch.data_ptr()), need.value,
                                            C.c_void_p(sums.data_ptr()), 0, stream), "matgcn_metric_sums_nodes")
    want = ops.metric_sums_nodes(pred, y, 1, **kw)
    assert torch.equal(sums[:out * n * 14].reshape(out, n, 14), want) and not torch.isnan(want).any()
    assert torch.isnan(sums[out * n * 14:]).all() and torch.isnan(scratch[need.value // 8:]).all()

    cols = 5 + len(PROBS)
    _lib.check(lib.matgcn_mc_scores_nodes_bytes(b, out, n, od, s, len(PROBS), C.byref(need)), "matgcn_mc_scores_nodes_bytes")
    scratch = _guarded(need.value // 8, dev)
    sums = _guarded(out * n * cols, dev)
    probs = (C.c_float * len(PROBS))(*PROBS)
    _lib.check(lib.matgcn_mc_scores_nodes(C.c_void_p(x.data_ptr()), s, C.c_void_p(y.data_ptr()), None, b, out, n, od, out + 1,
                                          od + 1, 1, C.byref(sc), NAN, probs, len(PROBS), C.c_void_p(scratch.data_ptr()),
                                          need.value, C.c_void_p(sums.data_ptr()), 0, stream), "matgcn_mc_scores_nodes")
    want = ops.mc_scores_nodes(x, y, PROBS, y_start=1, null_val=NAN, **kw)
    assert torch.equal(sums[:out * n * cols].reshape(out, n, cols), want) and not torch.isnan(want).any()
    assert torch.isnan(sums[out * n * cols:]).all() and torch.isnan(scratch[need.value // 8:]).all()
    assert not torch.isnan(scratch[:need.value // 8]).any()      # every element's terms are written, masked ones as zeros


# ---- the model surface, N = 21 ----------------------------------------------------------------------------------------------
OUT = 6


def _model(nodes, batch, scaler=None):
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd.model import MultiATGCN
    dev = torch.device("cuda:0")
    seed = 3
    df = syn.make_data_feature(nodes, seed, "DC", ext_dim=1, scaler=scaler)
    cfg = dict(input_window=24, output_window=OUT, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
               adjtype="multi", adpadj="unidirection", cheb_order=2, embed_dim_node=20, embed_dim_adj=20, rnn_units=64,
               num_layers=2, device=dev, batch_size=batch, start_dim=0, end_dim=1)
    shapes = syn.param_shapes(nodes, out_steps=OUT, feat_in=2, k_total=syn.k_total_for("multi", "unidirection", 2))
    model = MultiATGCN(cfg, df).to(dev).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.closed_form_state(shapes, seed).items()})
    return model


def test_node_evaluator_end_to_end(lib_built):
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd import windows as W
    from multistgraph_amd.evaluator import ALLOWED_METRICS, NodeEvaluator
    nodes, batch, s = 21, 3, 8
    mean, std = 2.0, 1.5
    model = _model(nodes, batch, scaler=syn.PlainScaler(mean, std))
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, nodes, 2)).astype(np.float32)
    pick = W.valid_label_starts(steps, rel, 24)[:batch].astype(np.int32)
    sb = {"series": _dev(series), "label_start": _dev(pick)}
    xw, yw = W.gather_windows(series, pick, rel, OUT)
    wb = {"X": _dev(xw), "y": _dev(yw)}
    gm, gs = rng.uniform(0, 3, nodes).astype(np.float32), rng.uniform(0.5, 2, nodes).astype(np.float32)
    evs = []
    for batch_d in (wb, sb):
        ev = NodeEvaluator({}, probs=PROBS, group_mean=gm, group_std=gs, s_small=1.0)
        for seed in (1, 2):      # two batches into one evaluator
            kept = model.score_mc_nodes(batch_d, ev, samples=s, seed=seed)
            pred = model.collect_node_metrics(ev, batch_d)
        assert tuple(kept.shape) == (s, batch, OUT, nodes, 1) and tuple(pred.shape) == (batch, OUT, nodes, 1)
        evs.append(ev)
    a, b = evs
    assert torch.equal(a._metric_sums, b._metric_sums) and torch.equal(a._score_sums, b._score_sums)
    for name in ("node_table", "node_horizon_table", "horizon_table", "node_scores", "node_horizon_scores", "horizon_scores"):
        ta, tb = getattr(a, name)(), getattr(b, name)()
        assert _equal_nan(ta, tb), name
    assert tuple(a.node_table().shape) == (nodes, 10) and tuple(a.node_horizon_table().shape) == (OUT, nodes, 10)
    assert tuple(a.horizon_table().shape) == (OUT, 10)
    cols = 4 + len(PROBS)
    assert tuple(a.node_scores().shape) == (nodes, cols) and tuple(a.node_horizon_scores().shape) == (OUT, nodes, cols)
    assert tuple(a.horizon_scores().shape) == (OUT, cols)
    # the sums against the reference, from the prediction and the samples the model returned (each batch twice)
    p, y = _host(pred), yw
    want = R.metric_sums_nodes_ref(p, y, 0, mean, std, gm, gs, 0.0, 1.0, -1.0)
    want = R.metric_sums_nodes_ref(p, y, 0, mean, std, gm, gs, 0.0, 1.0, -1.0, start=want)
    got = _host(a._metric_sums)
    assert np.array_equal(got[..., [0, 1, 5]], want[..., [0, 1, 5]])
    assert np.allclose(got, want, rtol=1e-5, atol=1e-6)      # continuous data: float32 quotients in sums 4 and 8
    score_want, mag = R.score_sums_nodes(_host(kept), y[:, :OUT, :, :1], PROBS, mean=mean, std=std, group_mean=gm,
                                         group_std=gs, clamp_min=0.0, truth_min=1.0, null_val=NAN, min_s=-1.0)
    assert np.array_equal(_host(a._score_sums)[..., 0], 2 * score_want[..., 0])
    one = NodeEvaluator({}, probs=PROBS, group_mean=gm, group_std=gs, s_small=1.0)
    assert torch.equal(model.score_mc_nodes(sb, one, samples=s, seed=2), kept)
    _check_scores(one._score_sums, score_want, mag, "score_mc_nodes")
    # the ranking of result_plot.py:128 from the reference table: ascending mean MAPE, tracts without a kept element absent
    folded = want.sum(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        mape = np.where(folded[:, 0] > 0, folded[:, 4] / folded[:, 1], np.nan)
    order = np.argsort(np.where(np.isnan(mape), np.inf, mape), kind="stable")
    order = np.concatenate([order[~np.isnan(mape[order])], order[np.isnan(mape[order])]])
    rank = a.rank("MAPE")
    assert rank.tolist() == order.tolist() and sorted(rank.tolist()) == list(range(nodes))
    table = a.node_table()[:, ALLOWED_METRICS.index("MAPE")].numpy()
    assert np.allclose(table[~np.isnan(mape)], mape[~np.isnan(mape)], rtol=1e-5)
    # NaN scores where nothing was counted
    empty = NodeEvaluator({}, probs=PROBS, s_small=1e9)
    model.score_mc_nodes(wb, empty, samples=s, seed=1)
    assert np.isnan(empty.node_scores().numpy()).all() and np.isnan(empty.horizon_scores().numpy()).all()
    # predict_interval: the defaults spelled out change nothing; the re-transformed band is the reference's
    plain = model.predict_interval(wb, samples=s, probs=PROBS, seed=4)
    again = model.predict_interval(wb, samples=s, probs=PROBS, seed=4, group_mean=None, group_std=None, clamp_min=None)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(plain, again))
    m2, s2, band = model.predict_interval(sb, samples=s, probs=PROBS, seed=4, group_mean=gm, group_std=gs, clamp_min=0.0)
    assert torch.equal(m2, plain[0]) and torch.equal(s2, plain[1])
    kept4 = model.predict_mc(wb, samples=s, seed=4, keep_samples=True)[2]
    want_band = R.quantiles_nodes(_host(kept4), PROBS, mean=mean, std=std, group_mean=gm, group_std=gs, clamp_min=0.0)
    assert np.array_equal(_host(band) + 0.0, want_band + 0.0) and float(band.min()) >= 0
