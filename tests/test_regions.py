"""Region totals on the GPU - matgcn_group_sums, matgcn_group_label_sums - against the numpy reference (regions_ref.py), and
the surface above them: ops, regions.RegionMap, evaluator.RegionEvaluator, ConformalCalibrator(regions=),
MultiATGCN.predict_interval(regions=) / predict_regions / collect_region_metrics / score_mc_regions.

Every comparison is on the raw bits: the same NaN positions and numpy.array_equal of the int32 (int64) views everywhere
else.  No tolerance: the reference adds a region's members in listed order in float64 and rounds once, and
tests/test_regions_host.py shows on the CPU that another order gives other bits.

Shapes.  rows (S*B*out) in {1, 105 = 3*5*7, 257}; N in {1, 21, 64, 65, 257}; od in {1, 2}; each value at least once, the
smallest and the largest together once.  N = 4096, od = 2: a row of 32 KB, one row per tile.  The tile holds 16 384 floats
with an odd row stride, so a row of 16 383 floats is the last one staged in LDS and a row of 16 384 the first one walked in
global memory: both, and 16 385.
Maps.  A partition into three uneven groups that leaves one node out; singletons (G = N); G = 70 with an empty group, a
whole-graph group, overlapping groups and members in non-ascending order (the whole-graph group holds every node, so the
node in no group is the partition's).  Each with weights absent and with non-dyadic weights."""
import numpy as np
import pytest
import torch

import conformal_ref as CR
import mc_scores_ref as MC
import node_metrics_ref as R
import regions_ref as G

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
PROBS = (0.05, 0.5, 0.95)
LEVELS = (0.25, 0.5, 0.75)      # coverage 0.5: k = ceil(4 * 0.5) = 2 <= n = 3 calibration rows
#            leading shape, N, od
GEOMETRIES = (((1,), 1, 1), ((3, 5, 7), 21, 1), ((257,), 64, 2), ((3, 5, 7), 65, 2), ((257,), 257, 1), ((1,), 257, 2),
              ((257,), 257, 2), ((6,), 4096, 2), ((2,), 16383, 1), ((2,), 16384, 1), ((3,), 16385, 1))
SCALES = ("identity", "scalar", "pernode", "group_clamp")


def _id(g):
    return "%sx%dx%d" % ("x".join(map(str, g[0])), g[1], g[2])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _same_bits(got, want):
    """the same shape and dtype, NaN in the same places, the same bits everywhere else"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return False
    view = np.int32 if got.dtype == np.float32 else np.int64
    return np.array_equal(got.view(view)[~nan], want.view(view)[~nan])


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ---- maps -----------------------------------------------------------------------------------------------------------------
def _map_groups(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "partition":
        a, b = n // 7, n // 7 + (2 * n) // 7
        left_out = n // 2 if n >= 4 else -1
        return [[k for k in range(lo, hi) if k != left_out] for lo, hi in ((0, a), (a, b), (b, n))]
    if kind == "singletons":
        return [[k] for k in range(n)]
    assert kind == "mixed"
    groups = [[], list(range(n))]
    for g in range(68):
        size = int(rng.integers(1, max(2, min(n, 40))))
        members = rng.permutation(n)[:size].tolist()
        if g % 2 and len(members) > 1:
            members = sorted(members, reverse=True)          # descending: never the ascending order
        if g == 5:
            members = members + members[:1]                   # a node twice in one group
        groups.append(members)
    return groups


def _region_map(kind, n, weighted):
    from multistgraph_amd.regions import RegionMap
    groups = _map_groups(kind, n)
    weights = None
    if weighted:
        rng = np.random.default_rng(7 + n)
        weights = [(rng.uniform(-1.0, 2.0, len(g)).astype(F32) / F32(3.0)).tolist() for g in groups]
    return RegionMap(n, groups=groups, weights=weights)


def _scale(name, n):
    rng = np.random.default_rng(n)
    pm, ps = rng.uniform(-2, 2, n).astype(F32), rng.uniform(0.5, 4, n).astype(F32)
    gm, gs = rng.uniform(-1, 3, n).astype(F32), rng.uniform(0.5, 2, n).astype(F32)
    return {"identity": {}, "scalar": dict(mean=-1.25, std=3.5), "pernode": dict(mean=pm, std=ps),
            "group_clamp": dict(mean=-1.25, std=3.5, group_mean=gm, group_std=gs, clamp_min=0.0)}[name]


def _values(lead, n, od, seed=0):
    """continuous values (no grid), a NaN and a -0.0 among them"""
    rng = np.random.default_rng(seed + n + 10 * od + sum(lead))
    x = (rng.standard_normal(tuple(lead) + (n, od)) * 4.0).astype(F32)
    flat = x.reshape(-1)
    if flat.size > 8:
        flat[flat.size // 3] = NAN
        flat[flat.size // 5] = -0.0
    return x


# ---- the kernel against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=_id)
def test_group_sums_against_the_reference(geometry, scale, lib_built):
    from multistgraph_amd import ops
    lead, n, od = geometry
    x = _values(lead, n, od)
    xd = _dev(x)
    kw = _scale(scale, n)
    kinds = ("partition", "mixed") if n > 4096 else ("partition", "singletons", "mixed")
    for kind in kinds:
        for weighted in (False, True):
            rm = _region_map(kind, n, weighted)
            want = G.group_sums(x, rm.ptr, rm.node, rm.weight, **kw)
            out = torch.full(tuple(lead) + (rm.num_groups, od), NAN, dtype=torch.float32, device="cuda:0")
            got = ops.group_sums(xd, rm, out=out, **kw)
            assert got is out and _same_bits(_host(got), want), (kind, weighted)
            if kind == "mixed":
                assert _same_bits(_host(got)[..., 0, :], np.zeros(tuple(lead) + (od,), dtype=F32))      # empty: +0.0
            if scale == "group_clamp" and not weighted and x.size > 64:
                assert np.nanmin(want) >= 0
    # any leading axes, and a fresh output tensor
    rm = _region_map("mixed", n, True)
    flat = ops.group_sums(xd.reshape(-1, n, od), rm, **kw)
    assert _same_bits(_host(flat).reshape(tuple(lead) + (70, od)), G.group_sums(x, rm.ptr, rm.node, rm.weight, **kw))


@pytest.mark.parametrize("rows,n,members,weighted", [(5, 64, 4096, False), (5, 64, 4097, False), (5, 64, 2048, True),
                                                     (5, 64, 2049, True), (2, 14000, 2383, False), (2, 14000, 2384, False)])
def test_maps_on_either_side_of_the_staging_limit(rows, n, members, weighted, lib_built):
    """A map is copied into LDS behind the rows while it holds at most 4096 floats (offsets, and weights if any) and still
    fits the 16 384 floats a workgroup has (a row of 14 000 has the odd stride 14 001: 2383 more fit); one member more and
    the chains read it from global memory.  The same bits either way."""
    from multistgraph_amd import ops
    from multistgraph_amd.regions import RegionMap
    rng = np.random.default_rng(members)
    cuts = sorted(rng.integers(0, members + 1, 6).tolist())
    nodes = rng.integers(0, n, members).tolist()
    groups = [nodes[lo:hi] for lo, hi in zip([0] + cuts, cuts + [members])]
    weights = [rng.uniform(0.1, 1.0, len(g)).astype(F32).tolist() for g in groups] if weighted else None
    rm = RegionMap(n, groups=groups, weights=weights)
    assert rm.num_members == members and rm.num_groups == 7
    x = _values((rows,), n, 1, seed=members)
    kw = _scale("group_clamp", n)
    got = ops.group_sums(_dev(x), rm, out=torch.full((rows, 7, 1), NAN, device="cuda:0"), **kw)
    assert _same_bits(_host(got), G.group_sums(x, rm.ptr, rm.node, rm.weight, **kw))


def test_the_listed_order_decides_the_bits(lib_built):
    """members (1, 2^60, -2^60): 0 in listed order, 1 with the 1 added last (tests/test_regions_host.py)"""
    from multistgraph_amd import ops
    from multistgraph_amd.regions import RegionMap
    x = np.zeros((5, 3, 1), dtype=F32)
    x[:, :, 0] = [1.0, 2.0 ** 60, -2.0 ** 60]
    x[3, 0, 0] = 3.0
    xd = _dev(x)
    listed, last = RegionMap(3, groups=[[0, 1, 2]]), RegionMap(3, groups=[[1, 2, 0]])
    a, b = _host(ops.group_sums(xd, listed)), _host(ops.group_sums(xd, last))
    assert _same_bits(a, G.group_sums(x, listed.ptr, listed.node)) and _same_bits(b, G.group_sums(x, last.ptr, last.node))
    assert (a == 0).all() and b[:, 0, 0].tolist() == [1.0, 1.0, 1.0, 3.0, 1.0]
    # float64 inside the chain: 2^24 + 1 + 1 is 2^24 + 2, where float32 adds would stay at 2^24
    y = np.array([[[2.0 ** 24], [1.0], [1.0]]], dtype=F32)
    assert float(ops.group_sums(_dev(y), listed)[0, 0, 0]) == 2.0 ** 24 + 2.0


def test_two_calls_give_the_same_bits(lib_built):
    from multistgraph_amd import ops
    lead, n, od = (257,), 257, 2
    x = _dev(_values(lead, n, od, seed=3))
    rm = _region_map("mixed", n, True)
    kw = _scale("group_clamp", n)
    first = ops.group_sums(x, rm, **kw)
    for _ in range(3):
        assert torch.equal(_bits(ops.group_sums(x, rm, **kw)), _bits(first))
    y = _dev(np.random.default_rng(1).standard_normal((5, 4, n, 3)).astype(F32))
    first = ops.group_label_sums(y, rm, 3, 2, 1, **kw)
    assert torch.equal(_bits(ops.group_label_sums(y, rm, 3, 2, 1, **kw)), _bits(first))
    with pytest.raises(Exception):
        ops.group_sums(x[:, :200].contiguous(), rm)            # the map covers 257 nodes
    with pytest.raises(Exception):
        ops.group_sums(x, rm, out=torch.empty(257, 70, 1, device="cuda:0"))
    with pytest.raises(Exception):
        ops.group_sums(x.cpu(), rm)


# ---- labels ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,od", [(21, 1), (65, 2), (257, 2)])
def test_label_sums_window_and_series_geometry(n, od, lib_built):
    import ctypes as C
    from multistgraph_amd import _lib, ops
    b, out, y_steps, y_feat, y_start = 3, 6, 8, od + 2, 1
    rng = np.random.default_rng(n)
    series = rng.standard_normal((40, n, y_feat)).astype(F32)
    starts = np.array([0, 17, 40 - out], dtype=np.int32)
    windows = np.stack([np.concatenate([series[t:t + out], series[:y_steps - out]], 0) for t in starts], 0)
    assert windows.shape == (b, y_steps, n, y_feat)
    kw = _scale("group_clamp", n)
    cnt = C.c_int64()
    _lib.check(_lib.load().matgcn_series_violations(C.byref(cnt), 1), "matgcn_series_violations")
    for kind in ("partition", "singletons", "mixed"):
        for weighted in (False, True):
            rm = _region_map(kind, n, weighted)
            want = G.group_label_sums(windows, rm.ptr, rm.node, rm.weight, out, od, y_start=y_start, **kw)
            outd = torch.full((b, out, rm.num_groups, od), NAN, dtype=torch.float32, device="cuda:0")
            got = ops.group_label_sums(_dev(windows), rm, out, od, y_start, out=outd, **kw)
            assert got is outd and _same_bits(_host(got), want), (kind, weighted)
            ser = ops.group_label_sums(_dev(series), rm, out, od, y_start, label_start=_dev(starts), **kw)
            assert torch.equal(_bits(ser), _bits(got)), (kind, weighted)
            assert _same_bits(_host(ser), G.group_label_sums(series, rm.ptr, rm.node, rm.weight, out, od, y_start=y_start,
                                                             label_start=starts, **kw))
    _lib.check(_lib.load().matgcn_series_violations(C.byref(cnt), 1), "matgcn_series_violations")
    assert cnt.value == 0


def test_a_nan_label_makes_exactly_its_regions_nan(lib_built):
    from multistgraph_amd import ops
    n, od, b, out = 65, 2, 2, 3
    y = np.random.default_rng(2).standard_normal((b, out, n, od)).astype(F32)
    node = 13
    y[1, 2, node, 0] = NAN
    rm = _region_map("mixed", n, False)
    got = _host(ops.group_label_sums(_dev(y), rm, out, od, mean=2.0, std=1.5))
    holds = np.array([node in rm.members(g) for g in range(rm.num_groups)])
    assert holds.sum() >= 2 and not holds.all()
    want_nan = np.zeros(got.shape, dtype=bool)
    want_nan[1, 2, holds, 0] = True
    assert np.array_equal(np.isnan(got), want_nan)
    assert _same_bits(got, G.group_label_sums(y, rm.ptr, rm.node, rm.weight, out, od, mean=2.0, std=1.5))


# ---- composition on a tiny model ------------------------------------------------------------------------------------------
NODES, BATCH, OUT, S = 65, 3, 3, 8
MEAN, STD = 2.0, 1.5


class _Tiny:
    def __init__(self, od):
        from multistgraph_amd import synthetic as syn
        from multistgraph_amd import windows as W
        from multistgraph_amd.model import MultiATGCN
        dev = torch.device("cuda:0")
        seed = 3
        self.od = od
        df = dict(syn.make_data_feature(NODES, seed, "DC", ext_dim=1, scaler=syn.PlainScaler(MEAN, STD)), output_dim=od,
                  feature_dim=od + 1)
        cfg = dict(input_window=24, output_window=OUT, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
                   adjtype="multi", adpadj="unidirection", cheb_order=2, embed_dim_node=20, embed_dim_adj=20, rnn_units=64,
                   num_layers=2, device=dev, batch_size=BATCH, start_dim=0, end_dim=od)
        shapes = syn.param_shapes(NODES, out_steps=OUT, feat_in=od + 1, out_dim=od,
                                  k_total=syn.k_total_for("multi", "unidirection", 2))
        self.model = MultiATGCN(cfg, df).to(dev).eval()
        self.model.load_state_dict({k: torch.from_numpy(v) for k, v in syn.closed_form_state(shapes, seed).items()})
        rel = W.window_offsets(24)
        steps = 24 * 28 + 24 * 2 + 7
        rng = np.random.default_rng(5)
        series = rng.standard_normal((steps, NODES, od + 1)).astype(F32)
        pick = W.valid_label_starts(steps, rel, 24)[:BATCH].astype(np.int32)
        # missing labels of tract 7, in label rows behind every row a window of this batch reads: X stays finite
        last_read = int(pick.max()) + max(int(max(rel)), -1)
        gaps = [t for t in range(int(pick.min()), int(pick.max()) + OUT) if t > last_read]
        assert gaps
        series[gaps, 7, 0] = NAN
        xw, yw = W.gather_windows(series, pick, rel, OUT)
        assert not np.isnan(xw).any() and np.isnan(yw).any()
        self.yw = yw
        self.wb = {"X": _dev(xw), "y": _dev(yw)}
        self.sb = {"series": _dev(series), "label_start": _dev(pick)}
        self.gm, self.gs = rng.uniform(0, 3, NODES).astype(F32), rng.uniform(0.5, 2, NODES).astype(F32)
        self.scale = dict(mean=MEAN, std=STD, group_mean=self.gm, group_std=self.gs)
        self.rm = _region_map("mixed", NODES, od == 2)
        self.kw = dict(group_mean=self.gm, group_std=self.gs, clamp_min=0.0)
        # shared, computed once, never written: the ensemble of seed 4, its prediction, and their reference totals
        with torch.no_grad():
            self.kept = self.model.predict_mc(self.wb, samples=S, seed=4, keep_samples=True)[2]
            self.pred = self.model.predict(self.wb)
        rm = self.rm
        self.totals = G.group_sums(_host(self.kept), rm.ptr, rm.node, rm.weight, clamp_min=0.0, **self.scale)
        self.pred_totals = G.group_sums(_host(self.pred), rm.ptr, rm.node, rm.weight, clamp_min=0.0, **self.scale)
        self.label_totals = G.group_label_sums(yw, rm.ptr, rm.node, rm.weight, OUT, od, **self.scale)


_TINY = {}


@pytest.fixture(params=[1, 2], ids=["od1", "od2"])
def tiny(request, lib_built):
    if request.param not in _TINY:
        _TINY[request.param] = _Tiny(request.param)
    return _TINY[request.param]


def test_the_series_input_sees_no_nan(tiny):
    """the NaN labels sit in rows no window of the batch reads, so X is finite and the same from both kinds of batch"""
    with torch.no_grad():
        assert torch.equal(tiny.model.predict(tiny.sb), tiny.pred) and not torch.isnan(tiny.pred).any()
    assert np.isnan(tiny.label_totals).any() and not np.isnan(tiny.label_totals).all()


def test_band_of_the_region_totals(tiny):
    from multistgraph_amd.regions import RegionMap
    m = tiny.model
    mean, std, band = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, regions=tiny.rm, **tiny.kw)
    assert tuple(band.shape) == (len(PROBS), BATCH, OUT, 70, tiny.od) and tuple(mean.shape) == (BATCH, OUT, 70, tiny.od)
    assert _same_bits(_host(band), MC.quantiles(tiny.totals, PROBS))
    td = _dev(tiny.totals)
    assert torch.equal(_bits(mean), _bits(td.mean(0))) and torch.equal(_bits(std), _bits(td.std(0, unbiased=False)))
    # the resident-series batch gives the same bits
    again = m.predict_interval(tiny.sb, samples=S, probs=PROBS, seed=4, regions=tiny.rm, **tiny.kw)
    assert all(torch.equal(_bits(u), _bits(v)) for u, v in zip(again, (mean, std, band)))
    # without the group pair and the clamp members get the scaler's inverse only
    plain = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, regions=tiny.rm)[2]
    rm = tiny.rm
    assert _same_bits(_host(plain), MC.quantiles(G.group_sums(_host(tiny.kept), rm.ptr, rm.node, rm.weight, mean=MEAN,
                                                              std=STD), PROBS))
    # singletons: the node-level band of the same call, bit for bit
    single = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, regions=RegionMap.singletons(NODES), **tiny.kw)[2]
    node = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, **tiny.kw)[2]
    assert torch.equal(_bits(single), _bits(node)) and float(node.min()) >= 0
    # the point forecast's totals
    got = m.predict_regions(tiny.wb, tiny.rm, **tiny.kw)
    assert _same_bits(_host(got), tiny.pred_totals)
    assert torch.equal(_bits(m.predict_regions(tiny.sb, tiny.rm, **tiny.kw)), _bits(got))
    with pytest.raises(Exception):
        m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, regions=RegionMap.total(NODES + 1))


def test_region_evaluator_streams_and_matches_the_reference(tiny):
    from multistgraph_amd.evaluator import RegionEvaluator
    m, od = tiny.model, tiny.od
    make = lambda: RegionEvaluator({}, tiny.rm, probs=PROBS, group_mean=tiny.gm, group_std=tiny.gs, s_small=1.0)
    y = tiny.wb["y"]
    whole, pieces, window, series = make(), make(), make(), make()
    whole.collect_scaled(tiny.pred, y, 0, MEAN, STD)
    whole.collect_samples(tiny.kept, y, 0, MEAN, STD)
    for lo, hi in ((0, 1), (1, BATCH)):
        pieces.collect_scaled(tiny.pred[lo:hi].contiguous(), y[lo:hi].contiguous(), 0, MEAN, STD)
        pieces.collect_samples(tiny.kept[:, lo:hi].contiguous(), y[lo:hi].contiguous(), 0, MEAN, STD)
    for ev, batch in ((window, tiny.wb), (series, tiny.sb)):
        assert torch.equal(m.collect_region_metrics(ev, batch), tiny.pred)
        assert torch.equal(m.score_mc_regions(batch, ev, samples=S, seed=4), tiny.kept)
    tables = ("node_horizon_table", "node_table", "horizon_table", "node_horizon_scores", "node_scores", "horizon_scores")
    for other in (pieces, window, series):
        assert torch.equal(_bits(other._metric_sums), _bits(whole._metric_sums))
        assert torch.equal(_bits(other._score_sums), _bits(whole._score_sums))
        for name in tables:
            assert _same_bits(getattr(other, name)().numpy(), getattr(whole, name)().numpy()), name
        assert other.rank("MAE").tolist() == whole.rank("MAE").tolist()
    assert tuple(whole.node_horizon_table().shape) == (OUT, 70, 10) and tuple(whole.node_table().shape) == (70, 10)
    assert tuple(whole.horizon_scores().shape) == (OUT, 4 + len(PROBS)) and sorted(whole.rank().tolist()) == list(range(70))
    # the sums: node_metrics_ref on the reference's totals, identity scale, NaN the only mask, s_small on the true total
    want = R.metric_sums_nodes_ref(tiny.pred_totals, tiny.label_totals, 0, None, None, None, None, NAN, 1.0, -1.0)
    got = _host(whole._metric_sums)
    with np.errstate(invalid="ignore"):
        print("metric sums: worst |got - want| = %.3e" % np.nanmax(np.abs(got - want)))
    assert want[..., 0].sum() > 0 and (want[:, 0, 0] == 0).all()                   # the empty region's total 0 is <= s_small
    assert _same_bits(got, want)
    score_want, mag = R.score_sums_nodes(tiny.totals, tiny.label_totals, PROBS, clamp_min=NAN, truth_min=1.0, null_val=NAN,
                                         min_s=-1.0)
    got = _host(whole._score_sums)
    print("score sums: worst |got - want| / magnitude = %.3e" % np.max(np.abs(got - score_want) / np.maximum(mag, 1e-300)))
    assert _same_bits(got, score_want)
    # a region holding the tract with missing labels has no label there: fewer of its elements are counted
    holds = np.array([7 in tiny.rm.members(g) for g in range(70)])
    valid = _host(whole._metric_sums)[..., 1]
    assert holds.sum() >= 2 and np.isnan(tiny.label_totals[:, :, holds]).any()
    assert not np.isnan(tiny.label_totals[:, :, ~holds]).any()
    assert valid[:, holds].sum() <= (~np.isnan(tiny.label_totals[:, :, holds])).sum()


@pytest.mark.parametrize("grouping", ["horizon", "element"])
def test_conformal_calibration_of_the_region_band(tiny, grouping):
    from multistgraph_amd.evaluator import ConformalCalibrator
    from multistgraph_amd.regions import RegionMap
    m = tiny.model
    cals = []
    for batch in (tiny.wb, tiny.sb):
        cal = ConformalCalibrator({}, probs=LEVELS, grouping=grouping, group_mean=tiny.gm, group_std=tiny.gs, regions=tiny.rm)
        assert torch.equal(m.calibrate_mc(batch, cal, samples=S, seed=4), tiny.kept)
        cal.fit()
        cals.append(cal)
    win, ser = cals
    assert torch.equal(_bits(win._store[:BATCH]), _bits(ser._store[:BATCH]))
    assert torch.equal(_bits(win.margin), _bits(ser.margin)) and torch.equal(win.count, ser.count)
    scores = CR.conformity(tiny.totals, tiny.label_totals, LEVELS, clamp_min=NAN, truth_min=NAN, null_val=NAN, min_s=-1.0)
    assert _same_bits(_host(win._store[:BATCH]), scores) and np.isnan(scores).any()
    margin, count = CR.quantile(scores, BATCH, grouping, CR.coverage_of(LEVELS))
    assert _same_bits(_host(win.margin), margin) and np.array_equal(_host(win.count), count)
    assert tuple(win.margin.shape) == ((OUT,) if grouping == "horizon" else (OUT, 70, tiny.od))
    # evaluate(): the calibration rows counted against their own margin
    m.calibrate_mc(tiny.sb, win, samples=S, seed=4, test=True)
    counts = CR.coverage_counts(scores, BATCH, grouping, margin)
    assert np.array_equal(_host(win._test_counts), counts)
    result = win.evaluate()
    pooled = counts.reshape(OUT, -1, 2).sum(1)
    for o in range(OUT):
        assert result["PICP@%d" % (o + 1)] == float(pooled[o, 1]) / float(pooled[o, 0])
        assert result["INF_MARGINS@%d" % (o + 1)] == int(np.isinf(margin).reshape(OUT, -1).sum(1)[o])
    # the calibrated band is apply() of the region band
    band = m.predict_interval(tiny.wb, samples=S, probs=LEVELS, seed=4, regions=tiny.rm, **tiny.kw)[2]
    got = m.predict_interval(tiny.wb, samples=S, probs=LEVELS, seed=4, regions=tiny.rm, calibrator=win, **tiny.kw)[2]
    assert torch.equal(_bits(got), _bits(win.apply(band)))
    assert _same_bits(_host(got), CR.apply_margin(MC.quantiles(tiny.totals, LEVELS), margin, grouping, clamp_min=0.0))
    # a calibrator fitted on another map, or on none, is refused; so is this one for a node-level band
    other = RegionMap(NODES, groups=[list(reversed(g)) for g in _map_groups("mixed", NODES)],
                      weights=None if tiny.rm.weight is None else [list(reversed(tiny.rm.weights_of(g))) for g in range(70)])
    for regions in (other, RegionMap.singletons(NODES), None):
        with pytest.raises(ValueError):
            m.predict_interval(tiny.wb, samples=S, probs=LEVELS, seed=4, regions=regions, calibrator=win, **tiny.kw)
    node_level = ConformalCalibrator({}, probs=LEVELS, grouping=grouping, group_mean=tiny.gm, group_std=tiny.gs)
    m.calibrate_mc(tiny.wb, node_level, samples=S, seed=4)
    node_level.fit()
    with pytest.raises(ValueError):
        m.predict_interval(tiny.wb, samples=S, probs=LEVELS, seed=4, regions=tiny.rm, calibrator=node_level, **tiny.kw)
    # the state carries the map
    loaded = ConformalCalibrator({})
    loaded.load_state_dict(win.state_dict())
    again = m.predict_interval(tiny.wb, samples=S, probs=LEVELS, seed=4, regions=tiny.rm, calibrator=loaded, **tiny.kw)[2]
    assert torch.equal(_bits(again), _bits(got))


def test_default_paths_are_the_node_level_ops(tiny):
    """regions=None: predict_interval, score_mc_nodes and calibrate_mc give what the node-level ops give directly"""
    from multistgraph_amd import ops
    from multistgraph_amd.evaluator import ConformalCalibrator, NodeEvaluator
    m, y = tiny.model, tiny.wb["y"]
    mean, std, band = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4)
    m0, s0, kept = m.predict_mc(tiny.wb, samples=S, seed=4, keep_samples=True)
    assert torch.equal(_bits(kept), _bits(tiny.kept))
    assert torch.equal(_bits(band), _bits(ops.mc_quantiles(kept, PROBS)))
    assert torch.equal(_bits(mean), _bits(m0)) and torch.equal(_bits(std), _bits(s0))
    scaled = m.predict_interval(tiny.wb, samples=S, probs=PROBS, seed=4, regions=None, **tiny.kw)
    assert torch.equal(_bits(scaled[2]), _bits(ops.mc_quantiles_scaled(kept, PROBS, MEAN, STD, tiny.gm, tiny.gs, 0.0)))
    assert torch.equal(_bits(scaled[0]), _bits(m0)) and torch.equal(_bits(scaled[1]), _bits(s0))
    ev = NodeEvaluator({}, probs=PROBS, group_mean=tiny.gm, group_std=tiny.gs, s_small=1.0)
    m.score_mc_nodes(tiny.wb, ev, samples=S, seed=4)
    want = ops.mc_scores_nodes(kept, y, PROBS, 0, MEAN, STD, tiny.gm, tiny.gs, clamp_min=0.0, truth_min=1.0, null_val=NAN,
                               min_s=-1.0)
    assert torch.equal(_bits(ev._score_sums), _bits(want))
    cal = ConformalCalibrator({}, probs=LEVELS, grouping="element", group_mean=tiny.gm, group_std=tiny.gs)
    m.calibrate_mc(tiny.wb, cal, samples=S, seed=4)
    want = ops.mc_conformity(kept, y, LEVELS, 0, MEAN, STD, tiny.gm, tiny.gs, clamp_min=0.0, truth_min=NAN, min_s=-1.0,
                             null_val=NAN)
    assert torch.equal(_bits(cal._store[:BATCH]), _bits(want)) and cal.regions is None
    assert cal.state_dict()["regions"] is None
