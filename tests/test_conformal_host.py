"""Conformal calibration on the host (matgcn_mc_conformity, matgcn_conformal_quantile, matgcn_conformal_coverage;
include/matgcn.h): symbols, header and binding, every refusal - all are made before a launch, so dummy pointers do -, the
calibrator's state, and the numpy reference (conformal_ref.py) held to what split conformal calibration promises, so that
the GPU tests need nothing but equality with it.

The statistical bound.  Calibration and test rows are exchangeable draws, so the coverage of one group's margin is
Beta(k, n + 1 - k) distributed: mean k / (n + 1) = 0.9 and sd 0.0095 at n = 999, k = 900.  Pooled over 63 element groups
(or 3 horizons of 21 columns each) and 126 000 test labels the sd is about 0.0015, so 0.90 +- 0.01 is more than six sd
(seeds 0 .. 5 gave pooled coverages between 0.8974 and 0.9032); the seed is fixed and the reference is inside: the bound
is a condition on the inputs, not on any kernel."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import conformal_ref as CR
import mc_scores_ref as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_mc_conformity", "matgcn_conformal_quantile", "matgcn_conformal_coverage")
OK, ERR_NULL, ERR_BAD_ARG = 0, -1, -2
PTR = C.c_void_p(4096)     # a non-NULL pointer nothing dereferences: every call below fails before its launch
NAN = float("nan")


def _lib():
    from multistgraph_amd import _lib
    return _lib


def _scale():
    sc = _lib().MetricScale()
    sc.mean, sc.std, sc.mean2, sc.std2, sc.per_node = None, None, None, None, 0
    sc.clamp_min, sc.truth_min, sc.min_s = NAN, NAN, -1.0
    return sc


def _conformity(lib, samples=PTR, s=32, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0, null_scale=False,
                probs=(0.05, 0.5, 0.95), null_probs=False, n_probs=None, scores=PTR):
    sc = _scale()
    arr = (C.c_float * max(1, len(probs)))(*probs)
    return lib.matgcn_mc_conformity(samples, s, y, None, b, out, n, od, y_steps, y_feat, y_start,
                                    None if null_scale else C.byref(sc), 0.0, None if null_probs else arr,
                                    len(probs) if n_probs is None else n_probs, scores, None)


def _quantile(lib, scores=PTR, rows=10, out=3, cols=65, grouping=1, coverage=0.9, margin=PTR, count=PTR):
    return lib.matgcn_conformal_quantile(scores, rows, out, cols, grouping, coverage, margin, count, None)


def _coverage(lib, scores=PTR, rows=10, out=3, cols=65, grouping=1, margin=PTR, counts=PTR, accumulate=0):
    return lib.matgcn_conformal_coverage(scores, rows, out, cols, grouping, margin, counts, accumulate, None)


def test_library_exports_and_binding(lib_built):
    from multistgraph_amd import evaluator, ops
    from multistgraph_amd.model import MultiATGCN
    _l = _lib()
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    lib = _l.load()
    for name in NEW_FUNCTIONS:
        assert name in _l.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12 == _l.ABI_VERSION
    for fn in (ops.mc_conformity, ops.conformal_quantile, ops.conformal_coverage, MultiATGCN.calibrate_mc,
               evaluator.ConformalCalibrator):
        assert callable(fn)


def test_conformity_arguments_are_checked_on_the_host(lib_built):
    _l = _lib()
    lib = _l.load()
    for name in ("samples", "y", "scores"):
        assert _conformity(lib, **{name: None}) == ERR_NULL, name
    assert _conformity(lib, null_scale=True) == ERR_NULL and _conformity(lib, null_probs=True) == ERR_NULL
    assert _conformity(lib, probs=(0.5,)) == ERR_BAD_ARG                      # a band needs two levels
    for n in (1, 0, -1, 9):
        assert _conformity(lib, probs=(0.1,) * 9, n_probs=n) == ERR_BAD_ARG, n
    for levels in ((-0.01, 0.5), (0.5, 1.01), (NAN, 0.9), (0.5, 0.25), (0.1, NAN, 0.9)):
        assert _conformity(lib, probs=levels) == ERR_BAD_ARG, levels
    for s in (0, -3, _l.MAX_MC_SAMPLES + 1):
        assert _conformity(lib, s=s) == ERR_BAD_ARG, s
    for geometry in (dict(b=0), dict(out=0), dict(out=65), dict(n=0), dict(od=0), dict(y_steps=2), dict(y_steps=0),
                     dict(y_feat=0), dict(y_start=-1), dict(y_start=1), dict(od=3)):
        assert _conformity(lib, **geometry) == ERR_BAD_ARG, geometry


def test_quantile_and_coverage_arguments_are_checked_on_the_host(lib_built):
    lib = _lib().load()
    for name in ("scores", "margin", "count"):
        assert _quantile(lib, **{name: None}) == ERR_NULL, name
    for name in ("scores", "margin", "counts"):
        assert _coverage(lib, **{name: None}) == ERR_NULL, name
    for call in (_quantile, _coverage):
        for grouping in (-1, 2, 7):
            assert call(lib, grouping=grouping) == ERR_BAD_ARG, grouping
        for bad in (dict(rows=0), dict(rows=-4), dict(out=0), dict(out=65), dict(out=-1), dict(cols=0), dict(cols=-3),
                    dict(rows=2 ** 62, out=64, cols=2 ** 30)):                # rows*out*cols leaves int64
            assert call(lib, **bad) == ERR_BAD_ARG, bad
    for coverage in (0.0, -0.5, NAN, 1.0000001, float("inf"), -float("inf")):
        for grouping in (0, 1):
            assert _quantile(lib, coverage=coverage, grouping=grouping) == ERR_BAD_ARG, coverage


def test_calibrator_arguments_and_state(lib_built):
    from multistgraph_amd.evaluator import ConformalCalibrator
    for bad in ((0.5,), (), (0.5, 0.1), (0.5, 0.5), (NAN, 0.9)):
        with pytest.raises(ValueError):
            ConformalCalibrator({}, probs=bad)
    with pytest.raises(ValueError):
        ConformalCalibrator({}, grouping="node")
    with pytest.raises(ValueError):
        ConformalCalibrator({}, group_mean=[0.0])
    with pytest.raises(ValueError):
        ConformalCalibrator({}, capacity=0)
    plain = ConformalCalibrator({"min_s": 0.5})
    group = ConformalCalibrator({"min_s": 0.5}, group_mean=[0.0, 1.0], group_std=[1.0, 2.0], s_small=6, grouping="element")
    assert (plain.min_s, plain.null_val) == (0.5, 0.0) and np.isnan(plain.clamp_min) and np.isnan(plain.truth_min)
    assert (group.min_s, group.clamp_min, group.truth_min) == (-1.0, 0.0, 6.0) and np.isnan(group.null_val)
    assert plain.coverage == CR.coverage_of((0.05, 0.5, 0.95)) and plain.probs == (0.05, 0.5, 0.95)
    for call in (plain.fit, plain.coverage_table, plain.evaluate, plain.infinite_margins):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        plain.apply(torch.zeros(3, 1, 2, 2, 1))

    # a fitted state round-trips, and the calibrator it is loaded into applies the same margin
    group.margin = torch.tensor([[[0.5], [np.inf]], [[-0.25], [2.0]]], dtype=torch.float32)
    group.count = torch.tensor([[[9], [0]], [[9], [7]]], dtype=torch.int32)
    group.affine = (14.5, 29.25)
    state = group.state_dict()
    other = ConformalCalibrator({})
    other.load_state_dict(state)
    again = other.state_dict()
    assert again["probs"] == state["probs"] == (0.05, 0.5, 0.95) and again["grouping"] == "element"
    for key in ("margin", "count"):
        assert torch.equal(again[key], state[key]) and again[key].dtype == state[key].dtype
    for key, val in state["scale"].items():
        got = again["scale"][key]
        if isinstance(val, torch.Tensor):
            assert torch.equal(got, val), key
        else:
            assert got == val or (got != got and val != val), key
    assert torch.equal(state["scale"]["group_std"], torch.tensor([1.0, 2.0])) and float(state["scale"]["std"]) == 29.25
    assert (other.min_s, other.clamp_min, other.truth_min) == (-1.0, 0.0, 6.0) and np.isnan(other.null_val)
    assert other.infinite_margins().tolist() == [1, 0]
    band = torch.tensor(np.random.default_rng(0).uniform(1, 2, (3, 2, 2, 2, 1)).astype(np.float32)).sort(0).values
    got = other.apply(band)
    want = CR.apply_margin(band.numpy(), state["margin"].numpy(), "element", clamp_min=0.0)
    assert np.array_equal(got.numpy(), want) and torch.equal(got[1], band[1])
    assert bool(torch.isinf(got[2, :, 0, 1]).all()) and bool((got[0, :, 0, 1] == 0).all())       # -inf held at the clamp
    # the call it can serve, and the ones it cannot
    other.check_call((0.05, 0.5, 0.95), (14.5, 29.25), [0.0, 1.0], [1.0, 2.0], 0.0)
    for bad in (((0.1, 0.5, 0.9), (14.5, 29.25), [0.0, 1.0], [1.0, 2.0], 0.0),
                ((0.05, 0.5, 0.95), (14.5, 29.0), [0.0, 1.0], [1.0, 2.0], 0.0),
                ((0.05, 0.5, 0.95), None, [0.0, 1.0], [1.0, 2.0], 0.0),
                ((0.05, 0.5, 0.95), (14.5, 29.25), [0.0, 1.0], [1.0, 2.5], 0.0),
                ((0.05, 0.5, 0.95), (14.5, 29.25), None, None, 0.0),
                ((0.05, 0.5, 0.95), (14.5, 29.25), [0.0, 1.0], [1.0, 2.0], None)):
        with pytest.raises(ValueError):
            other.check_call(*bad)


# ---- the reference against what conformal calibration promises --------------------------------------------------------
def _under_dispersed(rng, rows, geometry=(3, 21, 1), s=32):
    """an ensemble of sd 0.3 and labels of sd 1.0 around the same mean"""
    centre = rng.uniform(-2.0, 2.0, (rows,) + geometry)
    x = (centre[None] + 0.3 * rng.standard_normal((s, rows) + geometry)).astype(np.float32)
    y = (centre + 1.0 * rng.standard_normal((rows,) + geometry)).astype(np.float32)
    return x, y


def test_reference_calibrates_an_under_dispersed_ensemble():
    probs = (0.05, 0.95)
    rng = np.random.default_rng(2)
    cal = CR.conformity(*_under_dispersed(rng, 999), probs, null_val=NAN, min_s=-1.0)
    x, y = _under_dispersed(rng, 2000)
    test = CR.conformity(x, y, probs, null_val=NAN, min_s=-1.0)
    assert cal.dtype == np.float32 and not np.isnan(cal).any() and not np.isnan(test).any()
    # the raw band: its score is <= 0 exactly where the label is inside
    q = MC.quantiles(x, probs)
    inside = (q[0] <= y) & (y <= q[1])
    assert np.array_equal(inside, test <= 0) and inside.mean() < 0.5
    coverage = CR.coverage_of(probs)
    for grouping, groups in (("horizon", 3), ("element", 63)):
        margin, count = CR.quantile(cal, 999, grouping, coverage)
        assert margin.size == groups and (count == 999 * 63 // groups).all() and np.isfinite(margin).all() and (margin > 0).all()
        counts = CR.coverage_counts(test, 2000, grouping, margin)
        assert counts[..., 0].sum() == 126000
        pooled = counts[..., 1].sum() / counts[..., 0].sum()
        print("raw PICP %.4f, calibrated (%s) %.4f" % (inside.mean(), grouping, pooled))
        assert abs(pooled - 0.90) <= 0.01, (grouping, pooled)
        # the widened band holds exactly the labels whose score the margin covers
        band = CR.apply_margin(q[:, :50], margin, grouping)
        m = margin.reshape(-1, 1, 1) if grouping == "horizon" else margin
        held = (band[0] <= y[:50]) & (y[:50] <= band[1])
        assert (held == (test[:50] <= m)).mean() > 0.999          # up to the rounding of Q - m against l


def test_reference_rank_rule():
    assert [CR.rank(n, 0.9) for n in (0, 1, 8, 9, 10, 999)] == [1, 2, 9, 9, 10, 900]
    assert CR.rank(3, 0.5) == 2 and CR.rank(3, 1.0) == 4 and CR.rank(5, 1e-9) == 1
    for coverage in (0.5, 0.8, CR.coverage_of((0.05, 0.95)), 1.0):
        assert CR.ranks(np.arange(3000), coverage).tolist() == [CR.rank(n, coverage) for n in range(3000)]
    # the vectorised selection is np.sort(valid)[k - 1] group by group
    rng = np.random.default_rng(7)
    store = rng.standard_normal((40, 2, 5)).astype(np.float32)
    store[rng.random(store.shape) < 0.3] = NAN
    store[:, 1, 4] = NAN
    for grouping, groups in (("horizon", [store[:33, o].ravel() for o in range(2)]),
                             ("element", [store[:33, o, c] for o in range(2) for c in range(5)])):
        for coverage in (0.5, 0.9, 1.0):
            margin, count = CR.quantile(store, 33, grouping, coverage)
            for g, members in enumerate(groups):
                valid = members[~np.isnan(members)]
                k = CR.rank(valid.size, coverage)
                assert count.ravel()[g] == valid.size
                assert margin.ravel()[g] == (np.sort(valid)[k - 1] if k <= valid.size else np.inf)
    s = np.full((4, 2, 3), NAN, dtype=np.float32)
    s[:3, 0, 0] = [3.0, -1.0, 2.0]
    s[3, 0, 0] = -50.0                                            # behind `rows`: never read
    s[0, 1, 2] = 7.0
    margin, count = CR.quantile(s, 3, "element", 0.5)
    assert count.tolist() == [[3, 0, 0], [0, 0, 1]] and margin[0, 0] == 2.0 and np.isinf(margin[0, 1])
    assert margin[1, 2] == 7.0                                    # n = 1, k = 1
    margin, count = CR.quantile(s, 3, "horizon", 0.9)
    assert count.tolist() == [3, 1] and np.isinf(margin).all()    # k = 4 > 3 and k = 2 > 1
    counts = CR.coverage_counts(s, 4, "horizon", np.array([2.0, np.inf], dtype=np.float32))
    assert counts.tolist() == [[4, 3], [1, 1]]                    # a score on the margin is covered
