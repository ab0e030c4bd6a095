"""The per-node evaluation entry points on the host (matgcn_metric_sums_nodes, matgcn_metric_table_rows,
matgcn_mc_quantiles_scaled, matgcn_mc_scores_nodes; include/matgcn.h): symbols, header and binding, every refusal - all
are made before a launch, so dummy pointers do -, the scratch sizes, the argument errors of evaluator.NodeEvaluator, and
the numpy reference of the grouping (node_metrics_ref.py) against the per-horizon references it is built from."""
import ctypes as C
import os

import numpy as np
import pytest

import mc_scores_ref as MC
import metrics_ref as M
import node_metrics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_metric_sums_nodes_bytes", "matgcn_metric_sums_nodes", "matgcn_metric_table_rows",
                 "matgcn_mc_quantiles_scaled", "matgcn_mc_scores_nodes_bytes", "matgcn_mc_scores_nodes")
OK, ERR_NULL, ERR_BAD_ARG, ERR_SMALL_BUFFER = 0, -1, -2, -4
PTR = C.c_void_p(4096)     # a non-NULL pointer nothing dereferences: every call below fails before its launch
NAN = float("nan")
BAD_LEVELS = [(-0.01,), (1.01,), (NAN,), (0.5, 0.25), (0.1, NAN, 0.9)]


def _lib():
    from multistgraph_amd import _lib
    return _lib


def _scale(mean=None, std=None, mean2=None, std2=None, per_node=0):
    sc = _lib().MetricScale()
    sc.mean, sc.std, sc.mean2, sc.std2, sc.per_node = mean, std, mean2, std2, per_node
    sc.clamp_min, sc.truth_min, sc.min_s = NAN, NAN, -1.0
    return sc


def _probs(*vals):
    return (C.c_float * max(1, len(vals)))(*vals), len(vals)


def _sums(lib, pred=PTR, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0, scale=None, null_scale=False,
          scratch=None, scratch_bytes=0, sums=PTR):
    sc = _scale() if scale is None else scale
    return lib.matgcn_metric_sums_nodes(pred, y, None, b, out, n, od, y_steps, y_feat, y_start,
                                        None if null_scale else C.byref(sc), scratch, scratch_bytes, sums, 0, None)


def _scores(lib, samples=PTR, s=32, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0, scale=None,
            null_scale=False, probs=(0.05, 0.5, 0.95), null_probs=False, n_probs=None, scratch=PTR,
            scratch_bytes=1 << 40, sums=PTR):
    sc = _scale() if scale is None else scale
    arr, k = _probs(*probs)
    return lib.matgcn_mc_scores_nodes(samples, s, y, None, b, out, n, od, y_steps, y_feat, y_start,
                                      None if null_scale else C.byref(sc), 0.0, None if null_probs else arr,
                                      k if n_probs is None else n_probs, scratch, scratch_bytes, sums, 0, None)


def _quantiles(lib, samples=PTR, s=32, elems=2 * 3 * 65 * 2, n=65, od=2, scale=None, null_scale=False,
               probs=(0.05, 0.5, 0.95), null_probs=False, n_probs=None, out=PTR):
    sc = _scale() if scale is None else scale
    arr, k = _probs(*probs)
    return lib.matgcn_mc_quantiles_scaled(samples, s, elems, n, od, None if null_probs else arr,
                                          k if n_probs is None else n_probs, None if null_scale else C.byref(sc), out, None)


def _score_bytes(lib, b=2, out=3, n=65, od=2, s=32, nq=3):
    need = C.c_size_t(0)
    return lib.matgcn_mc_scores_nodes_bytes(b, out, n, od, s, nq, C.byref(need)), need.value


def _sum_bytes(lib, b=2, out=3, n=65, od=2):
    need = C.c_size_t(12345)
    return lib.matgcn_metric_sums_nodes_bytes(b, out, n, od, C.byref(need)), need.value


UNPAIRED = [dict(mean=4096), dict(std=4096), dict(mean2=4096), dict(std2=4096), dict(mean=4096, std=4096, mean2=4096)]
BAD_GEOMETRY = [dict(b=0), dict(b=-1), dict(out=0), dict(out=65), dict(n=0), dict(od=0), dict(od=-2), dict(y_steps=2),
                dict(y_steps=0), dict(y_start=-1), dict(y_start=1), dict(od=3)]


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
    for fn in (ops.metric_sums_nodes, ops.metric_table_rows, ops.mc_scores_nodes, ops.mc_quantiles_scaled,
               MultiATGCN.collect_node_metrics, MultiATGCN.score_mc_nodes, evaluator.NodeEvaluator):
        assert callable(fn)


def test_metric_sums_nodes_arguments_are_checked_on_the_host(lib_built):
    lib = _lib().load()
    for name in ("pred", "y", "sums"):
        assert _sums(lib, **{name: None}) == ERR_NULL, name
    assert _sums(lib, null_scale=True) == ERR_NULL
    for geometry in BAD_GEOMETRY:
        assert _sums(lib, **geometry) == ERR_BAD_ARG, geometry
    for fields in UNPAIRED:
        assert _sums(lib, scale=_scale(**fields)) == ERR_BAD_ARG, fields


def test_metric_table_rows_arguments_are_checked_on_the_host(lib_built):
    lib = _lib().load()
    assert lib.matgcn_metric_table_rows(None, 4, 1, 0, PTR, None) == ERR_NULL
    assert lib.matgcn_metric_table_rows(PTR, 4, 1, 0, None, None) == ERR_NULL
    for rows, fold in ((0, 1), (-1, 1), (4, 0), (4, -2)):
        assert lib.matgcn_metric_table_rows(PTR, rows, fold, 0, PTR, None) == ERR_BAD_ARG, (rows, fold)


def test_mc_scores_nodes_arguments_are_checked_on_the_host(lib_built):
    _l = _lib()
    lib = _l.load()
    for name in ("samples", "y", "scratch", "sums"):
        assert _scores(lib, **{name: None}) == ERR_NULL, name
    assert _scores(lib, null_scale=True) == ERR_NULL and _scores(lib, null_probs=True) == ERR_NULL
    for s in (0, -3, _l.MAX_MC_SAMPLES + 1):
        assert _scores(lib, s=s) == ERR_BAD_ARG, s
    for n in (0, -1, 9):
        assert _scores(lib, probs=(0.1,) * 9, n_probs=n) == ERR_BAD_ARG, n
    for levels in BAD_LEVELS:
        assert _scores(lib, probs=levels) == ERR_BAD_ARG, levels
    for geometry in BAD_GEOMETRY + [dict(y_feat=0)]:
        assert _scores(lib, **geometry) == ERR_BAD_ARG, geometry
    for fields in UNPAIRED:
        assert _scores(lib, scale=_scale(**fields)) == ERR_BAD_ARG, fields
    rc, need = _score_bytes(lib)
    assert rc == OK and need > 0
    assert _scores(lib, scratch_bytes=need - 1) == ERR_SMALL_BUFFER
    assert _scores(lib, scratch_bytes=0) == ERR_SMALL_BUFFER


def test_mc_quantiles_scaled_arguments_are_checked_on_the_host(lib_built):
    _l = _lib()
    lib = _l.load()
    assert _quantiles(lib, samples=None) == ERR_NULL and _quantiles(lib, out=None) == ERR_NULL
    assert _quantiles(lib, null_scale=True) == ERR_NULL and _quantiles(lib, null_probs=True) == ERR_NULL
    for s in (0, -1, _l.MAX_MC_SAMPLES + 1):
        assert _quantiles(lib, s=s) == ERR_BAD_ARG, s
    for bad in (dict(elems=0), dict(elems=-5), dict(n=0), dict(od=0), dict(elems=2 * 3 * 65 * 2 + 1)):
        assert _quantiles(lib, **bad) == ERR_BAD_ARG, bad
    for n in (0, -1, 9):
        assert _quantiles(lib, probs=(0.1,) * 9, n_probs=n) == ERR_BAD_ARG, n
    for levels in BAD_LEVELS:
        assert _quantiles(lib, probs=levels) == ERR_BAD_ARG, levels
    for fields in UNPAIRED:
        assert _quantiles(lib, scale=_scale(**fields)) == ERR_BAD_ARG, fields


def test_scratch_sizes(lib_built):
    """the metric sums need no scratch (a thread walks the batch of its own (horizon, node)); the scores keep one term
    per element and sum, whatever the tile width"""
    lib = _lib().load()
    for b, out, n, od, nq in ((2, 3, 65, 2, 3), (1, 1, 1, 1, 1), (64, 24, 403, 1, 8)):
        assert _sum_bytes(lib, b, out, n, od) == (OK, 0)
        for s in (1, 32, 257, 1024):
            assert _score_bytes(lib, b, out, n, od, s, nq) == (OK, b * out * n * od * (5 + nq) * 8), (s, b, out, n, od, nq)
    assert lib.matgcn_metric_sums_nodes_bytes(2, 3, 65, 2, None) == ERR_NULL
    assert lib.matgcn_mc_scores_nodes_bytes(2, 3, 65, 2, 32, 3, None) == ERR_NULL
    for bad in (dict(b=0), dict(out=0), dict(out=65), dict(n=0), dict(od=0)):
        assert _sum_bytes(lib, **bad)[0] == ERR_BAD_ARG, bad
        assert _score_bytes(lib, **bad)[0] == ERR_BAD_ARG, bad
    for bad in (dict(s=0), dict(s=1025), dict(nq=0), dict(nq=9)):
        assert _score_bytes(lib, **bad)[0] == ERR_BAD_ARG, bad


def test_node_evaluator_arguments(lib_built):
    from multistgraph_amd.evaluator import NodeEvaluator
    ev = NodeEvaluator({}, probs=(0.05, 0.5, 0.95))
    assert ev.score_columns == ["CRPS", "PICP", "MPIW", "WINKLER", "PINBALL_0.05", "PINBALL_0.5", "PINBALL_0.95"]
    for call in (ev.node_table, ev.node_horizon_table, ev.horizon_table, ev.node_scores, ev.node_horizon_scores,
                 ev.horizon_scores, ev.rank):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(ValueError):
        ev.rank("MAPE2")
    for bad in ((), (0.5, 0.1), (-0.1, 0.5), (0.5, 1.5), (NAN,), tuple([0.5] * 9)):
        with pytest.raises(ValueError):
            NodeEvaluator({}, probs=bad)
    for pair in (dict(group_mean=[0.0]), dict(group_std=[1.0])):
        with pytest.raises(ValueError):
            NodeEvaluator({}, **pair)
    with pytest.raises(RuntimeError):
        NodeEvaluator({}).collect_samples(None, None)
    with pytest.raises(ValueError):
        ev.collect_scaled(None, None, 0, mean=1.0)
    plain, group = NodeEvaluator({"min_s": 0.5}), NodeEvaluator({"min_s": 0.5}, group_mean=[0.0], group_std=[1.0], s_small=6)
    assert (plain.min_s, plain.null_val, plain.swap_r2) == (0.5, 0.0, False) and np.isnan(plain.clamp_min)
    assert np.isnan(plain.truth_min)
    assert (group.min_s, group.clamp_min, group.truth_min, group.swap_r2) == (-1.0, 0.0, 6.0, True) and np.isnan(group.null_val)


# ---- the reference against the references it is built from ------------------------------------------------------------
def test_reference_folds_to_the_per_horizon_references(lib_built):
    """the grouped reference added over the nodes is the per-horizon reference; its term tensor is what stage 1 of the
    scores writes, so its size is the scratch the library asks for"""
    c = M.grid_case(5, 3, 4, 7, 2, y_steps=5, y_feat=3, y_start=1, per_node=True, group=True)
    args = (c["pred"], c["y"], 1, c["mean"], c["std"], c["group_mean"], c["group_std"], 0.0, 1.0, 0.125)
    nodes = R.metric_sums_nodes_ref(*args)
    assert nodes.shape == (4, 7, 14) and np.array_equal(nodes.sum(1), M.metric_sums_ref(*args))      # grid: exact sums
    half = R.metric_sums_nodes_ref(*((c["pred"][:1], c["y"][:1]) + args[2:]))
    both = R.metric_sums_nodes_ref(*((c["pred"][1:], c["y"][1:]) + args[2:]), start=half)
    assert np.array_equal(both, nodes)

    rng = np.random.default_rng(3)
    x = rng.standard_normal((9, 2, 3, 5, 2)).astype(np.float32)
    y = rng.standard_normal((2, 3, 5, 2)).astype(np.float32)
    y[0, 0, 0] = 0.0
    probs = (0.05, 0.5, 0.95)
    sums, mag = R.score_sums_nodes(x, y, probs, mean=-1.25, std=3.5)
    assert _score_bytes(_lib().load(), 2, 3, 5, 2, 9, 3) == (OK, R.score_terms_nodes(x, y, probs).size * 8)
    want, _ = MC.score_sums(x, y, probs, mean=-1.25, std=3.5)
    assert np.array_equal(sums[..., 0].sum(1), want[:, 0]) and np.abs(sums.sum(1) - want).max() <= 1e-12 * mag.max()
    # a clamp above every sample: all quantiles are the clamp, the width is 0
    sums, _ = R.score_sums_nodes(x, y + 100.0, probs, clamp_min=50.0)
    assert np.array_equal(sums[..., 3], np.zeros((3, 5))) and (sums[..., 0] == 4).all()
    assert np.array_equal(R.quantiles_nodes(x, probs, clamp_min=50.0), np.full((3, 2, 3, 5, 2), 50.0, dtype=np.float32))
    # the truth filter leaves out what it should
    sums, _ = R.score_sums_nodes(x, y, probs, truth_min=0.25, min_s=-1.0, null_val=NAN)
    assert np.array_equal(sums[..., 0], (y > 0.25).sum(axis=(0, 3)).astype(np.float64))
