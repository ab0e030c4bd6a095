"""Quantiles and scores of a Monte-Carlo-dropout ensemble, on the host: the library surface (symbols, header, binding),
every argument check of the three entry points - they run before any launch, so they need no GPU -, and the numpy
reference against itself: its sorted CRPS against the O(S^2) form, its float32 quantile against np.quantile in float64."""
import ctypes as C
import os

import numpy as np
import pytest

import mc_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_mc_quantiles", "matgcn_mc_scores_bytes", "matgcn_mc_scores")
OK, ERR_NULL, ERR_BAD_ARG, ERR_SMALL_BUFFER = 0, -1, -2, -4
PTR = C.c_void_p(4096)     # a non-NULL pointer nothing dereferences: every call below fails before its launch


def test_library_exports_and_binding(lib_built):
    from multistgraph_amd import _lib, evaluator, ops
    from multistgraph_amd.model import MultiATGCN
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    lib = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "#define MATGCN_MAX_MC_QUANTILES 8" in header and "#define MATGCN_MC_SCORE_SUMS 5" in header
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12 == _lib.ABI_VERSION
    assert _lib.MAX_MC_QUANTILES == 8 and _lib.MC_SCORE_SUMS == 5
    assert callable(ops.mc_quantiles) and callable(ops.mc_scores)
    assert callable(MultiATGCN.predict_interval) and callable(MultiATGCN.score_mc)
    ev = evaluator.ProbabilisticEvaluator({}, probs=(0.05, 0.5, 0.95))
    assert ev.columns == ["CRPS", "PICP", "MPIW", "WINKLER", "PINBALL_0.05", "PINBALL_0.5", "PINBALL_0.95"]
    with pytest.raises(RuntimeError):
        ev.table()
    for bad in ((), (0.5, 0.1), (-0.1, 0.5), (0.5, 1.5), (float("nan"),), tuple([0.5] * 9)):
        with pytest.raises(ValueError):
            evaluator.ProbabilisticEvaluator({}, probs=bad)


def _probs(*vals):
    return (C.c_float * max(1, len(vals)))(*vals), len(vals)


BAD_LEVELS = [(-0.01,), (1.01,), (float("nan"),), (0.5, 0.25), (0.1, float("nan"), 0.9), (0.0, 0.5, 0.5, 0.4)]


def _quantiles(lib, samples=PTR, s=32, elems=100, probs=(0.05, 0.5, 0.95), n_probs=None, out=PTR):
    arr, n = _probs(*probs)
    return lib.matgcn_mc_quantiles(samples, s, elems, arr if probs is not None else None, n if n_probs is None else n_probs,
                                   0.0, 1.0, out, None)


def test_quantile_arguments_are_checked_on_the_host(lib_built):
    from multistgraph_amd import _lib
    lib = _lib.load()
    assert _quantiles(lib, samples=None) == ERR_NULL
    assert _quantiles(lib, out=None) == ERR_NULL
    assert lib.matgcn_mc_quantiles(PTR, 32, 100, None, 3, 0.0, 1.0, PTR, None) == ERR_NULL
    for s in (0, -1, _lib.MAX_MC_SAMPLES + 1):
        assert _quantiles(lib, s=s) == ERR_BAD_ARG, s
    for elems in (0, -5):
        assert _quantiles(lib, elems=elems) == ERR_BAD_ARG, elems
    for n in (0, -1, 9):
        assert _quantiles(lib, probs=(0.1,) * 9, n_probs=n) == ERR_BAD_ARG, n
    for levels in BAD_LEVELS:
        assert _quantiles(lib, probs=levels) == ERR_BAD_ARG, levels


def _scores(lib, samples=PTR, s=32, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0,
            probs=(0.05, 0.5, 0.95), n_probs=None, scratch=PTR, scratch_bytes=1 << 40, sums=PTR, label_start=None):
    arr, k = _probs(*probs)
    return lib.matgcn_mc_scores(samples, s, y, label_start, b, out, n, od, y_steps, y_feat, y_start, 0.0, 1.0, 0.0, 1e-4,
                                arr, k if n_probs is None else n_probs, scratch, scratch_bytes, sums, 0, None)


def _bytes(lib, b=2, out=3, n=65, od=2, s=32, nq=3):
    need = C.c_size_t(0)
    return lib.matgcn_mc_scores_bytes(b, out, n, od, s, nq, C.byref(need)), need.value


def test_score_arguments_are_checked_on_the_host(lib_built):
    from multistgraph_amd import _lib
    lib = _lib.load()
    for name in ("samples", "y", "scratch", "sums"):
        assert _scores(lib, **{name: None}) == ERR_NULL, name
    assert lib.matgcn_mc_scores(PTR, 32, PTR, None, 2, 3, 65, 2, 3, 2, 0, 0.0, 1.0, 0.0, 1e-4, None, 3, PTR, 1 << 40, PTR, 0,
                                None) == ERR_NULL
    for s in (0, -3, _lib.MAX_MC_SAMPLES + 1):
        assert _scores(lib, s=s) == ERR_BAD_ARG, s
    for n in (0, -1, 9):
        assert _scores(lib, probs=(0.1,) * 9, n_probs=n) == ERR_BAD_ARG, n
    for levels in BAD_LEVELS:
        assert _scores(lib, probs=levels) == ERR_BAD_ARG, levels
    for geometry in (dict(b=0), dict(b=-1), dict(out=0), dict(n=0), dict(od=0), dict(od=-2), dict(y_steps=2), dict(y_steps=0),
                     dict(y_feat=0), dict(y_start=-1), dict(y_start=1), dict(od=3)):
        assert _scores(lib, **geometry) == ERR_BAD_ARG, geometry
    rc, need = _bytes(lib)
    assert rc == OK and need > 0
    assert _scores(lib, scratch_bytes=need - 1) == ERR_SMALL_BUFFER
    assert _scores(lib, scratch_bytes=0) == ERR_SMALL_BUFFER


def test_scratch_size(lib_built):
    """one partial of 5 + n_probs doubles per tile; a tile never straddles a (b, horizon) row of N*od elements and is 64
    elements wide up to S = 256, 32 up to 512, 16 up to 1024"""
    from multistgraph_amd import _lib
    lib = _lib.load()
    for s, tile in ((1, 64), (32, 64), (256, 64), (257, 32), (512, 32), (513, 16), (1024, 16)):
        for b, out, n, od, nq in ((2, 3, 65, 2, 3), (1, 1, 1, 1, 1), (64, 6, 403, 1, 8)):
            rc, need = _bytes(lib, b, out, n, od, s, nq)
            assert rc == OK and need == b * out * -(-n * od // tile) * (5 + nq) * 8, (s, b, out, n, od, nq)
    assert lib.matgcn_mc_scores_bytes(2, 3, 65, 2, 32, 3, None) == ERR_NULL
    for bad in (dict(b=0), dict(out=0), dict(n=0), dict(od=0), dict(s=0), dict(s=1025), dict(nq=0), dict(nq=9)):
        assert _bytes(lib, **bad)[0] == ERR_BAD_ARG, bad


@pytest.mark.parametrize("s", [1, 2, 3, 33, 100, 1024])
def test_sorted_crps_equals_the_pairwise_form(s):
    rng = np.random.default_rng(s)
    x = (3.5 * rng.standard_normal((s, 40)) - 1.25).astype(np.float32)
    l = rng.standard_normal(40).astype(np.float32)
    fast, brute = R.crps_sorted(np.sort(x, axis=0), l), R.crps_brute(x, l)
    err = np.abs(fast - brute).max() / np.abs(brute).max()
    print("S = %d: sorted against pairwise CRPS, relative error %.2e" % (s, err))
    assert err <= 1e-12


@pytest.mark.parametrize("s", [1, 2, 3, 31, 32, 33, 100, 257, 1024])
def test_float32_quantile_against_numpy(s):
    rng = np.random.default_rng(100 + s)
    x = rng.standard_normal((s, 500)).astype(np.float32)
    probs = (0.0, 0.05, 0.5, 0.95, 1.0)
    got = R.quantiles(x, probs)
    want = np.quantile(x.astype(np.float64), [float(np.float32(q)) for q in probs], axis=0)
    err = np.abs(got.astype(np.float64) - want).max() / np.abs(x).max()
    print("S = %d: float32 quantile against np.quantile, error / max|x| %.2e" % (s, err))
    assert got.dtype == np.float32 and err <= 1e-6
    assert np.array_equal(got[0], x.min(0)) and np.array_equal(got[-1], x.max(0))
