"""Ensemble training (CRPS over dropout samples) without a GPU: symbols, header and binding, every refusal of the entry
points - all made before a launch, so dummy pointers do -, the label-geometry table of the two CRPS entry points against
matgcn_mc_scores', the constructor's validation of the two config keys, and the numpy reference crps_ref.py against the
pairwise form and against central differences."""
import ctypes as C
import os

import numpy as np
import pytest

import crps_ref as R
from helpers import Case
from test_label_geometry_host import BASE, ENTRIES, REFUSED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_train_mc_bytes", "matgcn_forward_train_mc", "matgcn_backward_mc", "matgcn_crps_loss_bytes",
                 "matgcn_crps_loss", "matgcn_crps_loss_grad")
NULL, BAD_ARG, UNSUPPORTED, SMALL = -1, -2, -3, -4
PTR = C.c_void_p(4096)     # a non-NULL, aligned pointer nothing dereferences
NAN = float("nan")
BIG = 1 << 40


def _L():
    from multistgraph_amd import _lib
    return _lib


def test_library_exports_and_binding(lib_built):
    L = _L()
    header = open(os.path.join(ROOT, "include", "matgcn.h")).read()
    lib = L.load()
    for name in NEW_FUNCTIONS:
        assert name in L.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12 and L.ABI_VERSION == 12
    from multistgraph_amd import ops
    for method in ("forward_train_mc", "backward_mc"):
        assert callable(getattr(ops.HotPath, method))
    assert callable(ops.crps_loss) and callable(ops.crps_loss_device)


# ---- matgcn_crps_loss / matgcn_crps_loss_grad ---------------------------------------------------------------------------------
def _crps(lib, entry, samples=PTR, s=8, y=PTR, series=False, batch=2, out_steps=3, nodes=5, out_dim=2, y_steps=3, y_feat=3,
          y_start=1, scratch=PTR, scratch_bytes=BIG, out=PTR):
    head = (samples, s, y, PTR if series else None, batch, out_steps, nodes, out_dim, y_steps, y_feat, y_start, 0.0, 1.0, NAN,
            1e-4, scratch, scratch_bytes)
    if entry == "matgcn_crps_loss":
        return lib.matgcn_crps_loss(*head, out, None)
    return lib.matgcn_crps_loss_grad(*head, 1.0, out, None)


@pytest.mark.parametrize("entry", ["matgcn_crps_loss", "matgcn_crps_loss_grad"])
def test_crps_refusals(entry, lib_built):
    lib = _L().load()
    for kw in (dict(samples=None), dict(y=None), dict(scratch=None), dict(out=None)):
        assert _crps(lib, entry, **kw) == NULL, kw
    for s in (0, -1, 1025):
        assert _crps(lib, entry, s=s) == BAD_ARG, s
    assert _crps(lib, entry, batch=0) == BAD_ARG
    need = C.c_size_t()
    assert lib.matgcn_crps_loss_bytes(2, 3, C.byref(need)) == 0 and need.value == (2 * 2 * 3 + 2) * 8
    assert _crps(lib, entry, scratch_bytes=need.value - 1) == SMALL
    assert lib.matgcn_crps_loss_bytes(2, 3, None) == NULL
    assert lib.matgcn_crps_loss_bytes(0, 3, C.byref(need)) == BAD_ARG
    assert lib.matgcn_crps_loss_bytes(2, 65, C.byref(need)) == BAD_ARG
    loss_need = C.c_size_t()
    assert lib.matgcn_loss_bytes(7, 24, C.byref(loss_need)) == 0 and lib.matgcn_crps_loss_bytes(7, 24, C.byref(need)) == 0
    assert need.value == loss_need.value


@pytest.mark.parametrize("entry", ["matgcn_crps_loss", "matgcn_crps_loss_grad"])
def test_crps_label_geometry_is_that_of_mc_scores(entry, lib_built):
    """the table of tests/test_label_geometry_host.py, column matgcn_mc_scores: the same cases are refused with the same
    status, the case it accepts (a series shorter than out_steps) is not refused for its geometry here either; the one
    difference is the cap of 64 horizons, which comes with matgcn_loss's scratch and second stage"""
    lib = _L().load()
    col = ENTRIES.index("matgcn_mc_scores")
    applied = 0
    for name, fields, status in REFUSED:
        f = dict(BASE, **fields)
        got = _crps(lib, entry, series=f.pop("series"), **f)
        if name == "horizons_past_the_cap":
            assert status[col] is None and got == BAD_ARG
            continue
        if status[col] is None:      # accepted by the rule: it would launch, so only its scratch is made too small here
            assert _crps(lib, entry, scratch_bytes=0, **dict(f, series=True)) == SMALL, name
            continue
        assert got == status[col] != 0, (entry, name)
        applied += 1
    assert applied >= 9


# ---- matgcn_forward_train_mc / matgcn_backward_mc ------------------------------------------------------------------------------
def _dims(**flags):
    from multistgraph_amd.ops import spec_from_config
    c = Case("tiny_multi_uni_c2")
    return spec_from_config(dict(c.config(), **flags), c.data_feature, c.n, min(c.n, 20), 0, 0).dims(c.b)


def _params():
    L = _L()
    p = L.Params()
    for name, _ in L.Params._fields_:
        v = getattr(p, name)
        if isinstance(v, C.Array):
            for i in range(len(v)):
                if isinstance(v[i], C.Structure):
                    for fn, _ in v[i]._fields_:
                        setattr(v[i], fn, 4096)
                else:
                    v[i] = 4096
        else:
            setattr(p, name, 4096)
    return p


def _fwd(lib, dims, drop=None, samples=4, X=PTR, out=PTR, ws=PTR, wsb=BIG, train=PTR, trb=BIG, prepared=PTR, has_drop=True):
    L = _L()
    d = drop if drop is not None else L.Dropout(1, 0, 0.1)
    return lib.matgcn_forward_train_mc(C.byref(dims), C.byref(_params()), prepared, X, None, None,
                                       C.byref(d) if has_drop else None, samples, None, None, out, ws, wsb, train, trb, None)


def _bwd(lib, dims, drop=None, samples=4, X=PTR, d_samples=PTR, grads=True, ws=PTR, wsb=BIG, train=PTR, trb=BIG,
         prepared=PTR, has_drop=True):
    L = _L()
    d = drop if drop is not None else L.Dropout(1, 0, 0.1)
    g = _params()
    return lib.matgcn_backward_mc(C.byref(dims), C.byref(_params()), prepared, X, None, None,
                                  C.byref(d) if has_drop else None, samples, d_samples, C.byref(g) if grads else None, None,
                                  ws, wsb, train, trb, None)


def test_train_mc_bytes(lib_built):
    lib = _L().load()
    dims = _dims()
    plain, mc4, mc32 = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert lib.matgcn_train_bytes(C.byref(dims), C.byref(plain)) == 0
    assert lib.matgcn_train_mc_bytes(C.byref(dims), 4, C.byref(mc4)) == 0
    assert lib.matgcn_train_mc_bytes(C.byref(dims), 32, C.byref(mc32)) == 0
    assert plain.value < mc4.value <= mc32.value
    # the existing query is what it was in every setting, and the ensemble buffer covers each of them
    for setter, value in ((lib.matgcn_set_deterministic, 1), (lib.matgcn_set_train_precision, 2),
                          (lib.matgcn_set_train_bf16x3, 1)):
        prev = setter(value)
        try:
            other, again = C.c_size_t(), C.c_size_t()
            assert lib.matgcn_train_bytes(C.byref(dims), C.byref(other)) == 0
            assert lib.matgcn_train_mc_bytes(C.byref(dims), 4, C.byref(again)) == 0
            assert other.value >= plain.value and again.value == mc4.value and other.value < mc4.value
        finally:
            setter(prev)
    for s in (0, -3, 1025):
        assert lib.matgcn_train_mc_bytes(C.byref(dims), s, C.byref(mc4)) == BAD_ARG
    assert lib.matgcn_train_mc_bytes(C.byref(dims), 4, None) == NULL


def test_forward_train_mc_refusals(lib_built):
    L = _L()
    lib = L.load()
    dims = _dims()
    assert _fwd(lib, dims, has_drop=False) == NULL
    assert _fwd(lib, dims, out=None) == NULL
    assert _fwd(lib, dims, X=None) == NULL
    assert _fwd(lib, dims, train=None) == NULL
    assert _fwd(lib, dims, prepared=None) == NULL
    assert _fwd(lib, dims, ws=None) == NULL
    for s in (0, -1, 1025):
        assert _fwd(lib, dims, samples=s) == BAD_ARG
    for p in (1.0, -0.1, NAN):
        assert _fwd(lib, dims, drop=L.Dropout(1, 0, p)) == BAD_ARG
    need, plain = C.c_size_t(), C.c_size_t()
    assert lib.matgcn_train_mc_bytes(C.byref(dims), 4, C.byref(need)) == 0
    assert lib.matgcn_train_bytes(C.byref(dims), C.byref(plain)) == 0
    assert _fwd(lib, dims, trb=need.value - 4) == SMALL
    assert _fwd(lib, dims, trb=plain.value) == SMALL           # a buffer of the plain training step is too small
    assert _fwd(lib, dims, wsb=64) == SMALL
    # the limits of k_head_mc: more than 64 output channels
    wide = _dims(output_window=65)
    assert _fwd(lib, wide) == UNSUPPORTED


def test_backward_mc_refusals(lib_built):
    L = _L()
    lib = L.load()
    dims = _dims()
    assert _bwd(lib, dims, has_drop=False) == NULL
    assert _bwd(lib, dims, d_samples=None) == NULL
    assert _bwd(lib, dims, grads=False) == NULL
    assert _bwd(lib, dims, X=None) == NULL
    assert _bwd(lib, dims, train=None) == NULL
    for s in (0, 1025):
        assert _bwd(lib, dims, samples=s) == BAD_ARG
    assert _bwd(lib, dims, drop=L.Dropout(1, 0, 1.0)) == BAD_ARG
    need = C.c_size_t()
    assert lib.matgcn_train_mc_bytes(C.byref(dims), 4, C.byref(need)) == 0
    assert _bwd(lib, dims, trb=need.value - 4) == SMALL
    assert _bwd(lib, _dims(output_window=65)) == UNSUPPORTED


# ---- the model's config keys -----------------------------------------------------------------------------------------------------
def test_constructor_validates_the_crps_keys():
    from multistgraph_amd._lib import MAX_MC_SAMPLES
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    base = MultiATGCN(c.config(), c.data_feature)
    assert base.hip_train_loss == "none" and base.hip_train_samples == 16
    m = MultiATGCN(dict(c.config(), hip_train_loss="crps", hip_dropout="device"), c.data_feature)
    assert m.hip_train_loss == "crps" and m.hip_train_samples == 16
    assert set(m.state_dict()) == set(base.state_dict())           # attributes: checkpoints unchanged
    m = MultiATGCN(dict(c.config(), hip_train_loss="crps", hip_dropout="device", hip_train_samples=MAX_MC_SAMPLES),
                   c.data_feature)
    assert m.hip_train_samples == MAX_MC_SAMPLES
    for dropout in ("torch", None):
        cfg = dict(c.config(), hip_train_loss="crps")
        if dropout:
            cfg["hip_dropout"] = dropout
        with pytest.raises(ValueError, match="device"):
            MultiATGCN(cfg, c.data_feature)
    for bad in (0, -1, MAX_MC_SAMPLES + 1, 2.5, "8", None, True):
        with pytest.raises(ValueError, match="hip_train_samples"):
            MultiATGCN(dict(c.config(), hip_train_loss="crps", hip_dropout="device", hip_train_samples=bad), c.data_feature)
        with pytest.raises(ValueError, match="hip_train_samples"):
            MultiATGCN(dict(c.config(), hip_train_samples=bad), c.data_feature)
    with pytest.raises(NotImplementedError, match="region"):
        MultiATGCN(dict(c.config(), hip_train_loss="crps", hip_dropout="device", hip_train_regions=[0] * c.n),
                   c.data_feature)
    with pytest.raises(ValueError, match="samples"):
        base.train_loss({}, "crps", samples=0)
    with pytest.raises(NotImplementedError, match="region"):
        base.train_loss({}, "crps", regions=[0] * c.n)
    # a step consumes S offsets
    assert [m._dropout_offset(8), m._dropout_offset(8)] == [0, 8]


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _data(s, geometry=(2, 3, 7, 2), seed=0, grid=False):
    rng = np.random.default_rng(seed + 31 * s)
    x = rng.standard_normal((s,) + geometry).astype(np.float32)
    y = rng.standard_normal(geometry).astype(np.float32)
    if grid:
        x, y = np.round(x * 4) / 4, np.round(y * 4) / 4
    y[rng.random(geometry) < 0.15] = 0.0
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("s", [1, 2, 5, 32, 33])
def test_reference_value_is_the_pairwise_form(s):
    x, y = _data(s)
    scale = dict(mean=-1.25, std=3.5)      # a raw label 0 de-scales to -1.25: that is the null value here
    p = R.M.descale(x, **scale)
    l, mask = R.M.labels(y, null_val=-1.25, **scale)
    sorted_form, pair = R.element_crps(p, l), R.pairwise(x, y, **scale)
    assert np.abs(sorted_form - pair).max() <= 1e-12 * max(1.0, np.abs(pair).max())
    res, exact, m = R.value(x, y, null_val=-1.25, **scale)
    assert m == mask.sum() and 0 < m < mask.size
    assert abs(exact[0] - pair[mask].sum() / m) <= 1e-12 * abs(exact[0])
    for k in range(3):
        assert abs(exact[1 + k] - pair[:, k][mask[:, k]].mean()) <= 1e-12 * abs(exact[1 + k])
    assert res.dtype == np.float32 and res.shape == (4,)
    # a whole horizon masked: its entry is 0, the total is over the others
    y2 = y.copy()
    y2[:, 1] = 0.0
    res2, exact2, m2 = R.value(x, y2, mean=0.0, std=1.0, null_val=0.0)
    assert res2[2] == 0.0 and m2 == (y2 != 0).sum()
    assert R.value(x, np.zeros_like(y), null_val=0.0)[0].tolist() == [0.0] * 4
    assert not R.grad(x, np.zeros_like(y), null_val=0.0).any()


def test_reference_ranks_break_ties_by_sample_index():
    p = np.array([[1.0], [0.5], [1.0], [0.5], [2.0]], dtype=np.float32)
    assert R.ranks(p)[:, 0].tolist() == [2, 0, 3, 1, 4]
    # all tied: the ranks are the sample indices, the gradients differ per sample and add up to the MAE gradient
    x = np.broadcast_to(np.float32(1.5), (4, 1, 1, 1, 1)).copy()
    y = np.full((1, 1, 1, 1), 0.25, dtype=np.float32)
    g = R.grad(x, y)
    assert g[:, 0, 0, 0, 0].tolist() == [(1 / 4) - (2 * r - 3) / 16 for r in range(4)]
    assert g.sum() == 1.0


@pytest.mark.parametrize("s", [1, 2, 5, 33])
def test_reference_gradient_by_central_differences(s):
    """away from ties and from the labels the CRPS is piecewise linear in every sample: central differences in float64 of
    the float64 pairwise form are exact up to rounding"""
    geometry = (2, 3, 5, 1)
    x, y = _data(s, geometry, seed=3)
    scale = dict(mean=0.5, std=2.0)
    g = R.grad(x, y, null_val=0.0, upstream=0.75, **scale)
    l, mask = R.M.labels(y, null_val=0.0, **scale)
    m = mask.sum()

    def total(xx):      # float64 throughout: the de-scale of the reference's float32 values, continued exactly
        p = xx * 2.0 + 0.5
        pair = np.zeros(geometry)
        for i in range(s):
            pair += np.abs(p - p[i][None]).sum(0)
        c = np.abs(p - l.astype(np.float64)[None]).mean(0) - 0.5 * pair / (s * s)
        return 0.75 * c[mask].sum() / m

    x64 = x.astype(np.float64)
    p = x64 * 2.0 + 0.5
    gaps = np.abs(p[:, None] - p[None]) + np.eye(s).reshape((s, s) + (1,) * 4) * 1e9
    h = 0.25 * min(gaps.min(), np.abs(p - l[None]).min()) / 2.0
    assert h > 1e-7
    rng = np.random.default_rng(0)
    for _ in range(40):
        at = tuple(rng.integers(0, d) for d in x.shape)
        up, dn = x64.copy(), x64.copy()
        up[at] += h
        dn[at] -= h
        fd = (total(up) - total(dn)) / (2 * h)
        assert abs(fd - g[at]) <= 1e-6 * max(abs(g).max(), 1e-30), (at, fd, g[at])
