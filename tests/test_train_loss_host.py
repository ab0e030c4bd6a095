"""The training objectives on the host (matgcn_loss_bytes, matgcn_loss, matgcn_loss_grad; include/matgcn.h): the numpy
reference (train_loss_ref.py) against what the reference's own loss functions gave (tests/golden/train_loss_small.npz),
symbols, header and binding, the table of names, the constructor's validation of ``hip_train_loss`` and every refusal of
the three entry points - all are made before a launch, so dummy pointers do.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import train_loss_ref as R
from helpers import GOLDEN_DIR, Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(GOLDEN_DIR, "train_loss_small.npz"))
NEW_FUNCTIONS = ("matgcn_loss_bytes", "matgcn_loss", "matgcn_loss_grad")
ELEVEN = ("mae", "mse", "rmse", "mape", "logcosh", "huber", "quantile", "masked_mae", "masked_mse", "masked_rmse",
          "masked_mape")     # traffic_state_executor.py:209-210 without r2 / evar
ZERO_FREE = ("mape", "logcosh", "huber", "quantile")
OK, ERR_NULL, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_SMALL_BUFFER = 0, -1, -2, -3, -4
PTR = C.c_void_p(4096)     # a non-NULL pointer nothing dereferences: every call below fails before its launch
NAN, INF = float("nan"), float("inf")


def _lib():
    from multistgraph_amd import _lib
    return _lib


def gold_inputs(name):
    return (GOLD["pred"], GOLD["y"]) if name in ZERO_FREE else (GOLD["pred_z"], GOLD["y_z"])


# ---- the reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ELEVEN)
def test_reference_reproduces_the_reference_closures_in_float64(name):
    pred, y = gold_inputs(name)
    r = R.train_loss_ref(name, pred, y, 0, float(GOLD["mean"]), float(GOLD["std"]))
    want, g = float(GOLD[name + "_value64"]), GOLD[name + "_grad64"]
    if name in R.LOSSES and R.LOSSES[name][0] in R.MASKED:
        # loss.masked_*_torch weigh by `mask.float()`, a float32 tensor in a float64 run too: mask / mean(mask) is
        # float32(1 / float32(count / n)) on every kept element instead of n / count.  That one constant factor on value
        # and gradient (1 when nothing is masked) is divided out; rmse takes its square root.
        n, cnt = pred.size, r["count"]
        w = float(np.float32(1.0) / (np.float32(cnt) / np.float32(n))) / (n / cnt)
        w = np.sqrt(w) if name.endswith("rmse") else w
        want, g = want / w, g / w
    assert abs(r["value"] - want) <= 1e-12 * abs(want), (r["value"], want)
    fin = np.isfinite(g)
    assert fin.sum() >= g.size - 13
    assert np.abs(r["grad"][fin] - g[fin]).max() <= 1e-12 * np.abs(g[fin]).max()
    # where torch's autograd leaves NaN (0 * inf under the mask) the convention is: no gradient
    assert (r["grad"][~fin] == 0).all()
    # the overall value is the count-weighted mean of the horizons' (their squares for rmse)
    h = r["horizons"]
    assert h.shape == (pred.shape[1],) and np.isfinite(h).all()


@pytest.mark.parametrize("name", ELEVEN)
def test_torch_restatement_reproduces_the_reference_closures(name):
    """train_loss_ref.torch_loss - the yardstick of the GPU tests' realistic bar - does the reference's operations in the
    reference's order: the same bits as the reference's own float32 and float64 runs, value and gradient"""
    import torch
    pred, y = gold_inputs(name)
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        v, g = R.torch_closure(name, pred, y, float(GOLD["mean"]), float(GOLD["std"]), dtype)
        assert np.array_equal(v, GOLD[name + "_value" + tag]), (name, tag, v, GOLD[name + "_value" + tag])
        assert np.array_equal(g, GOLD[name + "_grad" + tag], equal_nan=True), (name, tag)


def test_fixture_holds_the_cases_it_is_for():
    assert sorted(k[:-8] for k in GOLD.files if k.endswith("_value64")) == sorted(ELEVEN)
    l = GOLD["y_z"].astype(np.float64) * float(GOLD["std"]) + float(GOLD["mean"])
    assert (np.abs(l) < 1e-4).sum() >= 13                       # zero labels and one below min_s
    assert (GOLD["pred_z"] == GOLD["y_z"]).sum() >= 1           # p == l
    d = (GOLD["pred"].astype(np.float64) - GOLD["y"]) * float(GOLD["std"])
    assert np.abs(d).max() < 80.0                               # the reference's float32 log(cosh(d)) is finite
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "train_loss_small.npz")) < 100 * 1024


def test_reference_conventions():
    y = np.array([0.0, 1.0, NAN, 2.0]).reshape(1, 1, 4, 1)
    p = np.array([1.0, 1.0, 1.0, 4.0]).reshape(1, 1, 4, 1)
    r = R.train_loss_ref("masked_mape", p, y, 0, 0.0, 1.0)       # l = 0 masked; NaN label: NaN term -> 0, still counted
    assert r["count"] == 3 and r["value"] == (0.0 + 0.0 + 1.0) / 3 and r["grad"].reshape(-1)[2] == 0
    r = R.train_loss_ref("mape", p, y, 0, 0.0, 1.0)              # unmasked zero label: inf, as the reference
    assert r["value"] == INF
    r = R.train_loss_ref("rmse", y[..., 1:2, :], y[..., 1:2, :], 0, 0.0, 1.0)
    assert r["value"] == 0.0 and (r["grad"] == 0).all()          # rmse 0: no gradient (torch: NaN)
    r = R.train_loss_ref("masked_mse", p, np.zeros_like(y), 0, 0.0, 1.0)
    assert r["value"] == 0.0 and r["count"] == 0 and (r["grad"] == 0).all()      # all masked
    assert np.isnan(R.train_loss_ref("huber", p, y, 0, 0.0, 1.0)["value"])       # plain mean: NaN label -> NaN
    big = R.train_loss_ref("logcosh", p * 5000.0, np.zeros_like(y), 0, 0.0, 1.0)     # mean |d| = 8750, far past cosh's range
    assert np.isfinite(big["value"]) and abs(big["value"] - (8750.0 - np.log(2.0))) < 1e-9


# ---- symbols, names, configuration -------------------------------------------------------------------------------------------
def test_library_exports_and_binding(lib_built):
    from multistgraph_amd import ops
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
    assert C.sizeof(_l.LossDesc) == 24
    assert (_l.LOSS_MAE, _l.LOSS_MSE, _l.LOSS_RMSE, _l.LOSS_MAPE, _l.LOSS_LOGCOSH, _l.LOSS_HUBER,
            _l.LOSS_QUANTILE) == tuple(range(7))
    for fn in (ops.train_loss_device, ops.train_loss, MultiATGCN.train_loss):
        assert callable(fn)


def test_name_table_is_the_executors_eleven():
    from multistgraph_amd import _lib as L, ops
    assert sorted(ops.TRAIN_LOSSES) == sorted(ELEVEN) == sorted(R.LOSSES)
    for name in ELEVEN:
        kind, null_val, delta = ops.TRAIN_LOSSES[name]
        assert np.isnan(null_val) if not name.startswith("masked_") else null_val == 0.0, name
        assert delta == R.LOSSES[name][2], name
        d = ops.train_loss_desc(name, 2.0, 3.0)
        assert (d.kind, d.mean, d.std) == (kind, 2.0, 3.0)
        assert d.min_s == np.float32(1e-4) if kind <= L.LOSS_MAPE else d.min_s == 0.0
    assert ops.TRAIN_LOSSES["huber"][2] == 1.0 and ops.TRAIN_LOSSES["quantile"][2] == 0.25
    assert ops.train_loss_desc("quantile", 0.0, 1.0, 0.9).delta == np.float32(0.9)
    assert ops.train_loss_desc("Masked_MSE", 0.0, 1.0).kind == L.LOSS_MSE        # the executor lower-cases the name
    for name in ("r2", "evar"):
        with pytest.raises(ValueError, match="not differentiable"):
            ops.train_loss_desc(name, 0.0, 1.0)
    with pytest.raises(ValueError, match="expected one of"):
        ops.train_loss_desc("smape", 0.0, 1.0)
    for name, delta in (("huber", 0.0), ("huber", -1.0), ("huber", INF), ("quantile", 0.0), ("quantile", 1.0),
                        ("quantile", NAN), ("mae", INF)):
        with pytest.raises(ValueError, match="delta"):
            ops.train_loss_desc(name, 0.0, 1.0, delta)


def test_constructor_validates_hip_train_loss():
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    m = MultiATGCN(c.config(), c.data_feature)
    assert m.hip_train_loss == "none" and m.hip_train_loss_delta is None
    keys = set(m.state_dict())
    for name in ELEVEN:
        mm = MultiATGCN(dict(c.config(), hip_train_loss=name), c.data_feature)
        assert mm.hip_train_loss == name and set(mm.state_dict()) == keys       # an attribute: checkpoints unchanged
    mm = MultiATGCN(dict(c.config(), hip_train_loss="quantile", hip_train_loss_delta=0.9), c.data_feature)
    assert mm.hip_train_loss_delta == 0.9
    for bad in ("r2", "evar", "smape", ""):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_train_loss=bad), c.data_feature)
    with pytest.raises(ValueError, match="delta"):
        MultiATGCN(dict(c.config(), hip_train_loss="quantile", hip_train_loss_delta=1.5), c.data_feature)
    with pytest.raises(ValueError, match="not differentiable"):
        m.train_loss({}, "r2")


# ---- the entry points' refusals -------------------------------------------------------------------------------------------------
def _desc(kind=0, delta=0.0, mean=0.0, std=1.0, null_val=NAN, min_s=1e-4):
    return _lib().LossDesc(kind, mean, std, null_val, min_s, delta)


def _value(lib, pred=PTR, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0, desc=None, null_desc=False,
           scratch=PTR, scratch_bytes=1 << 30, result=PTR):
    d = _desc() if desc is None else desc
    return lib.matgcn_loss(pred, y, None, b, out, n, od, y_steps, y_feat, y_start, None if null_desc else C.byref(d),
                           scratch, scratch_bytes, result, None)


def _grad(lib, pred=PTR, y=PTR, b=2, out=3, n=65, od=2, y_steps=3, y_feat=2, y_start=0, desc=None, null_desc=False,
          scratch=PTR, scratch_bytes=1 << 30, upstream=PTR, d_pred=PTR):
    d = _desc() if desc is None else desc
    return lib.matgcn_loss_grad(pred, y, None, b, out, n, od, y_steps, y_feat, y_start, None if null_desc else C.byref(d),
                                scratch, scratch_bytes, upstream, d_pred, None)


def _bytes(lib, b, out):
    need = C.c_size_t(12345)
    return lib.matgcn_loss_bytes(b, out, C.byref(need)), need.value


BAD_GEOMETRY = [dict(b=0), dict(b=-1), dict(out=0), dict(out=65), dict(n=0), dict(od=0), dict(od=-2), dict(y_steps=2),
                dict(y_steps=0), dict(y_start=-1), dict(y_start=1), dict(od=3)]
BAD_DESC = [dict(kind=-1), dict(kind=7), dict(kind=0, delta=NAN), dict(kind=1, delta=INF), dict(kind=4, delta=-INF),
            dict(kind=5, delta=0.0), dict(kind=5, delta=-1.0), dict(kind=5, delta=INF), dict(kind=6, delta=0.0),
            dict(kind=6, delta=1.0), dict(kind=6, delta=NAN), dict(kind=6, delta=-0.25)]


def test_scratch_size(lib_built):
    lib = _lib().load()
    assert _bytes(lib, 1, 1) == (OK, 8 * (2 + 2))
    assert _bytes(lib, 64, 24) == (OK, 8 * (2 * 64 * 24 + 2))
    assert _bytes(lib, 3, 64) == (OK, 8 * (2 * 3 * 64 + 2))
    for b, out in ((0, 1), (-1, 1), (1, 0), (1, 65)):
        assert _bytes(lib, b, out)[0] == ERR_BAD_ARG, (b, out)
    assert lib.matgcn_loss_bytes(1, 1, None) == ERR_NULL
    assert _bytes(lib, 1 << 30, 2)[0] == ERR_UNSUPPORTED        # B * out workgroups: a 31-bit grid


@pytest.mark.parametrize("call", [_value, _grad], ids=["value", "grad"])
def test_arguments_are_checked_on_the_host(lib_built, call):
    lib = _lib().load()
    pointers = ("pred", "y", "scratch", "result") if call is _value else ("pred", "y", "scratch", "upstream", "d_pred")
    for name in pointers:
        assert call(lib, **{name: None}) == ERR_NULL, name
    assert call(lib, null_desc=True) == ERR_NULL
    for geometry in BAD_GEOMETRY:
        assert call(lib, **geometry) == ERR_BAD_ARG, geometry
    for fields in BAD_DESC:
        assert call(lib, desc=_desc(**fields)) == ERR_BAD_ARG, fields
    need = _bytes(lib, 2, 3)[1]
    assert call(lib, scratch_bytes=need - 1) == ERR_SMALL_BUFFER
    assert call(lib, scratch_bytes=0) == ERR_SMALL_BUFFER
    # the 31-bit guards: a slab's element index is an int, the gradient's grid a 31-bit block count
    assert call(lib, n=1 << 16, od=1 << 15, y_feat=1 << 15) == ERR_UNSUPPORTED
    assert call(lib, b=1 << 20, out=64, y_steps=64, n=1 << 14, scratch_bytes=1 << 40) == ERR_UNSUPPORTED
