"""The pieces every wrapper of multistgraph_amd/ops.py shares, at the smallest shapes that have every axis: B = 2, out = 2,
N = 3, od = 1, label windows (2, 3, 3, 2) read from channel 1, a series (6, 3, 2) with label starts [2, 3], S = 2 samples,
two regions that overlap.

Refusals: every label-reading wrapper refuses a prediction of the wrong rank, labels of another node count and a
label_start of the wrong dtype or length with MatgcnError before anything is called in the library; every wrapper that
writes a caller's tensor (sums=, out=, counts=) refuses a wrong shape, a wrong dtype and a non-contiguous view, and the
refused tensor keeps what it held.
Accumulation: two batches through sums= / counts= give the bits of one call over their concatenation.
train_loss is the (1, 0) case of the tract + region autograd function: its bits, the float64 reference of
tests/train_loss_ref.py under the rules of tests/test_train_loss.py, and an upstream gradient of 2.
bind / backward walk one field map: the keys backward() returns are the recorded ones (tests/golden/backward_keys.json,
in order), and a frozen node_emb gets no entry."""
import gc
import json
import os

import numpy as np
import pytest
import torch

import test_train_loss as TL
import train_loss_ref as R
from helpers import GOLDEN_DIR

pytestmark = pytest.mark.gpu

B, OUT, N, OD, S = 2, 2, 3, 1, 2
Y_STEPS, Y_FEAT, Y_START = 3, 2, 1
PROBS = (0.1, 0.5, 0.9)
MEAN, STD = 1.5, 2.0
SENTINEL = 7.0
F32, F64 = np.float32, np.float64


class Data:
    """two batches of B samples each (the accumulation tests feed them one by one), device tensors made once"""

    def __init__(self):
        from multistgraph_amd.regions import RegionMap
        rng = np.random.default_rng(5)
        self.dev = torch.device("cuda:0")
        y = rng.standard_normal((2 * B, Y_STEPS, N, Y_FEAT))
        y[0, 0, 0, Y_START] = (0.0 - MEAN) / STD        # a label that de-scales to 0: masked by null_val = 0
        pred = y[:, :OUT, :, Y_START:Y_START + OD] + 0.5 * rng.standard_normal((2 * B, OUT, N, OD))
        self.y, self.pred = self.t(y), self.t(pred)
        self.samples = self.t(pred[None] + 0.5 * rng.standard_normal((S, 2 * B, OUT, N, OD)))
        self.series = self.t(rng.standard_normal((6, N, Y_FEAT)))
        self.label_start = torch.tensor([2, 3], dtype=torch.int32, device=self.dev)
        self.regions = RegionMap(N, groups=[[0, 1], [1, 2]])
        torch.cuda.synchronize()

    def t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(self.dev)


@pytest.fixture(scope="module")
def data(lib_built):
    return Data()


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """as tests/test_train_loss.py does: the bindings and autograd nodes made here are gone, and torch's cached blocks
    handed back, before a later module watches which address the caching allocator hands out"""
    yield
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture
def launches(monkeypatch):
    """the names of the library calls the binding makes, in order"""
    from multistgraph_amd import _lib
    names, real = [], _lib.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", recording)
    return names


# ---- refusals of the label geometry ---------------------------------------------------------------------------------------
def _label_wrappers():
    """name -> (what the first argument is, call(data, first argument, y, label_start))"""
    from multistgraph_amd import ops
    loss = (Y_START, MEAN, STD, "mse")
    return {
        "masked_mae_device": ("pred", lambda d, p, y, ls: ops.masked_mae_device(p, y, Y_START, MEAN, STD, 0.0, label_start=ls)),
        "masked_mae_loss": ("pred", lambda d, p, y, ls: ops.masked_mae_loss(p, y, Y_START, MEAN, STD, 0.0, label_start=ls)),
        "train_loss_device": ("pred", lambda d, p, y, ls: ops.train_loss_device(p, y, *loss, label_start=ls)),
        "train_loss": ("pred", lambda d, p, y, ls: ops.train_loss(p, y, *loss, label_start=ls)),
        "metric_sums": ("pred", lambda d, p, y, ls: ops.metric_sums(p, y, Y_START, label_start=ls)),
        "metric_sums_nodes": ("pred", lambda d, p, y, ls: ops.metric_sums_nodes(p, y, Y_START, label_start=ls)),
        "region_loss_device": ("pred", lambda d, p, y, ls: ops.region_loss_device(p, y, d.regions, *loss, label_start=ls)),
        "region_train_loss": ("pred", lambda d, p, y, ls: ops.region_train_loss(p, y, d.regions, *loss, label_start=ls)),
        "tract_region_loss": ("pred", lambda d, p, y, ls: ops.tract_region_loss(p, y, d.regions, *loss, label_start=ls)),
        "mc_scores": ("samples", lambda d, s, y, ls: ops.mc_scores(s, y, PROBS, Y_START, label_start=ls)),
        "mc_scores_nodes": ("samples", lambda d, s, y, ls: ops.mc_scores_nodes(s, y, PROBS, Y_START, label_start=ls)),
        "mc_conformity": ("samples", lambda d, s, y, ls: ops.mc_conformity(s, y, PROBS, Y_START, label_start=ls)),
        "group_label_sums": (None, lambda d, _, y, ls: ops.group_label_sums(y, d.regions, OUT, OD, Y_START, label_start=ls)),
    }


LABEL_WRAPPERS = ("masked_mae_device", "masked_mae_loss", "train_loss_device", "train_loss", "metric_sums",
                  "metric_sums_nodes", "region_loss_device", "region_train_loss", "tract_region_loss", "mc_scores",
                  "mc_scores_nodes", "mc_conformity", "group_label_sums")


def test_the_table_names_every_label_reading_wrapper():
    """a public function of ops.py reads labels where it takes a label_start next to y"""
    import inspect
    from multistgraph_amd import ops
    public = [n for n, f in vars(ops).items() if inspect.isfunction(f) and not n.startswith("_")
              and f.__module__ == ops.__name__ and {"y", "label_start"} <= set(inspect.signature(f).parameters)]
    assert sorted(public) == sorted(LABEL_WRAPPERS) == sorted(_label_wrappers())


@pytest.mark.parametrize("name", LABEL_WRAPPERS)
def test_label_geometry_is_refused_before_any_call(name, data, launches):
    from multistgraph_amd._lib import MatgcnError
    d = data
    first, call = _label_wrappers()[name]
    arg = {"pred": d.pred[:B], "samples": d.samples[:, :B], None: None}[first]
    y = d.y[:B]
    # the arguments every refusal below changes one of are accepted, windows and series
    assert torch.isfinite(call(d, arg, y, None).detach()).any()
    assert torch.isfinite(call(d, arg, d.series, d.label_start).detach()).any()
    assert launches
    refused = {
        "y_nodes": (arg, torch.cat([y, y[:, :, :1]], 2), None),
        "series_nodes": (arg, torch.cat([d.series, d.series[:, :1]], 1), d.label_start),
        "label_start_dtype": (arg, d.series, d.label_start.long()),
        "label_start_on_the_host": (arg, d.series, d.label_start.cpu()),
    }
    if first is None:       # no prediction: the labels alone carry the rank, and label_start IS the batch size
        refused["rank"] = (arg, y[0, 0], None)
    else:
        refused["rank"] = (arg[0], y, None)
        refused["rank_above"] = (arg[None], y, None)
        refused["label_start_length"] = (arg, d.series, torch.cat([d.label_start, d.label_start[:1]]))
    for what, (a, yy, ls) in refused.items():
        del launches[:]
        with pytest.raises(MatgcnError):
            call(d, a, yy, ls)
        assert launches == [], (name, what, launches)


# ---- refusals of a caller's buffer ----------------------------------------------------------------------------------------
def _scores(d):
    from multistgraph_amd import ops
    return ops.mc_conformity(d.samples, d.y, PROBS, Y_START)        # (2 B, out, N, od): a store of 2 B rows


def _buffer_wrappers():
    """name -> (keyword, shape, dtype, call(data, buffer, batch slice))"""
    from multistgraph_amd import ops
    q = len(PROBS)

    def coverage(d, buf, sl):
        scores = _scores(d)[sl]
        margin = torch.full((OUT,), 0.4, dtype=torch.float32, device=d.dev)
        return ops.conformal_coverage(scores, scores.shape[0], "horizon", margin, counts=buf)
    return {
        "metric_sums": ("sums", (OUT, 14), torch.float64,
                        lambda d, buf, sl: ops.metric_sums(d.pred[sl], d.y[sl], Y_START, MEAN, STD, sums=buf)),
        "metric_sums_nodes": ("sums", (OUT, N, 14), torch.float64,
                              lambda d, buf, sl: ops.metric_sums_nodes(d.pred[sl], d.y[sl], Y_START, MEAN, STD, sums=buf)),
        "mc_scores": ("sums", (OUT, 5 + q), torch.float64,
                      lambda d, buf, sl: ops.mc_scores(d.samples[:, sl], d.y[sl], PROBS, Y_START, MEAN, STD, sums=buf)),
        "mc_scores_nodes": ("sums", (OUT, N, 5 + q), torch.float64,
                            lambda d, buf, sl: ops.mc_scores_nodes(d.samples[:, sl], d.y[sl], PROBS, Y_START, MEAN, STD,
                                                                   sums=buf)),
        "conformal_coverage": ("counts", (OUT, 2), torch.int64, coverage),
        "mc_conformity": ("out", (B, OUT, N, OD), torch.float32,
                          lambda d, buf, sl: ops.mc_conformity(d.samples[:, sl], d.y[sl], PROBS, Y_START, out=buf)),
        "group_sums": ("out", (B, OUT, 2, OD), torch.float32,
                       lambda d, buf, sl: ops.group_sums(d.pred[sl], d.regions, out=buf)),
        "group_label_sums": ("out", (B, OUT, 2, OD), torch.float32,
                             lambda d, buf, sl: ops.group_label_sums(d.y[sl], d.regions, OUT, OD, Y_START, out=buf)),
    }


BUFFER_WRAPPERS = ("metric_sums", "metric_sums_nodes", "mc_scores", "mc_scores_nodes", "conformal_coverage",
                   "mc_conformity", "group_sums", "group_label_sums")
ACCUMULATING = BUFFER_WRAPPERS[:5]
FIRST, SECOND, BOTH = slice(0, B), slice(B, 2 * B), slice(0, 2 * B)


def test_the_table_names_every_wrapper_that_writes_a_callers_tensor():
    import inspect
    from multistgraph_amd import ops
    public = [n for n, f in vars(ops).items() if inspect.isfunction(f) and not n.startswith("_")
              and f.__module__ == ops.__name__ and {"sums", "out", "counts"} & set(inspect.signature(f).parameters)]
    public = [n for n in public if n not in ("metric_table", "metric_table_rows")]     # they READ sums
    assert sorted(public) == sorted(BUFFER_WRAPPERS) == sorted(_buffer_wrappers())


@pytest.mark.parametrize("name", BUFFER_WRAPPERS)
def test_a_callers_buffer_is_checked_once_and_strictly(name, data, launches):
    from multistgraph_amd._lib import MatgcnError
    d = data
    kw, shape, dtype, call = _buffer_wrappers()[name]
    other = {torch.float64: torch.float32, torch.float32: torch.float64, torch.int64: torch.int32}[dtype]

    def full(shp, dt=dtype):
        return torch.full(shp, SENTINEL, dtype=dt, device=d.dev)
    good = full(shape)
    if name in ACCUMULATING:
        good.zero_()
    assert call(d, good, FIRST) is good                     # the caller's own tensor is written and returned
    assert not torch.equal(good, full(shape))
    wide = full(shape[:-1] + (2 * shape[-1],))
    view = wide[..., ::2]
    assert tuple(view.shape) == shape and not view.is_contiguous()
    refused = {"shape": full(shape[:-1] + (shape[-1] + 1,)), "fewer_axes": full(shape[1:]), "dtype": full(shape, other),
               "non_contiguous": view}
    fresh = call(d, None, FIRST)
    for what, buf in refused.items():
        base = wide if what == "non_contiguous" else buf
        del launches[:]
        with pytest.raises(MatgcnError):
            call(d, buf, FIRST)
        assert not [n for n in launches if n.endswith(name)], (name, what, launches)
        assert torch.equal(base, torch.full_like(base, SENTINEL)), (name, what)
    assert torch.equal(call(d, None, FIRST), fresh)


@pytest.mark.parametrize("name", ACCUMULATING)
def test_two_batches_through_the_buffer_are_one_call_over_both(name, data):
    d = data
    kw, shape, dtype, call = _buffer_wrappers()[name]
    whole = call(d, None, BOTH)
    running = call(d, None, FIRST)
    assert not torch.equal(running, whole)
    assert call(d, running, SECOND) is running
    assert torch.equal(running, whole), (name, (running.double() - whole.double()).abs().max())
    assert tuple(whole.shape) == shape and whole.dtype == dtype and float(whole.double().abs().sum()) > 0.0


# ---- train_loss through the tract + region autograd function ---------------------------------------------------------------
def _grid():
    return R.grid_case(11, B, OUT, N, OD, y_steps=Y_STEPS, y_feat=Y_FEAT, y_start=Y_START)


def _loss_and_grad(fn, c, upstream=None):
    p = TL._dev(c["pred"]).requires_grad_(True)
    loss = fn(p, TL._dev(c["y"]))
    (loss if upstream is None else upstream * loss).backward()
    return loss.detach(), p.grad


@pytest.mark.parametrize("name", sorted(R.LOSSES))
def test_train_loss_is_the_tract_half_of_the_merged_function(name, data, launches):
    from multistgraph_amd import ops
    assert sorted(ops.TRAIN_LOSSES) == sorted(R.LOSSES)
    c = _grid()
    args = (c["y_start"], c["mean"], c["std"], name)
    loss, grad = _loss_and_grad(lambda p, y: ops.train_loss(p, y, *args), c)
    assert launches == ["matgcn_loss_bytes", "matgcn_loss", "matgcn_loss_grad"]     # nothing of the region half
    both, both_grad = _loss_and_grad(
        lambda p, y: ops.tract_region_loss(p, y, data.regions, *args, tract_weight=1, region_weight=0), c)
    assert torch.equal(loss, both) and torch.equal(grad, both_grad)
    # the float64 reference, under the rules of test_train_loss.py: exact on the grid, logcosh against the float32 torch run
    want = TL._ref(name, c, upstream=1.0)
    value, g = np.asarray([TL._host(loss)], dtype=F32), TL._host(grad)
    if name in TL.EXACT_NAMES + TL.MAPE_NAMES:
        R.assert_exact(name, c)
        TL._assert_exact_values(name, value, dict(values=want["values"][:1]))
        TL._assert_exact_grad(name, g, want)
    else:
        slab = c["y"][:, :OUT, :, Y_START:Y_START + OD]
        v32, g32 = R.torch_closure(name, c["pred"], slab, c["mean"], c["std"], torch.float32)
        gmax = np.abs(want["grad"]).max()
        gap_v = abs(float(v32) - want["value"]) / abs(want["value"])
        gap_g = float(np.abs(g32.astype(F64) - want["grad"]).max() / gmax)
        err_v = abs(float(value[0]) - want["value"]) / abs(want["value"])
        err_g = float(np.abs(g.astype(F64) - want["grad"]).max() / gmax)
        print("%s: value torch32 gap %.3g ours %.3g, gradient torch32 gap %.3g ours %.3g" % (name, gap_v, err_v, gap_g, err_g))
        assert err_v <= TL._bar(gap_v) and err_g <= TL._bar(gap_g)
    # an upstream gradient of 2: the same value, exactly twice the gradient
    loss2, grad2 = _loss_and_grad(lambda p, y: ops.train_loss(p, y, *args), c, upstream=2.0)
    assert torch.equal(loss2, loss) and torch.equal(grad2, 2.0 * grad)
    assert float(grad.abs().max()) > 0.0


# ---- bind() and backward() walk one field map -------------------------------------------------------------------------------
with open(os.path.join(GOLDEN_DIR, "backward_keys.json")) as _fh:
    BACKWARD_KEYS = json.load(_fh)      # recorded from HotPath.backward before bind() and backward() shared their walk


@pytest.mark.parametrize("case", ["l2_n33_b3", "gcnoff_l3"])
def test_backward_returns_the_recorded_keys(case, lib_built):
    from test_stream_order import Binding, CASES
    assert case in CASES and CASES["gcnoff_l3"][3] == {"gcn_off": True} and CASES["l2_n33_b3"][3] == {}
    bd = Binding(case)
    hp = bd.hp
    hp.deterministic = True
    try:
        hp.forward_train(bd.x)
        grads = hp.backward(bd.x, bd.d_out, bd.state)
        assert list(grads) == BACKWARD_KEYS[case]
        assert set(grads) == {k for k in bd.state if not k.startswith("static_initial")}
        assert all(torch.isfinite(v).all() for v in grads.values())
        # a frozen node_emb (a Parameter that takes no gradient) gets no entry; every other gradient keeps its bits
        frozen = dict(bd.state, node_emb=torch.nn.Parameter(bd.state["node_emb"], requires_grad=False))
        hp.forward_train(bd.x)
        again = hp.backward(bd.x, bd.d_out, frozen)
        assert list(again) == [k for k in BACKWARD_KEYS[case] if k != "node_emb"]
        assert all(torch.equal(again[k], grads[k]) for k in again)
    finally:
        hp.deterministic = None
