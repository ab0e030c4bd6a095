"""Ensemble training on the GPU: matgcn_crps_loss / matgcn_crps_loss_grad against the numpy reference crps_ref.py,
matgcn_forward_train_mc against matgcn_forward_mc and matgcn_forward_train, matgcn_backward_mc against the sum of the
project's own explicit-mask backward over the samples and against float64 autograd through the oracle, and the model
surface (config['hip_train_loss'] = "crps").

Bounds.
CRPS on grid-valued inputs (samples and labels on multiples of 1/4, std a power of two, mean on the grid: no float32
operation rounds, and the fp64 sums |p - l| and (2i - S + 1) p are exact in any order): value bit-equal to float32 of the
reference and to float32(sum CRPS / count) of matgcn_mc_scores' sums; gradient within one float32 ulp of the reference,
exactly 0 where that is 0.  On continuous data both stay within twice the gap of a float32 torch run of the same
arithmetic against float64 (floor 2^-22), the bar of tests/test_train_loss.py.
matgcn_backward_mc against the float64 sum over s of matgcn_forward_train / matgcn_backward with the explicit mask of
offset + s and d_out = d_samples[s]: 2e-4 max-normalised per tensor (both sides are fp32 paths, each held to the project's
1e-4).  The cases in the bf16 training modes 1 and 2 run ONE sample: the sum over samples is a reference only where the
arithmetic behind the head is linear in the head's gradient, and rounding the summed sequence gradient to bf16 is not the
sum of the rounded ones; at S = 1 both sides round the same tensor (up to the fp32 order of the head product).  The
three-piece mode is fp32-accurate and runs two samples.
End to end against float64 (oracle.encoder -> oracle.output_head(seq * mask_s), CRPS by torch.sort, autograd): 1e-4
max-normalised, the project's gradient tolerance.
The figures the tests print are recorded in DESIGN.md section 5d.4."""
import ctypes as C
import gc

import numpy as np
import pytest
import torch

import crps_ref as R
import mc_scores_ref as M
from helpers import max_norm_err
from stream_gate import bits_equal, sandwich

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -22
SEED, P = 1234, 0.1
SUM_TOL = 2e-4
ORACLE_TOL = 1e-4
GUARD = 256
SAMPLES = (1, 2, 5, 32, 33, 257)
GEOMETRIES = ((3, 3, 65, 1), (3, 24, 65, 2))
GRID_SCALE = dict(mean=-1.25, std=2.0)       # exact in float32 on the grid; the raw label 0.625 de-scales to 0
REAL_SCALE = dict(mean=14.41, std=29.3)


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. CRPS value and gradient --------------------------------------------------------------------------------------------
def _grid_case(s, geometry, variant, seed=0):
    """samples (S, B, out, N, od) and raw labels (B, out + 1, N, od + 1), scored channels y[:, :out, :, 1:], all on the grid"""
    b, out, n, od = geometry
    rng = np.random.default_rng(100 * s + 7 * sum(geometry) + seed)
    x = (np.round(rng.standard_normal((s,) + geometry) * 4) / 4).astype(F32)
    y = (np.round(rng.standard_normal((b, out + 1, n, od + 1)) * 4) / 4).astype(F32)
    core = y[:, :out, :, 1:]
    null_raw = F32(0.625)
    core[core == null_raw] = F32(0.5)
    null_val = 0.0
    if variant == "scattered":
        core[rng.random(core.shape) < 0.15] = null_raw
    elif variant == "horizon":
        core[rng.random(core.shape) < 0.05] = null_raw
        core[:, 1] = null_raw
    elif variant == "nan":
        core[rng.random(core.shape) < 0.15] = NAN
        null_val = NAN
    return x, y, null_val


def _call_value(xd, yd, y_start, scale, null_val, ls=None, min_s=1e-4):
    from multistgraph_amd import ops
    return ops.crps_loss_device(xd, yd, y_start, scale["mean"], scale["std"], null_val, min_s, ls)


def _call_grad(xd, yd, y_start, scale, null_val, ls=None, min_s=1e-4, upstream=1.0, into=None):
    """matgcn_crps_loss + matgcn_crps_loss_grad through the binding's one call helper and label view; ``into``: the
    tensor the gradient is written to (None: a fresh one)"""
    from multistgraph_amd import _lib, ops
    v = ops._label_view(xd, yd, ls, samples=True)
    need = C.c_size_t()
    _lib.call("matgcn_crps_loss_bytes", v.b, v.out, C.byref(need))
    scratch = torch.empty(need.value // 8, dtype=torch.float64, device=xd.device)
    result = torch.empty(1 + v.out, dtype=torch.float32, device=xd.device)
    sc = (float(scale["mean"]), float(scale["std"]), float(null_val), float(min_s))
    stream = torch.cuda.current_stream().cuda_stream
    _lib.call("matgcn_crps_loss", *v.args(y_start), *sc, scratch.data_ptr(), need.value, result.data_ptr(), stream)
    d = torch.empty_like(xd) if into is None else into
    _lib.call("matgcn_crps_loss_grad", *v.args(y_start), *sc, scratch.data_ptr(), need.value, float(upstream),
              d.data_ptr(), stream)
    return result, d


def _assert_ulp(got, want64, what):
    want = want64.astype(F32)
    assert got.dtype == F32 and got.shape == want.shape, what
    zero = want64 == 0
    assert (got[zero] == 0).all(), "%s: a gradient where the reference has none" % (what,)
    err = np.abs(got.astype(F64) - want.astype(F64))
    assert (err <= np.spacing(np.abs(want)).astype(F64)).all(), "%s: worst %.3e" % (what, err.max())


def _scores_quotient(xd, yd, y_start, scale, null_val):
    """float32(sum CRPS / count) from matgcn_mc_scores' sums: over all horizons, then per horizon (0 where the count is 0)"""
    from multistgraph_amd import ops
    sums = _host(ops.mc_scores(xd, yd, (0.05, 0.95), y_start=y_start, null_val=null_val, **scale))
    cnt, tot = sums[:, 0], sums[:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.where(cnt > 0, tot / cnt, 0.0)
    total = tot.sum() / cnt.sum() if cnt.sum() > 0 else 0.0
    return np.concatenate([[total], per]).astype(F32)


@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("s", SAMPLES)
def test_crps_on_the_grid(s, geometry, lib_built):
    b, out, n, od = geometry
    for variant in ("scattered", "horizon", "nan"):
        x, y, null_val = _grid_case(s, geometry, variant)
        core = y[:, :out, :, 1:]
        want, _, m = R.value(x, core, null_val=null_val, **GRID_SCALE)
        assert m > 0
        xd, yd = _dev(x), _dev(y)
        got = _call_value(xd, yd, 1, GRID_SCALE, null_val)
        what = (s, geometry, variant)
        assert np.array_equal(_host(got), want), (what, _host(got), want)
        if variant == "horizon":
            assert want[2] == 0.0
        assert np.array_equal(_host(got), _scores_quotient(xd, yd, 1, GRID_SCALE, null_val)), what
        result, d = _call_grad(xd, yd, 1, GRID_SCALE, null_val, upstream=4.0)
        assert torch.equal(result, got), what
        g = R.grad(x, core, null_val=null_val, upstream=4.0, **GRID_SCALE)
        _assert_ulp(_host(d), g, what)
        # run to run, and the gradient written over the samples
        result2, d2 = _call_grad(xd, yd, 1, GRID_SCALE, null_val, upstream=4.0)
        assert torch.equal(_bits(result2), _bits(result)) and torch.equal(_bits(d2), _bits(d)), what
        alias = xd.clone()
        _call_grad(alias, yd, 1, GRID_SCALE, null_val, upstream=4.0, into=alias)
        assert torch.equal(_bits(alias), _bits(d)), what


def _torch_run(p32, l32, mask, dtype):
    """the CRPS arithmetic in torch on the CPU in ``dtype`` from the float32 de-scaled values: (values (1 + out,), gradient
    w.r.t. the de-scaled samples)"""
    p = torch.tensor(p32, dtype=dtype, requires_grad=True)
    l = torch.tensor(np.nan_to_num(l32), dtype=dtype)
    mk = torch.tensor(mask)
    s = p.shape[0]
    ps, _ = p.sort(0)
    coef = (2.0 * torch.arange(s, dtype=dtype) - s + 1.0).reshape((s,) + (1,) * (p.dim() - 1))
    c = (p - l[None]).abs().mean(0) - (coef * ps).sum(0) / float(s * s)
    c = torch.where(mk, c, torch.zeros_like(c))
    total = c.sum() / mk.sum()
    per = [c[:, k].sum() / mk[:, k].sum() for k in range(p.shape[2])]
    total.backward()
    return np.array([float(total)] + [float(v) for v in per]), p.grad.numpy().astype(F64)


@pytest.mark.parametrize("s", [5, 33, 257])
def test_crps_on_continuous_data(s, lib_built):
    geometry = b, out, n, od = (3, 3, 65, 2)
    rng = np.random.default_rng(s)
    x = rng.standard_normal((s,) + geometry).astype(F32)
    y = rng.standard_normal((b, out + 1, n, od + 1)).astype(F32)
    core = y[:, :out, :, 1:]
    pick = rng.random(core.shape)
    core[pick < 0.10] = F32(-REAL_SCALE["mean"] / REAL_SCALE["std"])      # de-scales to about 0: zeroed by min_s or kept
    core[(pick >= 0.10) & (pick < 0.15)] = F32((3e-5 - REAL_SCALE["mean"]) / REAL_SCALE["std"])
    want, exact, m = R.value(x, core, null_val=0.0, **REAL_SCALE)
    g64 = R.grad(x, core, null_val=0.0, upstream=4.0, **REAL_SCALE)
    p32 = M.descale(x, **REAL_SCALE)
    l32, mask = M.labels(core, null_val=0.0, **REAL_SCALE)
    assert 0 < mask.sum() < mask.size
    v32, g32 = _torch_run(p32, l32, mask, torch.float32)
    v64, g64t = _torch_run(p32, l32, mask, torch.float64)
    assert np.abs(v64 - exact).max() <= 1e-12 * np.abs(exact).max()          # the two float64 forms agree
    std = float(F32(REAL_SCALE["std"]))
    assert max_norm_err(g64t * std * 4.0, g64) <= 1e-12
    result, d = _call_grad(_dev(x), _dev(y), 1, REAL_SCALE, 0.0, upstream=4.0)
    got = _host(result).astype(F64)
    bar = np.maximum(2.0 * np.abs(v32 - v64), FLOOR * np.abs(exact))
    err = np.abs(got - exact)
    print("S = %d: value error %.3e (bar %.3e); float32 torch gap %.3e" % (s, err[0], bar[0], abs(v32[0] - v64[0])))
    assert (err <= bar).all(), (err, bar)
    e_grad = max_norm_err(_host(d), g64)
    gap = max_norm_err(g32 * std * 4.0, g64)
    print("S = %d: gradient error %.3e max-normalised; float32 torch gap %.3e" % (s, e_grad, gap))
    assert e_grad <= max(2.0 * gap, FLOOR)
    assert (_host(d)[:, ~mask] == 0).all()


def test_crps_gradient_with_forced_ties(lib_built):
    """duplicate sample rows: the samples of a tie get the ranks their indices give them - the reference's numbers"""
    geometry = b, out, n, od = (3, 3, 65, 2)
    for s, dup in ((5, [(1, 0), (4, 2)]), (33, [(k, 0) for k in range(1, 33)]), (2, [(1, 0)])):
        x, y, null_val = _grid_case(s, geometry, "scattered", seed=9)
        for dst, src in dup:
            x[dst] = x[src]
        core = y[:, :out, :, 1:]
        result, d = _call_grad(_dev(x), _dev(y), 1, GRID_SCALE, null_val)
        _assert_ulp(_host(d), R.grad(x, core, null_val=null_val, **GRID_SCALE), ("ties", s))
        assert np.array_equal(_host(result), R.value(x, core, null_val=null_val, **GRID_SCALE)[0])
        got = _host(d)
        for dst, src in dup[:2]:      # the two members of a tie differ by the step of one rank: 2 std / (M S^2)
            assert (got[dst] != got[src]).any()


@pytest.mark.parametrize("s", [2, 33])
def test_crps_series_labels(s, lib_built):
    """labels gathered from the resident series through label_start - a start whose rows run past the series' end is
    clamped (and counted) - against the same rows as windows"""
    from multistgraph_amd import _lib
    geometry = b, out, n, od = (3, 3, 65, 2)
    rng = np.random.default_rng(s)
    steps = 40
    series = (np.round(rng.standard_normal((steps, n, od + 1)) * 4) / 4).astype(F32)
    series[rng.random(series.shape) < 0.1] = F32(0.625)
    starts = np.array([0, 17, steps - 1], dtype=np.int32)            # the last one: rows 40 and 41 are clamped to 39
    rows = np.minimum(starts[:, None] + np.arange(out)[None, :], steps - 1)
    windows = series[rows]                                           # (B, out, N, od + 1)
    x, _, _ = _grid_case(s, geometry, "scattered", seed=4)
    xd = _dev(x)
    count = C.c_int64()
    _lib.call("matgcn_series_violations", C.byref(count), 1)
    r_ser, d_ser = _call_grad(xd, _dev(series), 1, GRID_SCALE, 0.0, ls=_dev(starts))
    r_win, d_win = _call_grad(xd, _dev(windows), 1, GRID_SCALE, 0.0)
    assert torch.equal(_bits(r_ser), _bits(r_win)) and torch.equal(_bits(d_ser), _bits(d_win))
    assert np.array_equal(_host(r_win), R.value(x, windows[..., 1:], null_val=0.0, **GRID_SCALE)[0])
    _lib.call("matgcn_series_violations", C.byref(count), 1)         # read and reset: later modules expect 0
    assert count.value > 0


def test_crps_guard_words(lib_built):
    """the words in front of and behind result and d_samples stay as they were; so does everything of the samples"""
    from multistgraph_amd import _lib, ops
    geometry = b, out, n, od = (3, 3, 65, 2)
    for s in (5, 33, 257):
        x, y, null_val = _grid_case(s, geometry, "scattered", seed=2)
        xd, yd = _dev(x), _dev(y)
        keep = xd.clone()
        v = ops._label_view(xd, yd, None, samples=True)
        need = C.c_size_t()
        _lib.call("matgcn_crps_loss_bytes", v.b, v.out, C.byref(need))
        scratch = torch.empty(need.value // 8, dtype=torch.float64, device=xd.device)
        res = torch.full((GUARD + 1 + out + GUARD,), -7.5, dtype=torch.float32, device=xd.device)
        d = torch.full((GUARD + xd.numel() + GUARD,), -7.5, dtype=torch.float32, device=xd.device)
        sc = (GRID_SCALE["mean"], GRID_SCALE["std"], null_val, 1e-4)
        stream = torch.cuda.current_stream().cuda_stream
        _lib.call("matgcn_crps_loss", *v.args(1), *sc, scratch.data_ptr(), need.value, res[GUARD:].data_ptr(), stream)
        _lib.call("matgcn_crps_loss_grad", *v.args(1), *sc, scratch.data_ptr(), need.value, 1.0, d[GUARD:].data_ptr(),
                  stream)
        for t, body in ((res, 1 + out), (d, xd.numel())):
            assert (t[:GUARD] == -7.5).all() and (t[GUARD + body:] == -7.5).all(), s
            assert not (t[GUARD:GUARD + body] == -7.5).any(), s
        assert torch.equal(_bits(xd), _bits(keep))
        want = R.grad(x, y[:, :out, :, 1:], null_val=null_val, **GRID_SCALE)
        _assert_ulp(_host(d[GUARD:GUARD + xd.numel()]).reshape(x.shape), want, ("guard", s))


def test_crps_wrappers_refuse_label_geometry_before_any_call(lib_built):
    """the refusals of the binding's one label view (tests/test_binding_arguments.py holds the other wrappers to them)"""
    from multistgraph_amd import ops
    from multistgraph_amd._lib import MatgcnError
    geometry = b, out, n, od = (3, 3, 65, 1)
    x, y, _ = _grid_case(2, geometry, "scattered")
    xd, yd = _dev(x), _dev(y)
    series = _dev(np.zeros((40, n, od + 1), dtype=F32))
    starts = _dev(np.array([0, 5, 9], dtype=np.int32))
    refused = {
        "y_nodes": (xd, torch.cat([yd, yd[:, :, :1]], 2), None),
        "y_batch": (xd, yd[:2], None),
        "series_nodes": (xd, torch.cat([series, series[:, :1]], 1), starts),
        "label_start_dtype": (xd, series, starts.long()),
        "label_start_on_the_host": (xd, series, starts.cpu()),
        "label_start_shape": (xd, series, starts[:2]),
        "samples_rank": (xd[0], yd, None),
        "samples_dtype": (xd.double(), yd, None),
    }
    for fn in (ops.crps_loss_device, ops.crps_loss):
        assert torch.isfinite(fn(xd.clone(), yd, 1).detach()).all()
        assert torch.isfinite(fn(xd.clone(), series, 1, label_start=starts).detach()).all()
        for name, (s_arg, y_arg, ls) in refused.items():
            with pytest.raises(MatgcnError):
                fn(s_arg, y_arg, 1, label_start=ls)


def test_crps_autograd_writes_in_place(lib_built):
    """ops.crps_loss: the gradient of the samples IS the samples tensor afterwards, times the upstream factor"""
    from multistgraph_amd import ops
    geometry = b, out, n, od = (3, 3, 65, 1)
    x, y, null_val = _grid_case(5, geometry, "scattered", seed=6)
    xd = _dev(x).requires_grad_(True)
    loss = ops.crps_loss(xd, _dev(y), 1, GRID_SCALE["mean"], GRID_SCALE["std"], null_val)
    (loss * 4.0).backward()
    assert np.array_equal(_host(loss), R.value(x, y[:, :out, :, 1:], null_val=null_val, **GRID_SCALE)[0][0])
    assert xd.grad.data_ptr() == xd.data_ptr()
    _assert_ulp(_host(xd.grad), R.grad(x, y[:, :out, :, 1:], null_val=null_val, upstream=4.0, **GRID_SCALE), "autograd")


# ---- the bound models ------------------------------------------------------------------------------------------------------
class _Setup:
    """a synthetic model of `nodes` nodes at batch size `batch` (closed-form parameters, synthetic inputs, the host graph
    prep's static supports): the HotPath binding, the plugin class, and what the float64 oracle needs"""

    def __init__(self, nodes, batch, out=3, od=1, layers=2, cheb=2, **flags):
        from multistgraph_amd import graph_prep, synthetic as syn
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        self.n, self.b, self.out, self.od, self.layers, self.cheb, self.flags = nodes, batch, out, od, layers, cheb, flags
        self.dev = dev = torch.device("cuda:0")
        seed = 3
        self.df = dict(syn.make_data_feature(nodes, seed, "DC", ext_dim=1), output_dim=od, feature_dim=od + 1)
        self.cfg = dict(input_window=24, output_window=out, add_time_in_day=True, add_day_in_week=False,
                        load_dynamic=False, adjtype="multi", adpadj="unidirection", cheb_order=cheb, embed_dim_node=20,
                        embed_dim_adj=20, rnn_units=64, num_layers=layers, device=dev, batch_size=batch, start_dim=0,
                        end_dim=od)
        self.cfg.update(flags)
        shapes = syn.param_shapes(nodes, out_steps=out, feat_in=od + 1, out_dim=od, layers=layers,
                                  k_total=syn.k_total_for("multi", "unidirection", cheb), **flags)
        self.state_np = syn.closed_form_state(shapes, seed)
        x, y = syn.make_batch_arrays(batch, nodes, out, seed, feat=od + 1)
        if od > 1:   # channels [flow 0 .. flow od-1 | time of day]
            x = np.ascontiguousarray(np.concatenate([x[..., :1], x[..., 2:], x[..., 1:2]], -1))
        self.x_np, self.y_np = x, y
        self.x, self.y = _dev(x), _dev(y)
        self.head_steps = 1 if flags.get("fnn_off") else 24
        self.mats = np.stack(graph_prep.build_static_supports(self.df["adj_mx"], self.df["coordinate"], None, "multi"), 0)
        self.model = None
        if flags.get("rnn_units", 64) < 64:      # through the plugin class, which pads to the kernels' 64 channels
            self.model = self.make_model()
            with torch.no_grad():
                self.hp = self.model._path_for_batch(batch, dev)
                self.state = {k: v for k, v in self.model._state().items() if not k.startswith("static_initial")}
        else:
            mats = torch.from_numpy(self.mats)
            spec = spec_from_config(self.cfg, self.df, nodes, min(nodes, 20), mats.shape[0], diagonal_mask(mats))
            self.hp = HotPath(spec, batch, dev)
            self.state = {k: _dev(v) for k, v in self.state_np.items()}
            self.hp.bind(self.state, mats.to(dev))

    def make_model(self, scaler=None, **extra):
        from multistgraph_amd.model import MultiATGCN
        df = self.df if scaler is None else dict(self.df, scaler=scaler)
        m = MultiATGCN(dict(self.cfg, **extra), df).to(self.dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in self.state_np.items()})
        return m

    def series_source(self):
        from multistgraph_amd import windows as W
        rel = W.window_offsets(24)
        steps = 24 * 28 + 24 * 2 + 7
        rng = np.random.default_rng(5)
        series = rng.standard_normal((steps, self.n, self.od + 1)).astype(F32)
        starts = W.valid_label_starts(steps, rel, 24)
        pick = starts[rng.permutation(len(starts))[:self.b]].astype(np.int32)
        return series, pick, rel

    def h0(self):
        s = self.hp.spec
        g = np.random.default_rng(11).standard_normal((s.layers, self.b, s.nodes, s.hidden)).astype(F32)
        return _dev(0.1 * g)

    def d_samples(self, s):
        g = np.random.default_rng(9 + s).standard_normal((s, self.b, self.out, self.n, self.od)).astype(F32)
        return _dev(g)

    def oracle_cfg(self):
        return dict(adjtype="multi", adpadj="unidirection", cheb_order=self.cheb, num_layers=self.layers, rnn_units=64,
                    len_closeness=48, len_period=24, len_trend=24, output_window=self.out, input_window=24, start_dim=0,
                    end_dim=self.od, add_time_in_day=True, add_day_in_week=False, load_dynamic=False, **self.flags)


@pytest.fixture(scope="module")
def setup(lib_built):
    cache = {}

    def get(nodes, batch, **kw):
        key = (nodes, batch, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _Setup(nodes, batch, **kw)
        return cache[key]

    yield get
    cache.clear()
    gc.collect()
    torch.cuda.empty_cache()


CONFIGS = {
    "default": {},
    "fnn_off": {"fnn_off": True},                 # headT = 1
    "gcn_off": {"gcn_off": True},
    "out48": {"out": 24, "od": 2},                # 48 output channels: the second 32-channel tile (NTc = 2)
    "rnn16": {"rnn_units": 16},                   # padded to the kernels' 64 channels
}


# ---- 2. forward_train_mc ---------------------------------------------------------------------------------------------------
def _plain_floats(hp):
    return hp._bytes("matgcn_train_bytes") // 4


def _check_forward(p, source, s=3, offset=2 ** 32 + 5):
    hp = p.hp
    drop = (SEED, offset, P)
    hp.forward_train_mc(source, drop, s)                       # sizes the buffers
    hp._train.view(torch.uint8).fill_(0xFF)
    kept, mean, std = hp.forward_train_mc(source, drop, s, keep_stats=True)
    n = _plain_floats(hp)
    tr_mc = _bits(hp._train[:n]).clone()
    hp._train.view(torch.uint8).fill_(0xFF)
    hp.forward_train(source)
    assert torch.equal(_bits(hp._train[:n]), tr_mc)            # the saved activations of the plain training forward
    m2, s2, want = hp.forward_mc(source, seed=SEED, offset=offset, p=P, samples=s, keep_samples=True)
    assert kept.shape == want.shape == (s, p.b, p.out, p.n, p.od)
    assert torch.isfinite(kept).all() and not torch.equal(kept[0], kept[-1])
    assert torch.equal(_bits(kept), _bits(want))
    assert torch.equal(_bits(mean), _bits(m2)) and torch.equal(_bits(std), _bits(s2))
    assert torch.equal(_bits(hp.forward_train_mc(source, drop, s)), _bits(want))     # without mean / std


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_forward_train_mc_equals_forward_mc(name, setup):
    _check_forward(setup(65, 3, **CONFIGS[name]), setup(65, 3, **CONFIGS[name]).x)


def test_forward_train_mc_from_the_series(setup):
    p = setup(65, 3)
    series, pick, rel = p.series_source()
    _check_forward(p, (_dev(series), _dev(pick), rel))


def test_forward_train_mc_refuses_bad_samples(setup):
    from multistgraph_amd import _lib
    p = setup(65, 3)
    for bad in (0, 1025):
        with pytest.raises(_lib.MatgcnError) as err:
            p.hp.forward_train_mc(p.x, (SEED, 0, P), bad)
        assert "(status -2)" in str(err.value)


# ---- 3. backward_mc against the project's own explicit-mask backward ----------------------------------------------------------
def _mc_grads(p, s, offset, d, h0, source=None):
    hp = p.hp
    x = p.x if source is None else source
    hp.forward_train_mc(x, (SEED, offset, P), s, h0)
    return {k: v.clone() for k, v in hp.backward_mc(x, d.clone(), p.state, (SEED, offset, P), h0).items()}


def _sum_grads(p, s, offset, d, h0, source=None):
    """float64 sum over the samples of matgcn_forward_train / matgcn_backward with the explicit mask of offset + s"""
    hp = p.hp
    x = p.x if source is None else source
    total = None
    for k in range(s):
        mask = hp.dropout_mask(SEED, offset + k, P)
        hp.forward_train(x, mask, h0)
        g = hp.backward(x, d[k].contiguous(), p.state, mask, h0)
        g = {name: v.double().cpu() for name, v in g.items()}
        total = g if total is None else {name: total[name] + g[name] for name in g}
    return total


def _compare(got, want, what, tol=SUM_TOL):
    assert set(got) == set(want)
    worst = 0.0
    for k in want:
        w = want[k].numpy()
        if np.abs(w).max() == 0.0:
            assert float(got[k].abs().max()) == 0.0, (what, k)
            continue
        e = max_norm_err(_host(got[k]), w)
        worst = max(worst, e)
        assert e <= tol, (what, k, e)
    print("%s: worst gradient gap %.2e (bound %.0e)" % (what, worst, tol))
    return worst


BACKWARD_CASES = {
    # name: (nodes, batch, samples, setup keywords, binding settings, with h0)
    "n65_b3_s5": (65, 3, 5, {}, {}, True),
    "n48_b17_s2": (48, 17, 2, {}, {}, True),
    "n257_b3_s1": (257, 3, 1, {}, {}, False),
    "n65_b17_s2": (65, 17, 2, {}, {}, False),
    "fnn_off": (65, 3, 2, CONFIGS["fnn_off"], {}, False),
    "gcn_off": (48, 3, 2, CONFIGS["gcn_off"], {}, False),
    "out48": (65, 3, 2, CONFIGS["out48"], {}, False),
    "rnn16": (48, 3, 2, CONFIGS["rnn16"], {}, False),
    "cheb3": (65, 3, 2, {"cheb": 3}, {}, False),
    "bf16_mix": (65, 3, 1, {}, {"precision": 1}, False),
    "bf16": (65, 3, 1, {}, {"precision": 2}, False),
    "bf16x3_train": (65, 3, 2, {}, {"train_bf16x3": True}, False),
}


@pytest.mark.parametrize("name", list(BACKWARD_CASES))
def test_backward_mc_is_the_sum_over_the_samples(name, setup):
    nodes, batch, s, kw, settings, with_h0 = BACKWARD_CASES[name]
    p = setup(nodes, batch, **kw)
    hp = p.hp
    d, h0 = p.d_samples(s), (p.h0() if with_h0 else None)
    for key, value in settings.items():
        setattr(hp, key, value)
    try:
        want = _sum_grads(p, s, 7, d, h0)
        got = _mc_grads(p, s, 7, d, h0)
    finally:
        hp.precision, hp.train_bf16x3 = None, None
    assert (hp.D_H0 in got) == with_h0
    assert float(got["end_conv.weight"].abs().max()) > 0 and float(got["weight_tsg"].abs().max()) > 0
    _compare(got, want, name)


def test_backward_mc_with_one_sample_is_the_seeded_step(setup):
    p = setup(65, 3)
    hp = p.hp
    d, h0 = p.d_samples(1), p.h0()
    got = _mc_grads(p, 1, 11, d, h0)
    hp.forward_train(p.x, h0=h0, dropout=(SEED, 11, P))
    want = {k: v.double().cpu() for k, v in hp.backward(p.x, d[0].contiguous(), p.state, h0=h0, dropout=(SEED, 11, P)).items()}
    _compare(got, want, "S = 1 against matgcn_backward_seeded", tol=1e-4)


def test_backward_mc_from_the_series(setup):
    p = setup(65, 3)
    series, pick, rel = p.series_source()
    src = (_dev(series), _dev(pick), rel)
    d = p.d_samples(2)
    _compare(_mc_grads(p, 2, 3, d, None, src), _sum_grads(p, 2, 3, d, None, src), "series")


# ---- 4. against float64 ------------------------------------------------------------------------------------------------------
def _oracle_crps_grads(p, model, samples, y_np, mean, std):
    """float64: oracle.encoder -> oracle.output_head(seq * mask_s) with the masks of matgcn_dropout_mask at the offsets the
    model's first ensemble step draws (0 .. S - 1, seed torch.initial_seed()), CRPS by torch.sort, autograd"""
    from oracle import matgcn_oracle as O
    cfg = p.oracle_cfg()
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.state_np.items()}
    st64 = O.supports_as_tensors(p.mats, torch.float64)
    x0 = O.fuse_heads(torch.from_numpy(p.x_np).double(), p64, cfg)
    init = torch.zeros(p.layers, p.b, p.n, 64, dtype=torch.float64)
    seq, _ = O.encoder(x0, init, p64, st64, "multi", "unidirection", p.cheb, p.layers, False, False)
    hp = model._path_for_batch(p.b, p.dev)
    outs = []
    for s in range(samples):
        mask = hp.dropout_mask(torch.initial_seed(), s, P).double().cpu()
        outs.append(O.output_head(seq * mask, p64, p.out, p.od))
    pr = torch.stack(outs, 0) * std + mean
    l = torch.from_numpy(y_np[..., :p.od]).double() * std + mean
    l = torch.where(l.abs() < 1e-4, torch.zeros_like(l), l)
    keep = l != 0
    ps, _ = pr.sort(0)
    coef = (2.0 * torch.arange(samples, dtype=torch.float64) - samples + 1.0).reshape(samples, 1, 1, 1, 1)
    c = (pr - l[None]).abs().mean(0) - (coef * ps).sum(0) / float(samples * samples)
    loss = torch.where(keep, c, torch.zeros_like(c)).sum() / keep.sum()
    loss.backward()
    return float(loss), {k: v.grad for k, v in p64.items()}


@pytest.mark.parametrize("nodes,layers", [(65, 2), (48, 4)])
def test_calculate_loss_crps_against_float64(nodes, layers, setup):
    from multistgraph_amd import synthetic as syn
    p = setup(nodes, 3, layers=layers)
    samples = 5
    scaler = syn.PlainScaler(REAL_SCALE["mean"], REAL_SCALE["std"])
    m = p.make_model(scaler=scaler, hip_train_loss="crps", hip_dropout="device", hip_train_samples=samples).train()
    y = p.y_np.copy()
    y[0, :, :3, 0] = F32(-REAL_SCALE["mean"] / REAL_SCALE["std"])      # de-scales to about 0: zeroed, then masked
    loss = m.calculate_loss({"X": p.x, "y": _dev(y)})
    loss.backward()
    want, grads = _oracle_crps_grads(p, m, samples, y, REAL_SCALE["mean"], REAL_SCALE["std"])
    print("N = %d, %d layers: CRPS %.6f (float64 %.6f)" % (nodes, layers, float(loss), want))
    assert abs(float(loss) - want) <= ORACLE_TOL * abs(want)
    worst = 0.0
    for k, prm in m.named_parameters():
        w = grads[k]
        if w is None or float(w.abs().max()) == 0.0:
            continue
        e = max_norm_err(_host(prm.grad), w.numpy())
        worst = max(worst, e)
        assert e <= ORACLE_TOL, (k, e)
    print("N = %d, %d layers: worst gradient error against float64 %.2e (bound %.0e)" % (nodes, layers, worst, ORACLE_TOL))


# ---- 5. identities -------------------------------------------------------------------------------------------------------------
def _composed(p, s, drop, y, scale, h0=None):
    """(loss, gradients) of forward_train_mc -> ops.crps_loss -> backward_mc"""
    from multistgraph_amd import ops
    kept = p.hp.forward_train_mc(p.x, drop, s, h0).requires_grad_(True)
    loss = ops.crps_loss(kept, y, 0, scale["mean"], scale["std"], 0.0)
    loss.backward()
    return loss.detach(), {k: v.clone() for k, v in p.hp.backward_mc(p.x, kept.grad, p.state, drop, h0).items()}


def test_without_dropout_the_ensemble_is_the_mae_step(setup):
    """p = 0: all samples tie; the CRPS is the masked MAE of the one forecast and the gradients those of the S = 1 run"""
    from multistgraph_amd import ops
    p = setup(65, 3)
    drop = (SEED, 0, 0.0)
    kept = p.hp.forward_train_mc(p.x, drop, 4)
    assert all(torch.equal(_bits(kept[k]), _bits(kept[0])) for k in range(1, 4))
    mae = ops.train_loss_device(kept[0].contiguous(), p.y, 0, REAL_SCALE["mean"], REAL_SCALE["std"], "masked_mae")[0]
    p.hp.deterministic = True      # a fixed order behind the head: the figure below is the same every run
    try:
        loss4, g4 = _composed(p, 4, drop, p.y, REAL_SCALE)
        loss1, g1 = _composed(p, 1, drop, p.y, REAL_SCALE)
    finally:
        p.hp.deterministic = None
    for loss in (loss4, loss1):
        assert abs(float(loss) - float(mae)) <= float(np.spacing(F32(abs(float(mae))))), (float(loss), float(mae))
    worst = 0.0
    for k in g1:
        if float(g1[k].abs().max()) == 0.0:
            continue
        e = max_norm_err(_host(g4[k]), _host(g1[k]))
        worst = max(worst, e)
        assert e <= 1e-6, (k, e)
    print("p = 0, S = 4 against S = 1: worst gradient gap %.2e (bound 1e-06)" % worst)


def test_another_offset_changes_the_gradients(setup):
    p = setup(65, 3)
    d = p.d_samples(2)
    a = _mc_grads(p, 2, 5, d, None)
    p.hp.forward_train_mc(p.x, (SEED, 5, P), 2)
    b = p.hp.backward_mc(p.x, d.clone(), p.state, (SEED, 6, P))
    assert any(not torch.equal(a[k], b[k]) for k in a)


def test_a_backward_after_a_second_forward_is_refused(setup):
    p = setup(65, 3)
    m = p.make_model(hip_train_loss="crps", hip_dropout="device", hip_train_samples=2).train()
    batch = {"X": p.x, "y": p.y}
    first = m.calculate_loss(batch)
    second = m.calculate_loss(batch)
    with pytest.raises(RuntimeError, match="another forward"):
        first.backward()
    second.backward()
    assert m.end_conv.weight.grad is not None and m._dropout_counter == 4


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------
def test_deterministic_backward_mc(setup):
    p = setup(65, 17)
    hp = p.hp
    d, h0 = p.d_samples(5), p.h0()
    hp.deterministic = True
    try:
        a = _mc_grads(p, 5, 2, d, h0)
        b = _mc_grads(p, 5, 2, d, h0)
    finally:
        hp.deterministic = None
    assert float(a["node_emb"].abs().max()) > 0
    diff = [k for k in a if not torch.equal(_bits(a[k]), _bits(b[k]))]
    assert not diff, diff


def test_head_gradients_have_the_same_bits_in_the_default_mode(setup):
    """the head stage adds in a fixed order in both settings: its own three outputs do not move from run to run"""
    p = setup(65, 17)
    d = p.d_samples(5)
    a, b = _mc_grads(p, 5, 2, d, None), _mc_grads(p, 5, 2, d, None)
    for k in ("end_conv.weight", "end_conv.bias"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


# ---- 7. the model ----------------------------------------------------------------------------------------------------------------
def _model_step(m, batch):
    m.zero_grad(set_to_none=True)
    m._dropout_counter = 0
    loss = m.calculate_loss(batch)
    loss.backward()
    return loss.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def test_calculate_loss_crps_is_the_composition_of_the_three_calls(setup):
    from multistgraph_amd import synthetic as syn
    p = setup(65, 3)
    s = 5
    m = p.make_model(scaler=syn.PlainScaler(REAL_SCALE["mean"], REAL_SCALE["std"]), hip_train_loss="crps",
                     hip_dropout="device", hip_train_samples=s, hip_deterministic=True).train()
    loss, grads = _model_step(m, {"X": p.x, "y": p.y})
    hp = m._path_for_batch(p.b, p.dev)
    q = _Setup.__new__(_Setup)
    q.hp, q.x, q.state = hp, p.x, {k: v.detach() for k, v in m.named_parameters()}
    hp.deterministic = True
    want_loss, want = _composed(q, s, (torch.initial_seed(), 0, P), p.y, REAL_SCALE)
    assert torch.equal(_bits(loss), _bits(want_loss))
    for k, g in grads.items():
        assert torch.equal(_bits(g), _bits(want[k])), k
    # on demand, and without autograd: the same ensemble through the inference forward
    m._dropout_counter = 0
    with torch.no_grad():
        again = m.train_loss({"X": p.x, "y": p.y}, "crps", samples=s)
    assert torch.equal(_bits(again), _bits(loss)) and m._dropout_counter == s


def test_window_and_resident_batches_give_the_same_bits(setup):
    from multistgraph_amd import windows as W
    p = setup(65, 3)
    series, pick, rel = p.series_source()
    x, y = W.gather_windows(series, pick, rel, p.out)
    m = p.make_model(hip_train_loss="crps", hip_dropout="device", hip_train_samples=3, hip_deterministic=True).train()
    l_win, g_win = _model_step(m, {"X": _dev(x), "y": _dev(y)})
    l_ser, g_ser = _model_step(m, {"series": _dev(series), "label_start": _dev(pick), "rel_steps": rel})
    assert torch.isfinite(l_win) and float(l_win) > 0
    assert torch.equal(_bits(l_win), _bits(l_ser))
    assert set(g_win) == set(g_ser) and all(torch.equal(_bits(g_win[k]), _bits(g_ser[k])) for k in g_win)


def test_twenty_steps_lower_the_crps(setup):
    from multistgraph_amd.optim import ClipAdam
    p = setup(48, 8, out=6)
    m = p.make_model(hip_train_loss="crps", hip_dropout="device", hip_train_samples=8).train()
    batch = {"X": p.x, "y": p.y}

    def crps():
        m._dropout_counter = 1 << 20         # the same masks before and after, none of them a training step's
        with torch.no_grad():
            return float(m.train_loss(batch, "crps", samples=8))

    before = crps()
    m._dropout_counter = 0
    opt = ClipAdam(m.parameters(), lr=1e-3, max_grad_norm=5.0)
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        m.calculate_loss(batch).backward()
        opt.step()
    assert m._dropout_counter == 20 * 8
    after = crps()
    print("CRPS on the training batch: %.6f -> %.6f after 20 steps" % (before, after))
    assert after < before


def test_the_default_training_step_is_unchanged(setup):
    p = setup(65, 3)
    batch = {"X": p.x, "y": p.y}
    base = p.make_model(hip_dropout="device", hip_deterministic=True).train()
    keyed = p.make_model(hip_dropout="device", hip_deterministic=True, hip_train_samples=8, hip_train_loss="none").train()
    l0, g0 = _model_step(base, batch)
    l1, g1 = _model_step(keyed, batch)
    assert torch.equal(_bits(l0), _bits(l1))
    assert set(g0) == set(g1) and all(torch.equal(_bits(g0[k]), _bits(g1[k])) for k in g0)


# ---- every new entry point keeps the order of the caller's stream -----------------------------------------------------------------
def test_the_ensemble_step_behind_a_gate_on_a_side_stream(setup):
    """tests/stream_gate.py's sandwich around forward_train_mc -> crps_loss (value and gradient) -> backward_mc on a side
    stream, inputs written behind the gate: the bits of the synchronised null-stream run"""
    from multistgraph_amd import ops
    p = setup(65, 3)
    hp = p.hp
    hp.deterministic = True
    x_stage, y_stage = p.x.clone(), p.y.clone()
    x, y = torch.empty_like(p.x), torch.empty_like(p.y)
    drop = (SEED, 9, P)

    def call():
        kept = hp.forward_train_mc(x, drop, 3).requires_grad_(True)
        loss = ops.crps_loss(kept, y, 0, REAL_SCALE["mean"], REAL_SCALE["std"], 0.0)
        loss.backward()
        return loss.detach(), hp.backward_mc(x, kept.grad, p.state, drop)

    def outputs(res):
        return dict(res[1], loss=res[0].reshape(1))

    bufs = lambda *_: [hp.workspace, hp._train]      # noqa: E731
    try:
        hp.forward_train_mc(p.x, drop, 3)            # sizes the buffers
        args = ([(x, x_stage), (y, y_stage)], call, outputs, bufs)
        want = sandwich(None, *args, poison_before=bufs, synchronous=True)
        got = sandwich(torch.cuda.Stream(), *args, poison_before=bufs)
    finally:
        hp.deterministic = None
    assert set(got) == set(want) and torch.isfinite(want["loss"]).all()
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, bad
