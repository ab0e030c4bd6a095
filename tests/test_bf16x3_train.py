"""Three-piece training: matgcn_set_train_bf16x3 (include/matgcn.h), HotPath.train_bf16x3, hip_precision "bf16x3_train".

With the switch on (and matgcn_set_train_precision at 0) matgcn_forward_train runs the inference forward's three-piece
graph mixes and matgcn_backward its transposed mixes on k_mix_bf16x3<2>: both operands split into three bf16 pieces, the
six leading products accumulated in fp32.  The claim is "as accurate as the fp32 path", so every tolerance here is the
fp32 path's own and none is derived from what the kernel gives: 1e-4 max-normalised per gradient tensor, 2e-4 on the
sums of the subsampled ones, 1e-4 max-normalised and element-wise for the prediction (test_shape_edges.py,
test_backward_gpu.py).  Everything else is torch.equal.

The seven gradient edges between them: odd and even column-tile counts (b3, b17, b33, b65 against b16), an odd number
of 16-index groups per support slot (n48: 3, n65: 5 - the last K-tile of a slot must not run into the next slot), no
padding row (n64), a ragged row tile (n48), partial sums with a last group of one K-tile (n1039_b3).

Every accuracy test prints its measured distance next to the fp32 step's and the oracle's own fp32-vs-float64 gap.  On an
MI355X (one run; the non-deterministic fp32 atomics move the last digit), worst gradient tensor against the float64
autograd, three-piece step | fp32 step | the oracle's own fp32 run: edge_n1039_b3 1.4e-6 | 1.7e-6 | 1.8e-6, edge_n256_b33
2.1e-6 | 1.4e-6 | 9.0e-7, edge_n257_b33 2.3e-6 | 3.1e-6 | 2.8e-6, edge_n257_b65 1.7e-6 | 1.2e-6 | 1.3e-6, edge_n48_b3
9.4e-7 | 2.0e-6 | 1.4e-6, edge_n64_b17 9.0e-7 | 1.8e-6 | 8.4e-7, edge_n65_b16 1.3e-6 | 1.1e-6 | 1.2e-6; prediction 4.1e-7 ..
7.2e-7 (the fp32 step 4.0e-7 .. 6.8e-7).  Three-piece against fp32 transposed mixes on one forward's activations
(edge_n257_b65, deterministic): 1.4e-6 on the worst tensor.

CONFIG_EDGES: three stacks of other configurations past one tile, whose planes (Ks * nKg * NpC) scale with the stack
(test_shape_edges.py has their table) - edge_c3_n65_b5 1.5e-6 | 1.4e-6 | 1.4e-6, edge_c1_n65_b17_l3 8.6e-7 | 9.5e-7 | 6.2e-7,
edge_oduni_n65_b3 5.5e-7 | 9.3e-7 | 7.8e-7.  The bf16 training modes 1 and 2 stay out of these cases: their 5e-3 / 2.7e-2
bounds were measured on cheb_order 2 stacks only, and nothing tells what a squared support costs them.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import EDGE_SHAPE_GRAD, GOLDEN_DIR, Case, EdgeCase, elementwise_excess, max_norm_err
from test_backward_gpu import _backward_vs_fixture
from test_shape_edges import _fixture_keys, _grad_errors
from test_train_precision import D_H0, _fixture_mask, _path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

E2E_TOL = 1e-4
GRAD_TOL = 1e-4
# the seven gradient edges of the default configuration, and the stacks of other configurations, whose planes scale with
# them (test_bf16x3.py: CONFIG_EDGES).  The bf16 training modes 1 and 2 stay out of the latter: their bounds were measured
# on cheb_order 2 stacks only, and nothing tells what a squared support costs them
SHAPE_EDGES = EDGE_SHAPE_GRAD
CONFIG_EDGES = ["edge_c3_n65_b5", "edge_c1_n65_b17_l3", "edge_oduni_n65_b3"]


def _load():
    from multistgraph_amd import _lib
    return _lib.load()


# ---- host side (these fail where the symbol does not exist) ------------------------------------------------------------
def test_setter(lib_built):
    """starts at 0, returns the previous value, any non-zero value is on; both precision setters are untouched and
    matgcn_set_train_precision(3) still means 0"""
    lib = _load()
    assert lib.matgcn_set_train_bf16x3(0) == 0
    try:
        assert lib.matgcn_set_train_bf16x3(1) == 0
        assert lib.matgcn_set_train_bf16x3(7) == 1
        assert lib.matgcn_set_train_bf16x3(-3) == 1        # 7 meant on
        assert lib.matgcn_set_mix_precision(0) == 0        # the precision settings are untouched
        assert lib.matgcn_set_train_precision(3) == 0
        assert lib.matgcn_set_train_precision(0) == 0      # 3 meant 0, switch or no switch
        assert lib.matgcn_set_train_bf16x3(0) == 1         # and -3 meant on
        assert lib.matgcn_set_train_bf16x3(0) == 0
    finally:
        lib.matgcn_set_train_bf16x3(0)
        lib.matgcn_set_train_precision(0)


def test_header_binding_and_library_agree(lib_built):
    from multistgraph_amd import _lib
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    assert "int matgcn_set_train_bf16x3(int enabled);" in header
    assert "#define MATGCN_ABI_VERSION 12" in header
    assert "matgcn_set_train_bf16x3" in _lib.EXPORTED_SYMBOLS
    assert set(re.findall(r"\b(matgcn_[a-z_0-9]+)\s*\(", header)) == set(_lib.EXPORTED_SYMBOLS)
    lib = _lib.load()
    assert hasattr(lib, "matgcn_set_train_bf16x3") and lib.matgcn_abi_version() == _lib.ABI_VERSION == 12


def test_both_buffers_count_the_planes_while_the_mode_is_effective(lib_built):
    from multistgraph_amd.ops import diagonal_mask, spec_from_config
    lib = _load()
    c = Case("tiny_multi_uni_c2")
    st = torch.from_numpy(c.gold["static_supports"])
    dims = spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), st.shape[0], diagonal_mask(st)).dims(c.b)
    ws, tr = C.c_size_t(), C.c_size_t()

    def sizes():
        assert lib.matgcn_workspace_bytes(C.byref(dims), C.byref(ws)) == 0
        assert lib.matgcn_train_bytes(C.byref(dims), C.byref(tr)) == 0
        return ws.value, tr.value

    assert lib.matgcn_set_train_bf16x3(0) == 0 and lib.matgcn_set_train_precision(0) == 0
    try:
        ws0, tr0 = sizes()
        lib.matgcn_set_train_bf16x3(1)
        ws1, tr1 = sizes()
        assert ws1 > ws0 and tr1 > tr0
        # three bf16 planes, 6 bytes per element, each total rounded up to 256 bytes.  Workspace: the forward's stack
        # [Np rounded up to 32][Ks * Np rounded up to 64] (test_bf16x3.py).  Train buffer: the plain stack slot by slot,
        # [Ks][Np rounded up to 32][N rounded up to 64]
        lay = (C.c_int64 * 4)()
        assert lib.matgcn_supports_layout(C.byref(dims), C.byref(lay)) == 0
        ld, np_, ks = int(lay[1]), int(lay[2]), int(lay[3])
        assert ks >= 2
        np32, npc = (np_ + 31) // 32 * 32, (c.n + 63) // 64 * 64
        assert ws1 - ws0 == (6 * np32 * ld + 255) // 256 * 256
        assert tr1 - tr0 == (6 * ks * np32 * npc + 255) // 256 * 256
        lib.matgcn_set_deterministic(1)                    # the slabs sit behind the planes: the same increment
        _, tr1d = sizes()
        lib.matgcn_set_train_bf16x3(0)
        _, tr0d = sizes()
        assert tr1d - tr0d == tr1 - tr0
        lib.matgcn_set_deterministic(0)
        lib.matgcn_set_train_bf16x3(1)
        lib.matgcn_set_train_precision(1)                  # an explicit bf16 mode wins: the switch is ignored
        assert sizes() == (ws0, tr0)
        lib.matgcn_set_train_precision(0)
        assert sizes() == (ws1, tr1)
        lib.matgcn_set_train_bf16x3(0)
        assert sizes() == (ws0, tr0)
    finally:
        lib.matgcn_set_train_bf16x3(0)
        lib.matgcn_set_train_precision(0)
        lib.matgcn_set_deterministic(0)


def test_hip_precision_bf16x3_train_is_a_config_value():
    from multistgraph_amd.model import HIP_PRECISIONS, MultiATGCN
    c = Case("tiny_multi_uni_c2")
    assert HIP_PRECISIONS["bf16x3_train"] == 3             # inference mode 3, as "bf16x3"
    torch.manual_seed(0)
    ref = MultiATGCN(c.config(), c.data_feature)
    torch.manual_seed(0)
    m = MultiATGCN(dict(c.config(), hip_precision="bf16x3_train"), c.data_feature)
    assert m.hip_precision == "bf16x3_train" and ref.hip_precision == "fp32"
    sd, rd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(sd[k].shape == rd[k].shape and torch.equal(sd[k], rd[k]) for k in sd)
    for bad in ("bf16x3-train", "bf16x3_train ", "bf16x3_training", "BF16X3_TRAIN", "bf16x3train", "train_bf16x3"):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_precision=bad), c.data_feature)


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _clone(grads):
    return {k: v.clone() for k, v in grads.items()}


def _same_bits(a, b):
    assert set(a) == set(b)
    return all(torch.equal(a[k], b[k]) for k in a)


class _Bound:
    """an edge case bound to the HIP path; step(): one training step with the binding's switches set as given"""

    def __init__(self, name):
        from multistgraph_amd.ops import HotPath
        c = self.c = EdgeCase(name)
        self.dev = torch.device("cuda:0")
        spec, st = c.spec_and_static()
        self.hp = HotPath(spec, c.b, self.dev)
        self.state = {k: torch.from_numpy(v).to(self.dev) for k, v in c.state.items()}
        self.hp.bind(self.state, None if st is None else st.to(self.dev))
        self.x = torch.from_numpy(c.x).to(self.dev)
        self.d_out = torch.from_numpy(c.d_out()).to(self.dev)

    def forward_train(self, x3, det=None, precision=None, h0=None):
        hp = self.hp
        hp.train_bf16x3, hp.deterministic, hp.precision = x3, det, precision
        return hp.forward_train(self.x, None, h0).clone()

    def backward(self, x3, det=None, h0=None):
        hp = self.hp
        hp.train_bf16x3, hp.deterministic = x3, det
        g = _clone(hp.backward(self.x, self.d_out, self.state, None, h0))
        torch.cuda.synchronize()
        return g

    def step(self, x3, det=None, precision=None, h0=None):
        y = self.forward_train(x3, det, precision, h0)
        return y, self.backward(x3, det, h0)

    def zeros(self):
        s = self.hp.spec
        return torch.zeros(s.layers, self.hp.batch, s.nodes, s.hidden, dtype=torch.float32, device=self.dev)


@pytest.fixture(scope="module")
def bound(lib_built):
    cache = {}

    def get(name):
        if name not in cache:
            cache.clear()                                        # one shape's buffers at a time
            torch.cuda.empty_cache()
            cache[name] = _Bound(name)
        return cache[name]

    yield get
    cache.clear()
    torch.cuda.empty_cache()
    lib = _load()
    assert lib.matgcn_set_train_bf16x3(0) == 0 and lib.matgcn_set_deterministic(0) == 0   # every call restored them
    assert lib.matgcn_set_train_precision(0) == 0 and lib.matgcn_set_mix_precision(0) == 0


# ---- 1. gradient accuracy at every edge --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", SHAPE_EDGES + CONFIG_EDGES)
def test_three_piece_step_matches_the_float64_autograd(name, bound):
    p = bound(name)
    gold = p.c.grad_gold
    y32, g32 = p.step(False)
    y3, g3 = p.step(True)
    assert set(g3) == _fixture_keys(gold)
    got, want = y3.cpu().numpy(), p.c.gold["pred64"]
    assert got.shape == want.shape and np.isfinite(got).all()
    perr, excess = max_norm_err(got, want), elementwise_excess(got, want)
    errs, bad = _grad_errors(gold, g3)
    errs32, _ = _grad_errors(gold, g32)
    worst, worst32 = max(errs, key=errs.get), max(errs32, key=errs32.get)
    print("%s: three-piece step vs fp64: prediction %.3e (element-wise excess %.3f; fp32 step %.3e), worst gradient %.3e "
          "(%s); fp32 step %.3e (%s); oracle fp32 vs fp64 %.3e" % (
              name, perr, excess, max_norm_err(y32.cpu().numpy(), want), errs[worst], worst, errs32[worst32], worst32,
              float(gold["gap32_grad"])))
    assert perr <= E2E_TOL, perr
    assert excess <= 1.0, excess
    bad.update({k: e for k, e in errs.items() if e > GRAD_TOL})
    assert not bad, bad
    p.hp._train = None


# ---- 2. real size ------------------------------------------------------------------------------------------------------
@gpu
def test_three_piece_step_matches_reference_autograd_at_real_size(lib_built):
    """Baltimore 403 (B = 4): the reference's own calculate_loss().backward(), prediction and every gradient at 1e-4 - the
    check test_backward_gpu.py::test_backward_matches_reference_autograd holds the fp32 path to"""
    c = Case("bm403_out24")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_bm403_out24.npz"))
    hp, dev, state = _path(c)
    hp.train_bf16x3 = True
    _backward_vs_fixture(c, gold, hp, dev, state)
    assert hp.lib.matgcn_set_train_bf16x3(0) == 0                # restored around every call


# ---- 3. the variant really ran, in both directions ---------------------------------------------------------------------
def _backward_on_copy(p, x3):
    """the saved activations (and planes) of the last forward_train back-propagated with the switch at `x3`, as
    test_train_precision.py::_backward_on_copy does it for the bf16 modes: a second train buffer is recorded for that mode
    by a forward_train of its own and then gets the first buffer's contents, the workspace what the first forward left"""
    hp = p.hp
    tr, ws = hp._train, hp.workspace
    tr_saved, ws_saved = tr.clone(), ws.clone()
    try:
        hp._train = torch.empty_like(tr)
        p.forward_train(x3, True)                                # records the mode of `x3` for the new buffer
        hp._train[:tr_saved.numel()].copy_(tr_saved)
        hp.workspace[:ws_saved.numel()].copy_(ws_saved)
        return p.backward(x3, True)
    finally:
        hp._train, hp.workspace = tr, ws
        hp.workspace.copy_(ws_saved)


@gpu
def test_the_three_piece_kernels_run_in_both_directions(bound):
    _both_directions(bound("edge_n257_b65"), "edge_n257_b65")


@gpu
@pytest.mark.parametrize("name", CONFIG_EDGES)
def test_the_three_piece_kernels_run_in_both_directions_at_the_configuration_edges(name, bound):
    """the accuracy test above would also pass if a stack of another configuration (Ks 6 on the unfused chain pair, the
    summed slot, the adaptive support alone) quietly took the fp32 mixes: deterministic, on one forward's activations,
    the gradients with the switch on differ from the ones with it off, and the forwards differ"""
    _both_directions(bound(name), name)


def _both_directions(p, name):
    y32 = p.forward_train(False, True)
    y3 = p.forward_train(True, True)
    assert not torch.equal(y3, y32)                              # the forward's three-piece mixes ran
    on = _backward_on_copy(p, True)
    off = _backward_on_copy(p, False)                            # the same activations, the fp32 transposed mixes
    assert not _same_bits(on, off)                               # the backward's three-piece mixes ran
    gaps = {k: float((on[k] - off[k]).abs().max()) / max(float(off[k].abs().max()), 1e-30) for k in on}
    print("%s: three-piece against fp32 transposed mixes on one forward's activations, worst tensor %.3e" %
          (name, max(gaps.values())))
    assert all(torch.isfinite(v).all() for v in on.values())
    bad = {k: e for k, e in gaps.items() if e > GRAD_TOL}
    assert not bad, bad
    p.hp._train = None


# ---- 4. the backward follows its forward_train -------------------------------------------------------------------------
@gpu
def test_backward_follows_the_mode_of_its_forward_train(bound):
    p = bound("edge_n257_b65")
    _, want3 = p.step(True, True)
    p.forward_train(True, True)
    assert _same_bits(p.backward(False, True), want3)            # switched off in between: still the three-piece backward
    _, want32 = p.step(False, True)
    assert not _same_bits(want32, want3)
    p.forward_train(False, True)
    assert _same_bits(p.backward(True, True), want32)            # switched on in between: still the fp32 backward
    p.hp._train = None


# ---- 5. small buffers --------------------------------------------------------------------------------------------------
@gpu
def test_buffers_sized_without_the_planes_are_refused_and_the_binding_resizes(lib_built):
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    hp, dev, state = _path(c)
    lib = hp.lib
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    y32 = hp.forward_train(x, mask).clone()                      # switch off: both buffers at their default size
    ws0, tr0 = hp.workspace.numel() * 4, hp._train.numel() * 4
    out = torch.empty_like(y32)

    def call(ws, tr):
        return lib.matgcn_forward_train(C.byref(hp.dims), C.byref(hp.params), C.c_void_p(hp.prepared.data_ptr()),
                                        C.c_void_p(x.data_ptr()), None, None, C.c_void_p(mask.data_ptr()),
                                        C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), C.c_size_t(ws.numel() * 4),
                                        C.c_void_p(tr.data_ptr()), C.c_size_t(tr.numel() * 4), hp._stream())

    assert lib.matgcn_set_train_bf16x3(1) == 0
    try:
        n = C.c_size_t()
        assert lib.matgcn_workspace_bytes(C.byref(hp.dims), C.byref(n)) == 0
        ws1 = n.value
        assert lib.matgcn_train_bytes(C.byref(hp.dims), C.byref(n)) == 0
        tr1 = n.value
        assert ws1 > ws0 and tr1 > tr0
        big_ws = torch.empty(ws1 // 4, dtype=torch.float32, device=dev)
        big_tr = torch.empty(tr1 // 4, dtype=torch.float32, device=dev)
        assert call(hp.workspace, big_tr) == -4                  # MATGCN_ERR_SMALL_BUFFER: the workspace
        assert call(big_ws, hp._train) == -4                     # the train buffer
        assert call(big_ws, big_tr) == 0
        torch.cuda.synchronize()
        y3 = out.clone()
    finally:
        lib.matgcn_set_train_bf16x3(0)
    assert not torch.equal(y3, y32)
    hp.train_bf16x3 = True
    assert torch.equal(hp.forward_train(x, mask), y3)            # the binding re-sizes both and repeats
    assert hp.workspace.numel() * 4 == ws1 and hp._train.numel() * 4 == tr1
    grads = hp.backward(x, torch.from_numpy(gold["d_out"]).to(dev), state, mask)
    assert all(torch.isfinite(v).all() for v in grads.values())
    assert lib.matgcn_set_train_bf16x3(0) == 0


# ---- 6. bit-reproducible when asked ------------------------------------------------------------------------------------
@gpu
def test_deterministic_three_piece_steps_have_equal_bits_in_both_schedules(bound):
    p = bound("edge_n65_b16")
    lib = p.hp.lib
    h0 = p.zeros()
    runs = []
    prev = lib.matgcn_set_wavefront(1)
    try:
        for schedule in (1, 0):
            lib.matgcn_set_wavefront(schedule)
            for _ in range(2):
                y, g = p.step(True, True, h0=h0)
                assert D_H0 in g
                runs.append(dict(g, __y__=y))
    finally:
        lib.matgcn_set_wavefront(prev)
    for other in runs[1:]:
        assert _same_bits(runs[0], other)
    y32, g32 = p.step(False, True, h0=h0)
    assert not _same_bits(dict(g32, __y__=y32), runs[0])         # and they are the three-piece step's bits
    p.hp._train = None


# ---- 7. nothing else moved ---------------------------------------------------------------------------------------------
@gpu
def test_the_other_modes_keep_their_bits_around_a_three_piece_step(bound):
    p = bound("edge_n64_b17")
    before = {mode: p.step(False, True, precision=mode) for mode in (None, 1, 2)}
    y3, g3 = p.step(True, True)
    assert not torch.equal(y3, before[None][0])
    for mode in (None, 1, 2):
        y, g = p.step(False, True, precision=mode)
        assert torch.equal(y, before[mode][0]) and _same_bits(g, before[mode][1]), mode
    for mode in (1, 2):                                          # an explicit bf16 mode wins over the switch
        y, g = p.step(True, True, precision=mode)
        assert torch.equal(y, before[mode][0]) and _same_bits(g, before[mode][1]), mode
        assert not torch.equal(y, y3)
    y, g = p.step(True, True)
    assert torch.equal(y, y3) and _same_bits(g, g3)
    p.hp._train = None


# ---- 8. plugin ---------------------------------------------------------------------------------------------------------
def _plugin_step(c, precision, mask, dev):
    """calculate_loss(batch).backward() of a deterministic model with hip_precision = `precision`; returns the model, its
    gradients and the d_out its backward was handed"""
    from multistgraph_amd.model import MultiATGCN
    model = MultiATGCN(dict(c.config("cuda:0"), hip_precision=precision, hip_deterministic=True), c.data_feature).to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    model.train()
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}
    hp = model._path_for(batch["X"])
    seen, inner = {}, hp.backward

    def spy(x, d_out, *args, **kw):
        seen["d_out"] = d_out.clone()
        return inner(x, d_out, *args, **kw)

    hp.backward = spy
    try:
        model.calculate_loss(batch).backward()
    finally:
        del hp.backward
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return model, hp, grads, seen["d_out"]


@gpu
def test_plugin_trains_with_three_pieces(lib_built, monkeypatch):
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    dev = torch.device("cuda:0")
    lib = _load()
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda inp, p=0.5, training=True, inplace=False: inp * mask)
    got = {}
    for precision in ("bf16x3_train", "bf16x3", "fp32"):
        got[precision] = _plugin_step(c, precision, mask, dev)
        assert lib.matgcn_set_train_bf16x3(0) == 0 and lib.matgcn_set_deterministic(0) == 0   # left as found
        assert lib.matgcn_set_train_precision(0) == 0 and lib.matgcn_set_mix_precision(0) == 0
    model, hp, grads, d_out = got["bf16x3_train"]
    # the same step through the binding, the switch and the deterministic setting set by hand
    x = torch.from_numpy(c.x).to(dev)
    state = {k: p for k, p in model.named_parameters()}
    hp.precision, hp.train_bf16x3, hp.deterministic = None, True, True
    hp.forward_train(x, mask)
    want = {k: v for k, v in hp.backward(x, d_out, state, mask).items() if k != D_H0}
    assert set(grads) == set(want) and all(torch.equal(grads[k], want[k]) for k in want)
    hp.train_bf16x3 = False
    hp.forward_train(x, mask)
    plain = hp.backward(x, d_out, state, mask)
    assert any(not torch.equal(grads[k], plain[k]) for k in grads)   # and not the fp32 step's
    # "bf16x3" keeps its meaning: inference mode 3, training steps in fp32
    g3, g32 = got["bf16x3"][2], got["fp32"][2]
    assert set(g3) == set(g32) and all(torch.equal(g3[k], g32[k]) for k in g32)
    assert torch.equal(got["bf16x3"][3], got["fp32"][3])
