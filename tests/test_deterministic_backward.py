"""Deterministic backward: matgcn_set_deterministic (include/matgcn.h), HotPath.deterministic, config['hip_deterministic'].

With the setting on, every sum of matgcn_backward that several workgroups form together is added in a fixed order
(partial slabs + one ordered reduction, or one contributor per address): the gradients of two runs on the same saved
activations are bit-identical, in both schedules (matgcn_set_wavefront 0 / 1) and in every training precision mode.  The
default keeps its fp32 atomics.  Tolerances: the fixtures' own 1e-4 (test_backward_matches_reference_autograd) and
ATOMIC_TOL of test_train_precision.py; everything else is torch.equal.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, Case
from test_train_precision import ATOMIC_TOL, D_H0, _errors, _fixture_mask, _path, _same_up_to_atomics, _step

GRAD_TOL = 1e-4
CASES = ["tiny_multi_uni_c2", "tiny_multi_bid_c2", "tiny_multi_uni_dyn7", "tiny_multi_uni_c2_static", "dc237_out12"]
EDGES = ["edge_n257_b33", "edge_n64_b17", "edge_n1039_b3"]
# stacks the ordered reductions scale with (test_shape_edges.py has the table): Ks 6 on the unfused chain pair - its blend
# shares come from (B * Np + 63) / 64 workgroups, its pool gradients entry by entry -, Ks 0 (no mix, no adjacency
# gradient), 14 input channels (the widest narrow residual weight gradient)
CONFIG_EDGES = ["edge_c3_n65_b5", "edge_ident_c3_n65_b5", "edge_ext13_n65_b7"]
HID = "hid48_gcnoff"


# ---- CPU -------------------------------------------------------------------------------------------------------------
def _dims(c):
    from multistgraph_amd.ops import spec_from_config
    return spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), 0, 0).dims(c.b)


def test_deterministic_setter_and_train_bytes(lib_built):
    """the setter exists, starts at 0, returns the previous value, any non-zero value is on; matgcn_train_bytes counts the
    partial slabs while it is on (on top of mode 2's copies too) and matgcn_workspace_bytes never does"""
    from multistgraph_amd import _lib
    lib = _lib.load()
    assert lib.matgcn_set_deterministic(0) == 0
    try:
        assert lib.matgcn_set_deterministic(1) == 0
        assert lib.matgcn_set_deterministic(7) == 1
        assert lib.matgcn_set_deterministic(-3) == 1      # 7 meant on
        assert lib.matgcn_set_deterministic(0) == 1       # and so did -3
        assert lib.matgcn_set_deterministic(0) == 0
        assert lib.matgcn_set_train_precision(0) == 0     # the precision settings are untouched
        dims = _dims(Case("tiny_multi_uni_c2"))
        ws, tr = C.c_size_t(), C.c_size_t()

        def sizes():
            assert lib.matgcn_workspace_bytes(C.byref(dims), C.byref(ws)) == 0
            assert lib.matgcn_train_bytes(C.byref(dims), C.byref(tr)) == 0
            return ws.value, tr.value

        ws0, tr0 = sizes()
        lib.matgcn_set_deterministic(1)
        ws1, tr1 = sizes()
        assert ws1 == ws0 and tr1 > tr0
        lib.matgcn_set_train_precision(2)
        ws2, tr2 = sizes()
        lib.matgcn_set_deterministic(0)
        ws3, tr3 = sizes()
        assert ws2 == ws3 and tr2 - tr3 == tr1 - tr0      # the same slabs behind mode 2's copies
        lib.matgcn_set_train_precision(0)
        assert sizes() == (ws0, tr0)
    finally:
        lib.matgcn_set_deterministic(0)
        lib.matgcn_set_train_precision(0)


def test_header_binding_and_library_agree(lib_built):
    from multistgraph_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "matgcn.h")) as fh:
        header = fh.read()
    assert "int matgcn_set_deterministic(int enabled);" in header
    assert "#define MATGCN_ABI_VERSION 12" in header
    assert "matgcn_set_deterministic" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "matgcn_set_deterministic") and lib.matgcn_abi_version() == 12
    assert "fixed order" in header and "not bitwise" in header        # the sentence about atomics names both modes


@pytest.mark.parametrize("value", [None, True, False])
def test_hip_deterministic_key(value):
    """config['hip_deterministic'] is accepted, kept as an attribute and leaves the checkpoint format alone; None follows
    torch.use_deterministic_algorithms, True / False force the setting"""
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    torch.manual_seed(0)
    ref = MultiATGCN(c.config(), c.data_feature)
    torch.manual_seed(0)
    m = MultiATGCN(dict(c.config(), hip_deterministic=value), c.data_feature)
    assert m.hip_deterministic is value and ref.hip_deterministic is None
    sd, rd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(sd[k].shape == rd[k].shape and torch.equal(sd[k], rd[k]) for k in sd)
    before = torch.are_deterministic_algorithms_enabled()
    try:
        for flag in (True, False):
            torch.use_deterministic_algorithms(flag)
            assert m._deterministic() is (flag if value is None else value)
    finally:
        torch.use_deterministic_algorithms(before)


def test_hip_deterministic_rejects_other_values():
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    for bad in ("yes", 2, 0.5):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_deterministic=bad), c.data_feature)


# ---- GPU -------------------------------------------------------------------------------------------------------------
class _Run:
    """a case bound to the HIP path with ONE forward_train kept (deterministic setting on, so the train buffer holds the
    partial slabs); backward() back-propagates it again with the setting given"""

    def __init__(self, hp, state, x, d_out, mask=None, h0=None, gold=None, errors=None):
        self.hp, self.state, self.x, self.d_out, self.mask, self.h0 = hp, state, x, d_out, mask, h0
        self.gold, self.errors = gold, errors
        hp.deterministic = True
        self.y = hp.forward_train(x, mask, h0).clone()
        self.cache = {}

    def backward(self, deterministic=True, fresh=False):
        """(the default and deterministic gradients are computed once and shared, unless `fresh`)"""
        if fresh or deterministic not in self.cache:
            self.hp.deterministic = deterministic
            try:
                g = {k: v.clone() for k, v in self.hp.backward(self.x, self.d_out, self.state, self.mask, self.h0).items()}
            finally:
                self.hp.deterministic = True
            if fresh:
                return g
            self.cache[deterministic] = g
        return self.cache[deterministic]


def _case_run(name):
    c = Case(name)
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_%s.npz" % name))
    hp, dev, state = _path(c)
    h0 = c.h0()
    return _Run(hp, state, torch.from_numpy(c.x).to(dev), torch.from_numpy(gold["d_out"]).to(dev),
                torch.from_numpy(_fixture_mask(gold)).to(dev), None if h0 is None else h0.to(dev), gold,
                lambda g: {k: e for k, e in _errors(gold, g).items() if e > GRAD_TOL})


def _edge_run(name):
    from test_shape_edges import _Bound, _grad_errors
    p = _Bound(name)
    gold = p.c.grad_gold

    def errors(g):
        errs, bad = _grad_errors(gold, g)
        bad.update({k: e for k, e in errs.items() if e > GRAD_TOL})
        return bad

    return _Run(p.hp, p.state, p.x, torch.from_numpy(p.c.d_out()).to(p.dev), h0=p.h0, gold=gold, errors=errors)


def _hid_run(monkeypatch):
    """rnn_units = 48 with dense cells runs through the plugin class only (zero-padded to the kernels' 64): its binding,
    its padded state, mask and initial state"""
    from multistgraph_amd import hidden_pad
    from multistgraph_amd.model import MultiATGCN
    c = Case(HID)
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_%s.npz" % HID))
    dev = torch.device("cuda:0")
    m = MultiATGCN(c.config("cuda:0"), c.data_feature).to(dev)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    if c.static_dim:
        v = torch.from_numpy(c.gold["pca_v"]).to(dev)
        monkeypatch.setattr(torch, "pca_lowrank", lambda A, q=None, center=True, niter=2: (None, None, v))
    with torch.no_grad():
        h0 = m._initial_state(c.b)
        h0 = None if h0 is None else hidden_pad.pad_last(h0).contiguous()
        hp = m._path_for_batch(c.b, dev)
        state = {k: v for k, v in m._state().items() if not k.startswith("static_initial")}
        mask = hidden_pad.pad_last(torch.from_numpy(_fixture_mask(gold)).to(dev)).contiguous()
    return _Run(hp, state, torch.from_numpy(c.x).to(dev), torch.from_numpy(gold["d_out"]).to(dev), mask, h0, gold)


@pytest.fixture(scope="module")
def runs(lib_built):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _edge_run(name) if name.startswith("edge_") else _case_run(name)
        return cache[name]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _assert_same_bits(a, b):
    assert set(a) == set(b)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + EDGES + CONFIG_EDGES)
def test_three_deterministic_backwards_have_equal_bits(name, runs):
    r = runs(name)
    first = r.backward()
    assert all(torch.isfinite(v).all() for v in first.values())
    for _ in range(2):
        _assert_same_bits(first, r.backward(fresh=True))
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_padded_dense_cells_have_equal_bits(lib_built, monkeypatch):
    r = _hid_run(monkeypatch)
    first = r.backward()
    assert all(torch.isfinite(v).all() for v in first.values())
    for _ in range(2):
        _assert_same_bits(first, r.backward(fresh=True))
    want = r.backward(False)
    for k in want:
        scale = float(want[k].abs().max()) + 1e-30
        assert float((want[k] - first[k]).abs().max()) <= GRAD_TOL * scale, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES + EDGES + CONFIG_EDGES)
def test_deterministic_gradients_match_the_fixture_and_the_default(name, runs):
    """the metric and tolerance of test_backward_matches_reference_autograd (edge cases: of
    test_training_step_matches_the_float64_autograd), and 1e-4 max-normalised against the default backward on the same
    saved activations; the gap to the default path is printed (DESIGN.md section 5c records it)"""
    r = runs(name)
    det, dflt = r.backward(), r.backward(False)
    grads = {k: v for k, v in det.items() if k != D_H0}
    bad = r.errors(grads)
    gaps = {k: float((det[k] - dflt[k]).abs().max()) / (float(dflt[k].abs().max()) + 1e-30) for k in dflt}
    worst = max(gaps, key=gaps.get)
    print("%s: deterministic vs default backward %.3e (%s)" % (name, gaps[worst], worst))
    assert not bad, bad
    assert set(det) == set(dflt)
    assert gaps[worst] <= GRAD_TOL, (worst, gaps[worst])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "edge_n257_b33"])
def test_default_backward_is_unharmed(name, runs):
    """a default backward after a deterministic one is the default backward before it, up to the order of its atomics"""
    r = runs(name)
    before = r.backward(False, fresh=True)
    r.backward(True, fresh=True)
    after = r.backward(False, fresh=True)
    _same_up_to_atomics(before, after)
    assert r.hp.lib.matgcn_set_deterministic(0) == 0       # the binding restored the process-wide setting


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "edge_n257_b33"])
def test_serial_and_wavefront_schedules_have_equal_bits(name, runs):
    """what crosses the library's streams is ordered too: matgcn_set_wavefront(0) against the wavefront, each with a
    forward_train of its own"""
    r = runs(name)
    hp = r.hp
    res = {}
    prev = hp.lib.matgcn_set_wavefront(1)
    try:
        for mode in (1, 0):
            hp.lib.matgcn_set_wavefront(mode)
            assert torch.equal(hp.forward_train(r.x, r.mask, r.h0), r.y)
            res[mode] = r.backward(fresh=True)
            torch.cuda.synchronize()
    finally:
        hp.lib.matgcn_set_wavefront(prev)
        hp.forward_train(r.x, r.mask, r.h0)                # the shared run's activations are the wavefront's again
    _assert_same_bits(res[1], res[0])
    _assert_same_bits(res[1], r.backward())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "edge_n257_b33"])
def test_nothing_depends_on_stale_scratch(name, runs):
    """twice with a fresh train buffer of NaN bytes in front of forward_train: the same bits as the shared run"""
    r = runs(name)
    hp = r.hp
    keep = hp._train
    try:
        for _ in range(2):
            hp._train = torch.empty_like(keep)
            hp._train.view(torch.uint8).fill_(0xFF)
            assert torch.equal(hp.forward_train(r.x, r.mask, r.h0), r.y)
            _assert_same_bits(r.backward(), r.backward(fresh=True))
    finally:
        hp._train = keep
        hp.forward_train(r.x, r.mask, r.h0)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_precision_modes_compose(mode, lib_built):
    """training precision modes 1 and 2 change operands, not reductions: bit-identical under the setting as well"""
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    hp, dev, state = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    d_out = torch.from_numpy(gold["d_out"]).to(dev)
    hp.precision = mode
    plain = hp.forward_train(x, mask).clone()
    hp.deterministic = True
    assert torch.equal(hp.forward_train(x, mask), plain)   # the forward does not see the setting
    a = {k: v.clone() for k, v in hp.backward(x, d_out, state, mask).items()}
    b = hp.backward(x, d_out, state, mask)
    _assert_same_bits(a, b)
    y32, g32 = _step(hp, c, gold, dev, state, None)
    assert any(not torch.equal(a[k], g32[k]) for k in g32)  # the bf16 backward ran


@pytest.mark.gpu
def test_forward_train_is_untouched(runs, lib_built):
    r = runs("tiny_multi_uni_c2")
    hp = r.hp
    try:
        hp.deterministic = False
        assert torch.equal(hp.forward_train(r.x, r.mask, r.h0), r.y)
    finally:
        hp.deterministic = True
        hp.forward_train(r.x, r.mask, r.h0)


@pytest.mark.gpu
def test_small_train_buffer_is_refused(lib_built):
    """a deterministic matgcn_backward on a train buffer of the default size: MATGCN_ERR_SMALL_BUFFER from the host-side
    size check, before any launch"""
    from multistgraph_amd import _lib
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    hp, dev, state = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    d_out = torch.from_numpy(gold["d_out"]).to(dev)
    hp.forward_train(x, mask)                              # default setting: the default size
    hp.deterministic = True
    with pytest.raises(_lib.MatgcnError) as err:
        hp.backward(x, d_out, state, mask)
    assert "(status -4)" in str(err.value)                 # MATGCN_ERR_SMALL_BUFFER
    hp.deterministic = None
    assert all(torch.isfinite(v).all() for v in hp.backward(x, d_out, state, mask).values())   # the default still runs


@pytest.mark.gpu
def test_two_training_runs_from_one_state_are_identical(lib_built, monkeypatch):
    """the point of it all: 10 Adam steps through the plugin with hip_deterministic = True, twice from the same state -
    equal losses and equal final parameters, bit for bit"""
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    dev = torch.device("cuda:0")
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda inp, p=0.5, training=True, inplace=False: inp)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}

    def run():
        model = MultiATGCN(dict(c.config("cuda:0"), hip_deterministic=True), c.data_feature).to(dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=3e-3)
        losses = []
        for _ in range(10):
            opt.zero_grad()
            loss = model.calculate_loss(batch)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}

    la, pa = run()
    lb, pb = run()
    assert la == lb
    assert la[-1] < la[0]
    _assert_same_bits(pa, pb)
    from multistgraph_amd import _lib
    assert _lib.load().matgcn_set_deterministic(0) == 0    # restored around every call
