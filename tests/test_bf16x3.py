"""Precision mode 3 of matgcn_set_mix_precision (include/matgcn.h): the graph mixes of the inference forward on the bf16
matrix instruction, both operands split into three bf16 pieces, the six leading cross products accumulated in fp32.

The claim is "as accurate as the fp32 path", so every tolerance here is the fp32 path's own and none is derived from what
the kernel gives: 1e-4 max-normalised and element-wise against the float64 oracle at the shape edges
(test_shape_edges.py), twice the reference's own fp32-vs-float64 gap at the real sizes (test_hip_parity.py,
_fp64_gap_check, restated below), three times that gap between two results that both sit within it.  A single-product
bf16 mix (mode 1) misses the second by three orders of magnitude.

Every accuracy test prints its measured distance next to the reference's own gap.  On an MI355X: 4.1e-7 .. 6.4e-7
max-normalised at the seven edges (the fp32 forward 4.0e-7 .. 8.2e-7), worst element 3.87e-7 / 2.66e-7 from float64 at
bm403_out24 / synth4096_out24 where the reference's own fp32 run is 4.45e-7 / 4.69e-7 away.

CONFIG_EDGES adds three stacks of other configurations past one tile (test_shape_edges.py has their table) - Ks 6 from the
Chebyshev recursion, Ks 1 from accumulated supports over three layers, Ks 1 from the adaptive support alone: 4.3e-7, 6.1e-7
and 3.9e-7 from float64 (the fp32 forward 4.6e-7, 6.8e-7, 4.3e-7).  Mode 3 only: the bf16 modes 1 and 2 stay out of these
cases, because their 5e-3 / 2.7e-2 bounds were measured on cheb_order 2 stacks only and nothing tells what a squared
support costs them.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers import Case, EdgeCase, elementwise_excess, max_norm_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

E2E_TOL = 1e-4
MODE = 3
# every rule the mix kernels are chosen by (test_shape_edges.py has the table): ragged 64-row tile and an odd number of
# column tiles; either side of the small-batch tile rule (17 column tiles: the last 128-wide tile is half empty); N % 8 = 7;
# two row blocks; the longest chain without partial sums (32 K-tiles of 32); partial sums with 65 K-groups of 16 - the
# last K-tile of 32 is half zeros and the last group of eight tiles holds one
EDGES = ["edge_n48_b3", "edge_n64_b17", "edge_n65_b16", "edge_n263_b8", "edge_n257_b65", "edge_n1024_b2", "edge_n1039_b2"]
# the stacks of other configurations, whose planes (Ks * nKg * NpC) scale with them: Ks 6 built by the Chebyshev recursion
# (a squared support in three pieces), Ks 1 from three accumulated supports over three layers, Ks 1 from the adaptive
# support alone.  Mode 3 only: the 5e-3 / 2.7e-2 bounds of the bf16 modes 1 and 2 were measured on cheb_order 2 stacks, and
# nothing tells what a squared support costs them - they stay out of these cases
CONFIG_EDGES = ["edge_c3_n65_b5", "edge_c1_n65_b17_l3", "edge_oduni_n65_b3"]


class _Mode:
    """matgcn_set_mix_precision(mode) around a block, the previous setting restored"""

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.prev = self.lib.matgcn_set_mix_precision(self.mode)
        return self.prev

    def __exit__(self, *exc):
        self.lib.matgcn_set_mix_precision(self.prev)


class _Bound:
    """an edge case bound to the HIP path; its fp32 forward is taken BEFORE mode 3 is ever set on this binding, its
    mode-3 forward once"""

    def __init__(self, name):
        from multistgraph_amd.ops import HotPath
        c = self.c = EdgeCase(name)
        self.dev = torch.device("cuda:0")
        spec, st = c.spec_and_static()
        self.hp = HotPath(spec, c.b, self.dev)
        self.hp.bind({k: torch.from_numpy(v).to(self.dev) for k, v in c.state.items()},
                     None if st is None else st.to(self.dev))
        self.x = torch.from_numpy(c.x).to(self.dev)
        self.pred32 = self.hp.forward(self.x).clone()
        with _Mode(self.hp.lib, MODE):
            self.pred3 = self.hp.forward(self.x).clone()


@pytest.fixture(scope="module")
def bound(lib_built):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Bound(name)
        return cache[name]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _case_path(c, batch=None):
    """a golden case (reference vectors) bound to the HIP path, as test_hip_parity.py binds it"""
    from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
    dev = torch.device("cuda:0")
    if c.meta.get("big"):     # N = 4096: the static supports come from the host graph prep (test_hip_parity._big_path)
        from multistgraph_amd import graph_prep
        mats = np.stack(graph_prep.build_static_supports(c.data_feature["adj_mx"], c.data_feature["coordinate"], None,
                                                         c.adjtype), 0)
        st = torch.from_numpy(mats).to(dev)
        mask = diagonal_mask(torch.from_numpy(mats))
    else:
        st = torch.from_numpy(c.gold["static_supports"]).to(dev)
        mask = diagonal_mask(st)
    b = c.b if batch is None else batch
    spec = spec_from_config(dict(c.config(), batch_size=b), c.data_feature, c.n, min(c.n, 20), st.shape[0], mask)
    hp = HotPath(spec, b, dev)
    hp.bind({k: torch.from_numpy(v).to(dev) for k, v in c.state.items()}, st)
    return hp, dev


def _fp64_gap_check(name, got, ref32, factor=2.0):
    """test_hip_parity._fp64_gap_check: |got - ref64| against the reference's OWN |ref32 - ref64| on the elements
    fp64_gap.npz holds, the worst element and the r.m.s. within ``factor``.  Returns (gap_ref max, gap_hip max)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "fp64_gap.npz"))
    sub = int(z[name + "_sub"])
    p64 = z[name + "_pred64"]
    g = np.asarray(got, dtype=np.float64).reshape(-1)[::sub]
    r = np.asarray(ref32, dtype=np.float64).reshape(-1)[::sub]
    assert g.shape == p64.shape == r.shape
    e_ref, e_hip = np.abs(r - p64), np.abs(g - p64)
    rms_ref, rms_hip = float(np.sqrt((e_ref ** 2).mean())), float(np.sqrt((e_hip ** 2).mean()))
    print("%s mode 3: reference fp32-vs-fp64 gap max %.3e rms %.3e | HIP-vs-fp64 max %.3e rms %.3e (max|y| %.4f)" % (
        name, e_ref.max(), rms_ref, e_hip.max(), rms_hip, np.abs(p64).max()))
    assert e_hip.max() <= factor * e_ref.max(), (e_hip.max(), e_ref.max())
    assert rms_hip <= factor * rms_ref, (rms_hip, rms_ref)
    return float(e_ref.max()), float(e_hip.max())


# ---- 1. accuracy at every mix rule ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", EDGES + CONFIG_EDGES)
def test_mode3_matches_the_float64_oracle_at_fp32_tolerance(name, bound):
    p = bound(name)
    got, want = p.pred3.cpu().numpy(), p.c.gold["pred64"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err, excess = max_norm_err(got, want), elementwise_excess(got, want)
    print("%s: mode-3 forward vs fp64 %.3e (element-wise excess %.3f); fp32 forward vs fp64 %.3e; oracle fp32 vs fp64 "
          "%.3e" % (name, err, excess, max_norm_err(p.pred32.cpu().numpy(), want), float(p.c.gold["gap32_pred"])))
    assert not torch.equal(p.pred3, p.pred32)                    # the variant really ran
    assert err <= E2E_TOL, err
    assert excess <= 1.0, excess


# ---- 2. the fp64 gap at the real sizes --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ["bm403_out24", "synth4096_out24"])
def test_mode3_is_as_close_to_float64_as_the_fp32_path_must_be(name, lib_built):
    """the bound the fp32 path is held to (factor 2.0), at N = 403 (B = 4) and at N = 4096 (B = 2: partial sums)"""
    c = Case(name)
    hp, dev = _case_path(c)
    x = torch.from_numpy(c.x).to(dev)
    with _Mode(hp.lib, MODE):
        got = hp.forward(x).cpu().numpy()
    assert max_norm_err(got, c.gold["pred"]) <= E2E_TOL
    _fp64_gap_check(name, got, c.gold["pred"])
    del hp
    torch.cuda.empty_cache()


# ---- 3. it is its own kernel, with its own workspace tail -------------------------------------------------------------
@gpu
def test_mode3_is_its_own_kernel_and_sizes_its_own_workspace(lib_built):
    c = Case("bm403_out24")
    hp, dev = _case_path(c)
    lib = hp.lib
    x = torch.from_numpy(c.x).to(dev)
    exact = hp.forward(x).clone()
    n0, n3 = C.c_size_t(), C.c_size_t()
    assert lib.matgcn_workspace_bytes(C.byref(hp.dims), C.byref(n0)) == 0
    with _Mode(lib, MODE):
        assert lib.matgcn_workspace_bytes(C.byref(hp.dims), C.byref(n3)) == 0
        small = torch.empty(n0.value // 4, dtype=torch.float32, device=dev)
        out = torch.empty_like(exact)
        status = lib.matgcn_forward(C.byref(hp.dims), C.byref(hp.params), C.c_void_p(hp.prepared.data_ptr()),
                                    C.c_void_p(x.data_ptr()), None, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(small.data_ptr()), C.c_size_t(n0.value), hp._stream())
        assert status == -4                                      # MATGCN_ERR_SMALL_BUFFER
        got = hp.forward(x).clone()                              # the binding re-sizes and repeats
    # three bf16 planes of the support stack [Np rounded up to 32][Ks * Np rounded up to 64]: 6 bytes per element
    lay = (C.c_int64 * 4)()
    assert lib.matgcn_supports_layout(C.byref(hp.dims), C.byref(lay)) == 0
    ld, np_ = int(lay[1]), int(lay[2])
    planes = 6 * ((np_ + 31) // 32 * 32) * ld
    assert n3.value - n0.value == (planes + 255) // 256 * 256, (n3.value - n0.value, planes)
    assert hp.workspace.numel() * 4 == n3.value
    assert not torch.equal(got, exact)
    gap_ref, _ = _fp64_gap_check("bm403_out24", got.cpu().numpy(), c.gold["pred"])
    floor = 3.0 * gap_ref / float(np.abs(c.gold["pred"]).max())
    dist = max_norm_err(got.cpu().numpy(), exact.cpu().numpy())
    print("bm403_out24: mode 3 vs mode 0 %.3e max-normalised; floor 3 x gap_ref = %.3e" % (dist, floor))
    assert float((got - exact).abs().max()) <= 3.0 * gap_ref
    assert torch.equal(hp.forward(x), exact)


# ---- 4. nothing else moved --------------------------------------------------------------------------------------------
@gpu
def test_setter_returns_the_previous_mode(lib_built):
    from multistgraph_amd import _lib
    lib = _lib.load()
    prev = lib.matgcn_set_mix_precision(0)
    try:
        assert lib.matgcn_set_mix_precision(3) == 0
        assert lib.matgcn_set_mix_precision(3) == 3
        assert lib.matgcn_set_mix_precision(4) == 3              # any other value means 0
        assert lib.matgcn_set_mix_precision(0) == 0
        assert lib.matgcn_set_train_precision(3) == 0            # training has no mode 3: it means 0
        assert lib.matgcn_set_train_precision(0) == 0
    finally:
        lib.matgcn_set_mix_precision(prev)


@gpu
@pytest.mark.parametrize("name", ["edge_n257_b65", "edge_n64_b17"])
def test_the_other_modes_keep_their_bits_around_a_mode3_forward(name, bound):
    p = bound(name)                                              # pred32 was taken before mode 3 was ever set
    lib = p.hp.lib
    before = {}
    for mode in (1, 2):
        with _Mode(lib, mode):
            before[mode] = p.hp.forward(p.x).clone()
    with _Mode(lib, MODE):
        assert torch.equal(p.hp.forward(p.x), p.pred3)
    assert torch.equal(p.hp.forward(p.x), p.pred32)              # fp32 after set_mix_precision(0): the bits of before
    for mode in (1, 2):
        with _Mode(lib, mode):
            assert torch.equal(p.hp.forward(p.x), before[mode])
        assert not torch.equal(before[mode], p.pred3)
    assert torch.equal(p.hp.forward(p.x), p.pred32)


@gpu
def test_wavefront_and_serial_schedules_agree_bitwise_in_mode3(bound):
    p = bound("edge_n65_b16")
    lib = p.hp.lib
    prev = lib.matgcn_set_wavefront(1)
    try:
        with _Mode(lib, MODE):
            a = p.hp.forward(p.x).clone()
            lib.matgcn_set_wavefront(0)
            b = p.hp.forward(p.x).clone()
            zeros = torch.zeros(p.hp.spec.layers, p.hp.batch, p.hp.spec.nodes, p.hp.spec.hidden, device=p.dev)
            from_zeros = p.hp.forward(p.x, zeros).clone()        # the general step 0: mixes of the all-zero state
    finally:
        lib.matgcn_set_wavefront(prev)
    assert torch.equal(a, b) and torch.equal(a, p.pred3)
    assert torch.equal(a, from_zeros)


@gpu
def test_forward_series_equals_forward_on_gathered_windows_in_mode3(lib_built):
    from multistgraph_amd import windows as W
    c = Case("tiny_multi_uni_c2")
    hp, dev = _case_path(c)
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, c.feat)).astype(np.float32)
    starts = W.valid_label_starts(steps, rel, 24)
    pick = starts[rng.permutation(len(starts))[:c.b]].astype(np.int32)
    sd, pd = torch.from_numpy(series).to(dev), torch.from_numpy(pick).to(dev)
    x, _ = W.gather_windows(series, pick, rel, c.out)
    xd = torch.from_numpy(x).to(dev)
    exact = hp.forward(xd).clone()
    with _Mode(hp.lib, MODE):
        got = hp.forward_series(sd, pd, rel).clone()
        assert torch.equal(got, hp.forward(xd))
    assert not torch.equal(got, exact)
    assert torch.equal(hp.forward_series(sd, pd, rel), exact)


@gpu
def test_plugin_inference_in_bf16x3(lib_built):
    """predict() with hip_precision = "bf16x3" is HotPath.forward under matgcn_set_mix_precision(3), bit for bit, and
    leaves both library settings as it found them"""
    from multistgraph_amd import _lib
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    m = MultiATGCN(dict(c.config("cuda:0"), hip_precision="bf16x3"), c.data_feature).to(dev).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    x = torch.from_numpy(c.x).to(dev)
    with torch.no_grad():
        got = m.predict({"X": x}).clone()
        hp = m._path_for(x)
    assert lib.matgcn_set_mix_precision(0) == 0 and lib.matgcn_set_train_precision(0) == 0
    hp.precision = None
    with _Mode(lib, MODE):
        want = hp.forward(x).clone()
    assert torch.equal(got, want)
    assert not torch.equal(got, hp.forward(x))


# ---- 5. host side -----------------------------------------------------------------------------------------------------
def test_hip_precision_bf16x3_is_a_config_value():
    from multistgraph_amd.model import HIP_PRECISIONS, MultiATGCN
    c = Case("tiny_multi_uni_c2")
    assert HIP_PRECISIONS["bf16x3"] == 3
    m = MultiATGCN(dict(c.config(), hip_precision="bf16x3"), c.data_feature)
    assert m.hip_precision == "bf16x3"
    assert MultiATGCN(c.config(), c.data_feature).hip_precision == "fp32"
    for bad in ("bf16x2", "bf16x3 ", 3):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_precision=bad), c.data_feature)


def test_header_binding_and_library_agree_on_mode3(lib_built):
    from multistgraph_amd import _lib
    header = open(os.path.join(ROOT, "include", "matgcn.h")).read()
    declared = set(re.findall(r"\b(matgcn_[a-z_0-9]+)\s*\(", header))
    assert declared == set(_lib.EXPORTED_SYMBOLS)
    abi = int(re.search(r"#define\s+MATGCN_ABI_VERSION\s+(\d+)", header).group(1))
    lib = _lib.load()
    assert lib.matgcn_abi_version() == _lib.ABI_VERSION == abi
    assert "matgcn_set_mix_precision(3)" in header
    prev = lib.matgcn_set_mix_precision(3)
    try:
        assert lib.matgcn_set_mix_precision(prev) == 3           # the library knows the mode (before it: 3 meant 0)
    finally:
        lib.matgcn_set_mix_precision(prev)
