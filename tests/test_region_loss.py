"""The region-level training loss on the GPU (csrc/matgcn_region_loss.hip: k_region_grad_tile / k_region_grad_walk behind
matgcn_region_loss_grad; matgcn_region_loss composes the total kernels with k_loss_partial / k_loss_final) against the numpy
reference of tests/region_loss_ref.py, which tests/test_region_loss_host.py checks against finite differences first.

COMPOSITION: the (1 + out) values are the bits of train_loss_device(group_sums(pred), group_label_sums(y)) with an identity
affine - every name, window labels and label_start.
EXACT: grid-valued inputs under region_loss_ref.assert_region_exact (asserted per case on the reference alone): values
bit-equal to the reference; the gradient zero where the reference is zero, bit-equal or within one float32 spacing
elsewhere, 2^-22 relative for mape (the rule of test_train_loss._assert_exact_grad).
REALISTIC: continuous draws at B = 5, out = 24, N = 403 under Baltimore's scaler, ten regions plus the whole city: value and
gradient against the float64 reference within max(2 x gap, 2^-22), gap = the error of a float32 CPU torch run of the same
arithmetic (dense membership matmul, train_loss_ref.torch_loss, autograd).  Both start from the same float32 de-scaled
values.  logcosh alone uses a unit scaler: the float32 log(cosh) of the torch run overflows past |d| = 89, which region
totals under Baltimore's std = 29.3 exceed; that departure is test_train_loss's subject, not this file's, so the draw is
kept where the yardstick is a number (asserted)."""
import ctypes as C
import functools
import gc
import os

import numpy as np
import pytest
import torch

import region_loss_ref as RL
import train_loss_ref as T
from helpers import GOLDEN_DIR, Case, max_norm_err

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -22
UPSTREAM = 4.0          # a power of two keeps upstream * std exact
EXACT_NAMES = ("mae", "masked_mae", "mse", "masked_mse", "rmse", "masked_rmse", "huber", "quantile")
MAPE_NAMES = ("mape", "masked_mape")
ELEVEN = tuple(T.LOSSES)
ZERO_FREE = ("mape", "logcosh", "huber", "quantile")
GOLD = np.load(os.path.join(GOLDEN_DIR, "train_loss_small.npz"))
MEAN, STD = float(GOLD["mean"]), float(GOLD["std"])


@pytest.fixture(scope="module", autouse=True)
def _leave_the_allocator_as_found():
    """as in test_train_loss: the models of the end-to-end tests die in reference cycles; collect them with the module.
    The cached region maps keep their device copies: drop them too, or the blocks they pin change which address the
    caching allocator hands a later module that watches it."""
    yield
    for cached in (_map, _city_map, _grid):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ---- maps -----------------------------------------------------------------------------------------------------------------
def _weights(groups, kind, seed=3):
    if kind is None or kind == "mean":
        return kind
    rng = np.random.default_rng(seed)
    if kind == "dyadic":
        return [rng.choice([1.0, 0.5, 2.0], len(g)).tolist() for g in groups]
    assert kind == "continuous"
    return [rng.uniform(0.25, 1.75, len(g)).astype(F32).tolist() for g in groups]


def _mixed_groups(n):
    """an empty group, the whole city, nested and overlapping groups, a node twice in one group, and nodes n-1, n-2, n-3
    in 8, 9 and 17 groups (below, at and twice past the prefetch depth REGION_AHEAD = 8) next to nodes in one group"""
    if n < 16:
        return [[], list(range(n)), list(range(n))[::-1][:max(1, n // 2)]]
    a, b, c = n - 1, n - 2, n - 3
    groups = [[], list(range(n)), list(range(n // 2)), list(range(n // 4)), [n - 4, 5, n - 4]]
    for i in range(16):
        groups.append([c] + ([b] if i < 8 else []) + ([a] if i < 7 else []) + [(n // 2 + i) % (n - 4)])
    return groups


def _small_groups(n, n_groups, n_members):
    """n_groups groups of one or two members over n nodes, n_members memberships in all"""
    assert n_groups <= n_members <= 2 * n_groups
    two = n_members - n_groups
    return [[i % n, (7 * i + 3) % n] if i < two else [i % n] for i in range(n_groups)]


@functools.lru_cache(maxsize=None)
def _map(kind, n, weights=None):
    from multistgraph_amd.regions import RegionMap
    if kind == "partition":            # three regions by label, every seventh node in none
        groups = [[k for k in range(n) if k % 7 != 6 and k % 3 == g] for g in range(3)]
    elif kind == "eights":             # consecutive groups of 8 (weights "mean" = 1/8 stay dyadic); the rest in none
        groups = [list(range(8 * g, 8 * g + 8)) for g in range(max(1, n // 8))] if n >= 8 else [[0]]
    elif kind == "mixed":
        groups = _mixed_groups(n)
    elif kind == "whole":
        groups = [list(range(n))]
    else:
        tag, n_groups, n_members = kind
        assert tag == "small"
        groups = _small_groups(n, n_groups, n_members)
    return RegionMap(n, groups=groups, weights=_weights(groups, weights))


def test_the_mixed_map_is_what_the_cases_need():
    rm = _map("mixed", 257)
    nptr = rm.by_node()[0]
    counts = np.diff(nptr)
    assert {1, 8, 9, 17} <= set(counts.tolist()) and counts[256] == 8 and counts[255] == 9 and counts[254] == 17
    assert rm.members(0) == [] and rm.members(1) == list(range(257)) and rm.members(4).count(253) == 2
    assert (np.diff(_map("partition", 257).by_node()[0]) == 0).sum() == 36       # nodes in no group


# ---- running a case -------------------------------------------------------------------------------------------------------
def _ls(label_start):
    return None if label_start is None else _dev(np.asarray(label_start, dtype=np.int32))


def _run(name, c, rm, label_start=None, delta=None, upstream=UPSTREAM):
    """((1 + out,) values, gradient) of case c through ops.region_loss_device / ops.region_train_loss"""
    from multistgraph_amd import ops
    ls, y = _ls(label_start), _dev(c["y"])
    p = _dev(c["pred"]).requires_grad_(True)
    full = ops.region_loss_device(p.detach(), y, rm, c["y_start"], c["mean"], c["std"], name, delta, ls)
    loss = ops.region_train_loss(p, y, rm, c["y_start"], c["mean"], c["std"], name, delta, ls)
    (loss * upstream).backward()
    full = _host(full)
    assert full.dtype == F32 and _same(full[0], _host(loss)).all()
    return full, _host(p.grad)


def _raw(name, c, rm, fill=None, base=None, upstream=UPSTREAM, by_node=None, short=0):
    """matgcn_region_loss / matgcn_region_loss_grad on caller buffers pre-filled with ``fill``: (values, gradient, scratch).
    base: None, "alias" (d_pred itself holds it) or "separate"; both start from the values of ``c["base"]``."""
    from multistgraph_amd import _lib, ops
    lib = _lib.load()
    pred, y = _dev(c["pred"]), _dev(c["y"])
    b, out, n, od = pred.shape
    desc = ops.train_loss_desc(name, c["mean"], c["std"])
    need = C.c_size_t()
    _lib.check(lib.matgcn_region_loss_bytes(b, out, rm.num_groups, od, C.byref(need)), "matgcn_region_loss_bytes")
    assert need.value % 8 == 0
    scratch = torch.full((need.value // 8,), 0.0 if fill is None else fill, dtype=torch.float64, device=pred.device)
    result = torch.full((1 + out,), 0.0 if fill is None else fill, dtype=torch.float32, device=pred.device)
    d_pred = torch.full_like(pred, 0.0 if fill is None else fill)
    base_t = None
    if base == "alias":
        d_pred = _dev(c["base"]).clone()
        base_t = d_pred
    elif base == "separate":
        base_t = _dev(c["base"]).clone()
    up = torch.full((1,), upstream, dtype=torch.float32, device=pred.device)
    stream = C.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
    geo = (b, out, n, od, int(y.shape[1]), int(y.shape[3]), c["y_start"])
    bg = rm.groups_on(pred.device)
    bn = (rm if by_node is None else by_node).node_groups_on(pred.device)
    _lib.check(lib.matgcn_region_loss(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), None, *geo, C.byref(desc),
                                      C.byref(bg), C.c_void_p(scratch.data_ptr()), need.value - short,
                                      C.c_void_p(result.data_ptr()), stream), "matgcn_region_loss")
    _lib.check(lib.matgcn_region_loss_grad(C.c_void_p(pred.data_ptr()), C.c_void_p(y.data_ptr()), None, *geo,
                                           C.byref(desc), C.byref(bg), C.byref(bn), C.c_void_p(scratch.data_ptr()),
                                           need.value, C.c_void_p(up.data_ptr()),
                                           C.c_void_p(None if base_t is None else base_t.data_ptr()),
                                           C.c_void_p(d_pred.data_ptr()), stream), "matgcn_region_loss_grad")
    return _host(result), _host(d_pred), _host(scratch)


def _ref(name, c, rm, label_start=None, delta=None, upstream=UPSTREAM, base=None, reverse=False, dtype=F32):
    return RL.region_loss_ref(name, c["pred"], c["y"], c["y_start"], c["mean"], c["std"], rm.ptr, rm.node, rm.weight,
                              delta, label_start, upstream, base, reverse, dtype)


def _assert_exact_values(name, got, want):
    if name in MAPE_NAMES:
        with np.errstate(invalid="ignore"):
            ok = _same(got, want["values"]) | (np.abs(got - want["values"]) <= FLOOR * np.abs(want["values"]))
        assert ok.all(), (name, got, want["values"])
    else:
        assert np.array_equal(got, want["values"].astype(F32)), (name, got, want["values"].astype(F32))


def _assert_exact_grad(name, got, want):
    """the rule of test_train_loss._assert_exact_grad"""
    g = want["grad"]
    assert got.dtype == F32 and got.shape == g.shape
    zero = g == 0
    assert (got[zero] == 0).all(), "%s: a gradient where the reference has none" % name
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(F64) - g)
        tol = FLOOR * np.abs(g) if name in MAPE_NAMES else np.spacing(np.abs(g).astype(F32)).astype(F64)
        ok = _same(got, g.astype(F32)) | (err <= tol)
    assert ok.all(), (name, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], g[~ok][:5])


# ---- COMPOSITION ----------------------------------------------------------------------------------------------------------
def _shape(b=3, out=6, n=257, od=1, y_steps=None, y_feat=None, y_start=0):
    return (b, out, n, od, out if y_steps is None else y_steps, y_start + od if y_feat is None else y_feat, y_start)


SHAPES = {"base": _shape()}
# N * od across the 256-thread block: one element, one short of a block, a block, and three channels
for _n, _od in ((1, 1), (255, 1), (256, 1), (171, 3)):
    SHAPES["n%d_od%d" % (_n, _od)] = _shape(n=_n, od=_od)
SHAPES["od2_feat5_start2"] = _shape(od=2, y_feat=5, y_start=2)
for _out in (1, 24, 64):
    SHAPES["out%d" % _out] = _shape(out=_out, n=65)
SHAPES["b1"] = _shape(b=1)
# B * out = 1025 rows of N = 5: the gradient kernel takes R = 2 rows per tile (region_loss_ref.rows_per_tile, asserted in
# the test), so the last tile holds one row - one past 512 full tiles
SHAPES["rows_one_past_a_tile"] = _shape(b=25, out=41, n=5)
SHAPE_IDS = list(SHAPES)


@functools.lru_cache(maxsize=None)
def _grid(shape_name, nan_labels):
    b, out, n, od, y_steps, y_feat, y_start = SHAPES[shape_name]
    c = T.grid_case(SHAPE_IDS.index(shape_name) + 1, b, out, n, od, y_steps=y_steps, y_feat=y_feat, y_start=y_start)
    if nan_labels:
        rng = np.random.default_rng(7)
        c = dict(c, y=c["y"].copy())
        c["y"].reshape(-1)[rng.integers(0, c["y"].size, max(1, c["y"].size // 50))] = NAN
    return c


def _case_for(name, shape_name):
    return _grid(shape_name, T.LOSSES[name][0] in T.MASKED and not name.startswith("masked_"))


def test_value_is_the_composition_of_the_three_entry_points(lib_built):
    """bit-equal to train_loss_device(group_sums(pred), group_label_sums(y)) with an identity affine: every name, window
    labels and label_start, continuous data"""
    from multistgraph_amd import ops
    t_steps, out, n, od, feat, y_start, b = 40, 6, 257, 2, 4, 1, 5
    rng = np.random.default_rng(31)
    series = rng.standard_normal((t_steps, n, feat)).astype(F32)
    series[rng.random(series.shape) < 0.01] = F32(-MEAN / STD)
    starts = np.array([0, t_steps - out, 5, 5, 7], dtype=np.int32)
    windows = np.stack([series[s:s + out] for s in starts], 0)
    pred = (windows[..., y_start:y_start + od] + 0.3 * rng.standard_normal((b, out, n, od))).astype(F32)
    pd, wd, sd, ls = _dev(pred), _dev(windows), _dev(series), _dev(starts)
    for weights in (None, "continuous"):
        rm = _map("mixed", n, weights)
        P = ops.group_sums(pd, rm, mean=MEAN, std=STD)
        for y, start in ((wd, None), (sd, ls)):
            L = ops.group_label_sums(y, rm, out, od, y_start, mean=MEAN, std=STD, label_start=start)
            assert L.shape == P.shape == (b, out, rm.num_groups, od)
            for name in ELEVEN:
                want = ops.train_loss_device(P, L, 0, 0.0, 1.0, name)
                got = ops.region_loss_device(pd, y, rm, y_start, MEAN, STD, name, None, start)
                assert got.shape == (1 + out,) and _bits_equal(_host(got), _host(want)), (name, start is None)
                assert np.isfinite(_host(got)).all()


# ---- EXACT ----------------------------------------------------------------------------------------------------------------
def _check_exact(names, c_for, rm, label_start=None, grid_bits=RL.GRID_BITS):
    for name in names:
        c = c_for(name)
        RL.assert_region_exact(name, c, rm.ptr, rm.node, rm.weight, None, label_start, grid_bits)
        want = _ref(name, c, rm, label_start)
        got, grad = _run(name, c, rm, label_start)
        _assert_exact_values(name, got, want)
        _assert_exact_grad(name, grad, want)
        outside = np.diff(rm.by_node()[0]) == 0
        assert _bits_equal(grad[:, :, outside], np.zeros_like(grad[:, :, outside])), "a node in no group: +0.0"
        if name not in MAPE_NAMES:
            assert np.isfinite(got).all() and np.isfinite(grad).all() and want["count"] > 0
            assert np.abs(grad).max() > 0


MAPS = [("partition", None), ("partition", "dyadic"), ("mixed", None), ("mixed", "dyadic"), ("eights", "mean")]


@pytest.mark.parametrize("kind,weights", MAPS, ids=["%s-%s" % m for m in MAPS])
def test_exact_maps(kind, weights, lib_built):
    """the base shape under every kind of map and weighting; weights "mean" over groups of 8: products on the 2^-7 grid"""
    rm = _map(kind, 257, weights)
    _check_exact(EXACT_NAMES + MAPE_NAMES, lambda name: _case_for(name, "base"), rm,
                 grid_bits=7 if weights == "mean" else RL.GRID_BITS)


@pytest.mark.parametrize("shape_name", SHAPE_IDS[1:])
def test_exact_shapes(shape_name, lib_built):
    b, out, n, od = SHAPES[shape_name][:4]
    rm = _map("mixed", n, "dyadic")
    if shape_name == "rows_one_past_a_tile":
        assert RL.rows_per_tile(b * out, n, od, rm.num_groups) == 2 and (b * out) % 2 == 1
    else:
        assert RL.rows_per_tile(b * out, n, od, rm.num_groups) == 1
    _check_exact(EXACT_NAMES + MAPE_NAMES, lambda name: _case_for(name, shape_name), rm)


def test_exact_one_group(lib_built):
    _check_exact(EXACT_NAMES, lambda name: _case_for(name, "out24"), _map("whole", 65, "dyadic"))


# G * od on both sides of REGION_Q_FLOATS (tile with R = 1 / walk), and a by-node map on both sides of REGION_MAP_FLOATS
# (staged in LDS / read from global memory; a weighted map takes two floats per membership): one- and two-member groups
SMALL = {
    "q_cap_tile": (RL.REGION_Q_FLOATS, 12000, None), "q_cap_walk": (RL.REGION_Q_FLOATS + 1, 12000, None),
    "q_cap_walk_weighted": (RL.REGION_Q_FLOATS + 1, 12000, "dyadic"),
    "map_cap_staged": (3000, RL.REGION_MAP_FLOATS, None), "map_cap_global": (3000, RL.REGION_MAP_FLOATS + 1, None),
    "map_cap_staged_weighted": (1500, RL.REGION_MAP_FLOATS // 2, "dyadic"),
    "map_cap_global_weighted": (1500, RL.REGION_MAP_FLOATS // 2 + 1, "dyadic"),
}


@pytest.mark.parametrize("which", list(SMALL))
def test_exact_across_the_caps(which, lib_built):
    n_groups, n_members, weights = SMALL[which]
    b, out, n, od = 2, 2, 65, 1
    rm = _map(("small", n_groups, n_members), n, weights)
    assert rm.num_groups == n_groups and rm.num_members == n_members
    assert (RL.rows_per_tile(b * out, n, od, n_groups) is None) == ("walk" in which)
    c = T.grid_case(77, b, out, n, od)
    nan = dict(c, y=c["y"].copy())
    nan["y"][1, 0, 9, 0] = NAN
    _check_exact(("mse", "masked_mae", "rmse", "huber", "mae"), lambda name: nan if name == "mae" else c, rm)


def test_label_start_gathers_what_the_windows_hold(lib_built):
    t_steps, out, n, od, feat, y_start = 40, 6, 65, 2, 4, 1
    rng = np.random.default_rng(31)
    series = (rng.integers(-64, 65, (t_steps, n, feat)) / 16.0).astype(F32)
    starts = np.array([0, t_steps - out, 5, 5, 7], dtype=np.int32)
    windows = np.stack([series[s:s + out] for s in starts], 0)
    pred = (windows[..., y_start:y_start + od] + rng.integers(-16, 17, (5, out, n, od)) / 16.0).astype(F32)
    cw = dict(y=windows, pred=pred, y_start=y_start, mean=-1.0, std=2.0)
    cs = dict(cw, y=series)
    rm = _map("mixed", n, "dyadic")
    for name in ("mse", "masked_rmse", "huber", "quantile", "mape"):
        RL.assert_region_exact(name, cw, rm.ptr, rm.node, rm.weight)
        want = _ref(name, cs, rm, label_start=starts)
        vw, gw = _run(name, cw, rm)
        vs, gs = _run(name, cs, rm, label_start=starts)
        assert _same(vw, vs).all() and _same(gw, gs).all(), name
        _assert_exact_values(name, vs, want)
        _assert_exact_grad(name, gs, want)


# ---- the order of a chain -------------------------------------------------------------------------------------------------
def test_chain_order_is_the_member_position(lib_built):
    """continuous data, mse, weights float32(0.3) and float32(0.7), a node in 5 groups: the gradient has the bits of the
    reference chain (ascending member position); the reversed chain gives other bits - shown on the reference first.
    A float64 chain rounded to float32 shows its order only where terms cancel, so two of the five regions hold draws
    2^30 times larger whose differences d = P - L are each other's negatives (region 3 has region 1's predictions as labels
    and its labels as predictions): next to them the small terms lose bits, and which ones depends on the order."""
    from multistgraph_amd.regions import RegionMap
    b, out, n = 3, 6, 33
    rng = np.random.default_rng(11)
    y = rng.standard_normal((b, out, n, 1)).astype(F32)
    pred = (y + 0.3 * rng.standard_normal(y.shape)).astype(F32)
    y[:, :, 11:21] *= F32(2.0 ** 30)
    pred[:, :, 11:21] *= F32(2.0 ** 30)
    y[:, :, 21:31], pred[:, :, 21:31] = pred[:, :, 11:21].copy(), y[:, :, 11:21].copy()
    pred[:, :, 7] = y[:, :, 7]
    c = dict(y=y, pred=pred, y_start=0, mean=MEAN, std=STD)
    groups = [[0, 1, 2, 7], list(range(11, 21)) + [7], [5, 7], list(range(21, 31)) + [7], [7, 6, 8, 9, 10]]
    weights = [[0.3 if (k + g) % 2 else 0.7 for k in range(len(m))] for g, m in enumerate(groups)]
    rm = RegionMap(n, groups=groups, weights=weights)
    assert np.diff(rm.by_node()[0])[7] == 5 and set(rm.weight) == {float(F32(0.3)), float(F32(0.7))}
    want = _ref("mse", c, rm, upstream=1.0)
    d = want["P"].astype(F64) - want["L"].astype(F64)
    assert np.array_equal(d[:, :, 1], -d[:, :, 3]) and np.abs(d[:, :, 1]).min() > 2.0 ** 20 * np.abs(d[:, :, [0, 2, 4]]).max()
    other = _ref("mse", c, rm, upstream=1.0, reverse=True)
    differ = want["grad32"][:, :, 7] != other["grad32"][:, :, 7]
    assert differ.sum() >= 3                                     # the order matters here (in 8 of the 18 rows)
    got, grad = _run("mse", c, rm, upstream=1.0)
    assert np.isfinite(got).all() and _bits_equal(grad, want["grad32"])


# ---- base -----------------------------------------------------------------------------------------------------------------
def test_base(lib_built):
    """base = NULL gives the region-only gradient; base aliased with d_pred and base in a buffer of its own give the same
    bits, those of the reference; a node in no group gets its base bit for bit (-0.0 and NaN included)"""
    rm = _map("partition", 257, "dyadic")
    outside = np.diff(rm.by_node()[0]) == 0
    for name in ("mse", "masked_mae", "huber", "rmse"):
        c = _case_for(name, "base")
        rng = np.random.default_rng(13)
        base = (rng.integers(-64, 65, c["pred"].shape) / 64.0).astype(F32)
        base[0, 0, 6, 0], base[1, 2, 13, 0] = -0.0, NAN                               # nodes 6 and 13: in no group
        assert outside[6] and outside[13]
        c = dict(c, base=base)
        v0, g0 = _run(name, c, rm)
        v1, g1, _ = _raw(name, c, rm, fill=NAN)
        assert _bits_equal(v0, v1) and _bits_equal(g0, g1), name
        want = _ref(name, c, rm, base=base)
        _, ga, _ = _raw(name, c, rm, base="alias")
        _, gs, _ = _raw(name, c, rm, fill=NAN, base="separate")
        assert _bits_equal(ga, gs), name
        fin = ~np.isnan(base)
        assert _bits_equal(ga[:, :, outside], base[:, :, outside]), name
        _assert_exact_grad(name, np.where(fin, ga, F32(0)), dict(grad=np.where(fin, want["grad"], 0.0)))


@pytest.mark.parametrize("name", ["mse", "huber", "masked_mae"])
def test_tract_region_loss_is_one_gradient(name, lib_built):
    """tract_region_loss(...).backward() = float32(float64(tract gradient) + region part), the value the weighted sum of
    the two device values in float32"""
    from multistgraph_amd import ops
    rm = _map("mixed", 257, "dyadic")
    c = _case_for(name, "base")
    tw, rw = 0.5, 2.0
    y, args = _dev(c["y"]), (c["y_start"], c["mean"], c["std"], name)
    p = _dev(c["pred"]).requires_grad_(True)
    loss = ops.tract_region_loss(p, y, rm, *args, tract_weight=tw, region_weight=rw)
    (loss * UPSTREAM).backward()
    vt = ops.train_loss_device(p.detach(), y, *args)[0]
    vr = ops.region_loss_device(p.detach(), y, rm, *args)[0]
    assert torch.equal(loss.detach(), vt * tw + vr * rw)
    pt = _dev(c["pred"]).requires_grad_(True)
    (ops.train_loss(pt, y, *args) * (UPSTREAM * tw)).backward()
    tract = _host(pt.grad)
    want = _ref(name, c, rm, upstream=UPSTREAM * rw, base=tract)
    _assert_exact_grad(name, _host(p.grad), want)
    assert not np.array_equal(_host(p.grad), tract)
    # a weight of 0 skips its half
    halves = ((1.0, 0.0, lambda q: ops.train_loss(q, y, *args)),
              (0.0, 1.0, lambda q: ops.region_train_loss(q, y, rm, *args)))
    for a, b, fn in halves:
        q1, q2 = _dev(c["pred"]).requires_grad_(True), _dev(c["pred"]).requires_grad_(True)
        l1, l2 = ops.tract_region_loss(q1, y, rm, *args, tract_weight=a, region_weight=b), fn(q2)
        l1.backward()
        l2.backward()
        assert torch.equal(l1.detach(), l2.detach()) and torch.equal(q1.grad, q2.grad)


# ---- masks ----------------------------------------------------------------------------------------------------------------
def test_a_nan_tract_label_masks_the_regions_that_hold_it(lib_built):
    """under mae: exactly the regions containing the tract, in that (b, horizon), drop out - value and gradient"""
    from multistgraph_amd.regions import RegionMap
    n = 40
    rm = RegionMap(n, groups=[list(range(0, 10)), list(range(10, 25)), list(range(20, 40)), [12]])
    c = T.grid_case(5, 2, 3, n, 1)
    c = dict(c, y=c["y"].copy())
    c["y"][1, 2, 22, 0] = NAN                                   # node 22: regions 1 and 2
    got, grad = _run("mae", c, rm)
    want = _ref("mae", c, rm)
    assert want["count"] == 2 * 3 * 4 - 2 and np.isnan(want["L"][1, 2, [1, 2], 0]).all()
    assert np.isnan(want["L"]).sum() == 2
    _assert_exact_values("mae", got, want)
    _assert_exact_grad("mae", grad, want)
    masked = np.zeros(grad.shape, dtype=bool)
    masked[1, 2, 10:, 0] = True                                 # the members of regions 1, 2 (and 3, inside 1)
    masked[1, 2, 12, 0] = False                                 # region 3 = [12] is still scored
    assert (grad[masked] == 0).all() and (grad[~masked] != 0).mean() > 0.9
    assert grad[1, 2, 12, 0] != 0


def test_all_masked_and_rmse_zero(lib_built):
    rm = _map("mixed", 257, "dyadic")
    c = _case_for("masked_mae", "base")
    zero = dict(c, y=np.zeros_like(c["y"]), mean=0.0, std=2.0)
    for name in ("masked_mae", "masked_mse", "masked_rmse", "masked_mape"):
        got, grad = _run(name, zero, rm)
        assert (got == 0).all() and _bits_equal(grad, np.zeros_like(grad)), name
    nan = dict(c, y=np.full_like(c["y"], NAN))
    for name in ("mae", "mse", "rmse", "mape"):
        got, grad = _run(name, nan, rm)
        assert (got == 0).all() and _bits_equal(grad, np.zeros_like(grad)), name
    same = dict(c, pred=c["y"][:, :, :, :1].copy())
    for name in ("rmse", "masked_rmse"):
        got, grad = _run(name, same, rm)
        assert (got == 0).all() and (grad == 0).all(), name     # torch: 0 / 0 = NaN


def test_min_s_acts_on_the_total(lib_built):
    """masked_mse: a region whose label TOTAL is below min_s = 1e-4 is zeroed and masked although none of its member tracts
    is; tract labels below min_s simply add to their region"""
    from multistgraph_amd.regions import RegionMap
    n = 12
    rm = RegionMap(n, groups=[[0, 1, 2, 3], [4, 5], [6, 7, 8, 9, 10, 11]])
    y = np.full((2, 3, n, 1), 2.0, dtype=F32)
    pred = np.full((2, 3, n, 1), 3.0, dtype=F32)
    y[:, :, 4, 0], y[:, :, 5, 0] = 1.5, -1.5                    # region 1: labels far from 0, total 0
    y[0, 0, 6, 0] = 5e-5                                        # below min_s as a tract: its region's total is 10.00005
    c = dict(y=y, pred=pred, y_start=0, mean=0.0, std=1.0)
    got, grad = _run("masked_mse", c, rm)
    want = _ref("masked_mse", c, rm)
    assert want["count"] == 2 * 3 * 2
    assert np.allclose(got, want["values"], rtol=2e-7)          # one float32 total is rounded (10.00005), one result
    assert (grad[:, :, 4:6] == 0).all() and (grad[:, :, :4] > 0).all() and (grad[:, :, 6:] > 0).all()
    assert max_norm_err(grad, want["grad"]) <= 2e-7
    tract = _dev(pred).requires_grad_(True)
    from multistgraph_amd import ops
    ops.train_loss(tract, _dev(y), 0, 0.0, 1.0, "masked_mse").backward()
    assert (_host(tract.grad)[:, :, 4:6] != 0).all()            # the member tracts themselves are not masked


# ---- run to run, dirty buffers --------------------------------------------------------------------------------------------
def _realistic_case(seed, b, out, n, zeros, mean=MEAN, std=STD):
    rng = np.random.default_rng(seed)
    y = rng.standard_normal((b, out, n, 1)).astype(F32)
    pred = (y + 0.3 * rng.standard_normal((b, out, n, 1))).astype(F32)
    if zeros:
        y[0, :, :3, 0] = F32(-mean / std)
        y[1, 2, 5, 0] = F32((5e-5 - mean) / std)
        pred[1, 3, 7, 0] = y[1, 3, 7, 0]
    return dict(y=y, pred=pred, y_start=0, mean=mean, std=std)


def test_run_to_run_and_dirty_buffers(lib_built):
    """two calls give equal bits (continuous data, every name), and neither NaN nor another finite filling of the caller's
    scratch, result and gradient buffers reaches a result; everything finite stays finite"""
    rm = _map("mixed", 301, "continuous")
    for name in ELEVEN:
        c = _realistic_case(3, 5, 7, 301, name not in ZERO_FREE)
        v1, g1 = _run(name, c, rm)
        v2, g2 = _run(name, c, rm)
        assert _bits_equal(v1, v2) and _bits_equal(g1, g2), name
        rv, rg, rs = _raw(name, c, rm, fill=NAN)
        assert _bits_equal(rv, v1) and _bits_equal(rg, g1), name
        tot = 2 * 5 * 7 * rm.num_groups                          # the float32 totals, then doubles, then the affine pair
        assert np.isfinite(rv).all() and np.isfinite(rg).all(), name
        assert np.isfinite(rs.view(F32)[:tot]).all() and np.isfinite(rs[tot // 2:-1]).all(), name
        assert np.array_equal(rs[-1:].view(F32), np.array([MEAN, STD], dtype=F32)), name
        rv, rg, _ = _raw(name, c, rm, fill=7.5)
        assert _bits_equal(rv, v1) and _bits_equal(rg, g1), name


# ---- REALISTIC ------------------------------------------------------------------------------------------------------------
def _bar(gap):
    return max(2.0 * gap, FLOOR) if np.isfinite(gap) else FLOOR


@functools.lru_cache(maxsize=None)
def _city_map(weights):
    from multistgraph_amd.regions import RegionMap
    n = 403
    labels = np.random.default_rng(403).integers(0, 10, n)
    groups = [np.flatnonzero(labels == g).tolist() for g in range(10)] + [list(range(n))]
    return RegionMap(n, groups=groups, weights=_weights(groups, weights))


def _torch_route(name, c, rm, dtype):
    """value, horizons and d value / d pred of the torch statement in ``dtype`` on the CPU: de-scaled float32 values, dense
    membership matmul, train_loss_ref.torch_loss, autograd"""
    m = torch.tensor(RL.dense_membership(rm.ptr, rm.node, rm.weight, rm.num_nodes), dtype=dtype)
    p0 = torch.tensor(c["pred"], requires_grad=True)
    p = (p0 * F32(c["std"]) + F32(c["mean"])).to(dtype)
    l = (torch.tensor(c["y"]) * F32(c["std"]) + F32(c["mean"])).to(dtype)
    P, L = torch.einsum("gn,bonc->bogc", m, p), torch.einsum("gn,bonc->bogc", m, l)
    v = T.torch_loss(name, P, L)
    v.backward()
    with torch.no_grad():
        h = [float(T.torch_loss(name, P[:, k:k + 1], L[:, k:k + 1])) for k in range(P.shape[1])]
    return float(v.detach()), np.array(h), p0.grad.numpy().astype(F64)


@pytest.mark.parametrize("name", ELEVEN)
def test_realistic(name, lib_built):
    scaler = dict(mean=0.5, std=1.0) if name == "logcosh" else {}
    c = _realistic_case(41, 5, 24, 403, name not in ZERO_FREE, **scaler)
    rm = _city_map("continuous")
    v32, h32, g32 = _torch_route(name, c, rm, torch.float32)
    if name == "logcosh":
        assert np.isfinite(v32)                                  # the yardstick is a number (module docstring)
    # the float64 reference from the same float32 de-scaled values; its gradient is taken by them: times std for d / d pred
    pd = np.asarray(c["pred"] * F32(c["std"]), dtype=F32) + F32(c["mean"])
    ld = np.asarray(c["y"] * F32(c["std"]), dtype=F32) + F32(c["mean"])
    want = RL.region_loss_ref(name, pd, ld, 0, 0.0, 1.0, rm.ptr, rm.node, rm.weight, upstream=1.0, dtype=F64)
    v64, h64, g64 = want["value"], want["values"][1:], want["grad"] * float(F32(c["std"]))
    t64 = _torch_route(name, c, rm, torch.float64)                # the torch statement in float64 agrees with it
    assert abs(t64[0] - v64) <= 1e-6 * abs(v64) and np.abs(t64[2] - g64).max() <= 1e-6 * np.abs(g64).max()
    got, grad = _run(name, c, rm, upstream=1.0)
    gmax = np.abs(g64).max()
    gap_v, gap_h = abs(v32 - v64) / abs(v64), np.abs(h32 - h64) / np.abs(h64)
    gap_g = float(np.abs(g32 - g64).max() / gmax)
    err_v = abs(float(got[0]) - v64) / abs(v64)
    err_h = np.abs(got[1:].astype(F64) - h64) / np.abs(h64)
    err_g = float(np.abs(grad.astype(F64) - g64).max() / gmax)
    print("REGION-LOSS-GAP %-11s value: torch32 gap %.3g ours %.3g | horizons: worst gap %.3g ours %.3g | gradient: "
          "torch32 gap %.3g ours %.3g" % (name, gap_v, err_v, gap_h.max(), err_h.max(), gap_g, err_g))
    assert np.isfinite(got).all() and np.isfinite(grad).all()
    assert err_v <= _bar(gap_v), (name, err_v, gap_v)
    # A horizon's error - ours and the float32 torch run's alike - is dominated by the float32 rounding of its 5 x 11 totals:
    # one draw from the same distribution for every horizon, and a single draw of the yardstick can fall near 0 by chance
    # (it does for some horizon of mae and mse).  So the worst of the 24 float32 draws is the yardstick of each horizon.
    assert (err_h <= _bar(gap_h.max())).all(), (name, err_h, gap_h)
    assert err_g <= _bar(gap_g), (name, err_g, gap_g)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def _model(c, **extra):
    from multistgraph_amd import synthetic as syn
    from multistgraph_amd.model import MultiATGCN
    dev = torch.device("cuda:0")
    cfg = dict(c.config("cuda:0"), hip_deterministic=True, **extra)
    m = MultiATGCN(cfg, dict(c.data_feature, scaler=syn.PlainScaler(MEAN, STD))).to(dev).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    return m, dev


def _grads(m):
    return {k: (p.grad.clone() if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}


def _labels_with_zeros(c):
    y = torch.from_numpy(c.y).clone()
    y[0, :, :3, 0] = -MEAN / STD
    return y


def _three_regions(n):
    return [k % 3 for k in range(n)]


@pytest.mark.parametrize("name", ["huber", "masked_mse"])
def test_calculate_loss_trains_on_tracts_and_regions(name, lib_built):
    """hip_region_loss_weight = 0.5, a 3-region map: calculate_loss(batch).backward() against the same model's HIP
    prediction pushed through tw * torch_loss(p, l) + rw * torch_loss(M p, M l) by autograd; the suite's 1e-4"""
    from multistgraph_amd.regions import RegionMap
    c = Case("tiny_multi_uni_c2")
    tw, rw = 1.0, 0.5
    m, dev = _model(c, hip_train_loss=name, hip_train_regions=_three_regions(c.n), hip_region_loss_weight=rw)
    rm = RegionMap(c.n, labels=_three_regions(c.n))
    y = _labels_with_zeros(c)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": y.to(dev)}
    loss = m.calculate_loss(batch)
    assert loss.requires_grad
    loss.backward()
    got = _grads(m)
    m.zero_grad(set_to_none=True)
    sc = m._scaler
    mem = torch.tensor(RL.dense_membership(rm.ptr, rm.node, rm.weight, c.n), dtype=torch.float32, device=dev)
    p, l = sc.inverse_transform(m.predict(batch)), sc.inverse_transform(batch["y"][..., 0:1])
    want_loss = tw * T.torch_loss(name, p, l) + rw * T.torch_loss(name, torch.einsum("gn,bonc->bogc", mem, p),
                                                                  torch.einsum("gn,bonc->bogc", mem, l))
    want_loss.backward()
    want = _grads(m)
    assert abs(float(loss.detach()) - float(want_loss.detach())) <= 1e-4 * abs(float(want_loss.detach()))
    bad = {k: max_norm_err(_host(got[k]), _host(want[k])) for k in want
           if float(want[k].abs().max()) > 0 and max_norm_err(_host(got[k]), _host(want[k])) > 1e-4}
    assert not bad, bad
    assert all(float(got[k].abs().max()) <= 1e-6 for k in want if float(want[k].abs().max()) == 0)
    with torch.no_grad():
        assert torch.equal(m.calculate_loss(batch), loss.detach())
        assert torch.equal(m.train_loss(batch, name, regions=rm, region_weight=rw), loss.detach())
        assert not torch.equal(m.train_loss(batch, name), loss.detach())
    # hip_deterministic: a second training step gives the same bits
    m.zero_grad(set_to_none=True)
    again = m.calculate_loss(batch)
    again.backward()
    g2 = _grads(m)
    assert torch.equal(again.detach(), loss.detach()) and all(torch.equal(got[k], g2[k]) for k in got)


@pytest.mark.parametrize("name", ["huber", "masked_mse"])
def test_resident_series_batch_gives_the_window_batch_bits(name, lib_built):
    from multistgraph_amd import windows as W
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_train_loss=name, hip_train_regions=_three_regions(c.n), hip_region_loss_weight=0.5)
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 40
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, c.feat)).astype(F32)
    series[rng.random(series.shape) < 0.02] = F32(-MEAN / STD)
    starts = W.valid_label_starts(steps, rel, 24)
    pick = starts[rng.permutation(len(starts))[:c.b]].astype(np.int32)
    pick[-1] = starts[-1]
    x, y = W.gather_windows(series, pick, rel, c.out)
    win = {"X": torch.from_numpy(x).to(dev), "y": torch.from_numpy(y).to(dev)}
    res = {"series": torch.from_numpy(series).to(dev), "label_start": torch.from_numpy(pick).to(dev), "rel_steps": rel}
    with torch.no_grad():
        a, b = m.calculate_loss(win), m.calculate_loss(res)
        assert torch.equal(a, b) and torch.isfinite(a)
    la = m.calculate_loss(win)
    la.backward()
    ga = _grads(m)
    m.zero_grad(set_to_none=True)
    lb = m.calculate_loss(res)
    lb.backward()
    gb = _grads(m)
    assert torch.equal(la.detach(), lb.detach()) and torch.equal(la.detach(), a)
    bad = {k: max_norm_err(_host(gb[k]), _host(ga[k])) for k in ga
           if float(ga[k].abs().max()) > 0 and max_norm_err(_host(gb[k]), _host(ga[k])) > 1e-4}
    assert not bad, bad


def test_without_the_keys_calculate_loss_is_what_it_was(lib_built):
    """no key, a map with weight 0, and a map with the default weight: loss and gradients bit for bit today's default"""
    c = Case("tiny_multi_uni_c2")
    y = _labels_with_zeros(c)
    out = []
    for extra in ({}, dict(hip_train_regions=_three_regions(c.n), hip_region_loss_weight=0.0),
                  dict(hip_train_regions=_three_regions(c.n)),
                  dict(hip_train_regions=_three_regions(c.n), hip_region_loss_weight=0.5)):
        m, dev = _model(c, **extra)
        batch = {"X": torch.from_numpy(c.x).to(dev), "y": y.to(dev)}
        loss = m.calculate_loss(batch)
        loss.backward()
        out.append((loss.detach().clone(), _grads(m)))
    (l0, g0), (l1, g1), (l2, g2), (l3, g3) = out
    assert torch.equal(l0, l1) and all(torch.equal(g0[k], g1[k]) for k in g0)
    assert torch.equal(l0, l2) and all(torch.equal(g0[k], g2[k]) for k in g0)
    assert any(float(g0[k].abs().max()) > 0 for k in g0)
    assert not torch.equal(l0, l3)                              # "none" with a region weight: masked_mae on both levels


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals(lib_built):
    from multistgraph_amd import _lib, ops
    from multistgraph_amd.regions import RegionMap
    c = _case_for("mse", "out1")
    rm = _map("mixed", 65, None)
    pred, y = _dev(c["pred"]), _dev(c["y"])
    args = (c["y_start"], c["mean"], c["std"], "mse")
    with pytest.raises(_lib.MatgcnError, match="GPU"):
        ops.region_loss_device(pred.cpu(), y, rm, *args)
    with pytest.raises(_lib.MatgcnError, match="GPU"):
        ops.region_loss_device(pred, y.cpu(), rm, *args)
    with pytest.raises(_lib.MatgcnError, match="nodes"):
        ops.region_loss_device(pred, y, _map("mixed", 64, None), *args)
    with pytest.raises(_lib.MatgcnError, match="status -2"):     # a by_node map of another member count: BAD_ARG
        _raw("mse", c, rm, by_node=RegionMap(65, groups=[[0, 1]]))
    with pytest.raises(_lib.MatgcnError, match="status -4"):     # a short scratch: SMALL_BUFFER
        _raw("mse", c, rm, short=1)
    with pytest.raises(ValueError, match="delta"):
        ops.region_loss_device(pred, y, rm, c["y_start"], c["mean"], c["std"], "quantile", 1.5)
    case = Case("tiny_multi_uni_c2")
    m, dev = _model(case, hip_train_loss="huber", hip_train_regions=_three_regions(case.n), hip_region_loss_weight=0.5)

    class Cubic:
        def inverse_transform(self, d):
            return d * d * d
    m._scaler = Cubic()
    batch = {"X": torch.from_numpy(case.x).to(dev), "y": torch.from_numpy(case.y).to(dev)}
    with torch.no_grad():
        with pytest.raises(NotImplementedError):
            m.calculate_loss(batch)
        with pytest.raises(NotImplementedError):
            m.train_loss(batch, "mse", regions=_three_regions(case.n))
