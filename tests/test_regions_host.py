"""Region totals on the host (matgcn_group_sums, matgcn_group_label_sums; include/matgcn.h): symbols, header and binding,
every refusal - all are made before a launch, so dummy device pointers do -, regions.RegionMap, and the numpy reference
(regions_ref.py) held to what makes the GPU tests mean something: the order of a chain changes its bits, and a chain of
one member is the member."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import node_metrics_ref as R
import regions_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_group_sums", "matgcn_group_label_sums")
OK, ERR_NULL, ERR_BAD_ARG, ERR_UNSUPPORTED = 0, -1, -2, -3
PTR = C.c_void_p(4096)     # a non-NULL pointer nothing dereferences: every call below fails before its launch
NAN = float("nan")


def _lib():
    from multistgraph_amd import _lib
    return _lib


def _scale(lone=False):
    sc = _lib().MetricScale()
    sc.mean, sc.std, sc.mean2, sc.std2, sc.per_node = (4096 if lone else None), None, None, None, 0
    sc.clamp_min, sc.truth_min, sc.min_s = NAN, NAN, -1.0
    return sc


def _groups(ptr=(0, 2, 2, 5), n_groups=None, n_members=None, null_ptr=False, null_dev=False, null_node=False):
    """(descriptor, the host array it points to): ptr is read on the host, the device pointers are dummies"""
    host = (C.c_int32 * len(ptr))(*ptr)
    g = _lib().Groups()
    g.ptr = None if null_ptr else C.cast(host, C.POINTER(C.c_int32))
    g.ptr_dev = None if null_dev else 4096
    g.node = None if null_node else 4096
    g.weight = None
    g.n_groups = len(ptr) - 1 if n_groups is None else n_groups
    g.n_members = ptr[-1] if n_members is None else n_members
    return g, host


def _sums(lib, values=PTR, rows=6, nodes=5, od=2, scale="id", groups="default", out=PTR, **map_kw):
    sc = _scale(lone=scale == "lone")
    g, keep = _groups(**map_kw)
    status = lib.matgcn_group_sums(values, rows, nodes, od, None if scale is None else C.byref(sc),
                                   None if groups is None else C.byref(g), out, None)
    del keep
    return status


def _label_sums(lib, y=PTR, b=2, out_steps=3, nodes=5, od=2, y_steps=3, y_feat=2, y_start=0, scale="id", groups="default",
                out=PTR, **map_kw):
    sc = _scale(lone=scale == "lone")
    g, keep = _groups(**map_kw)
    status = lib.matgcn_group_label_sums(y, None, b, out_steps, nodes, od, y_steps, y_feat, y_start,
                                         None if scale is None else C.byref(sc), None if groups is None else C.byref(g),
                                         out, None)
    del keep
    return status


def test_library_exports_and_binding(lib_built):
    from multistgraph_amd import evaluator, ops, regions
    from multistgraph_amd.model import MultiATGCN
    _l = _lib()
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    lib = _l.load()
    for name in NEW_FUNCTIONS:
        assert name in _l.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "} matgcn_groups;" in header
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12 == _l.ABI_VERSION
    assert [f[0] for f in _l.Groups._fields_] == ["ptr", "ptr_dev", "node", "weight", "n_groups", "n_members"]
    assert C.sizeof(_l.Groups) == 4 * C.sizeof(C.c_void_p) + 8
    for fn in (ops.group_sums, ops.group_label_sums, regions.RegionMap, evaluator.RegionEvaluator,
               MultiATGCN.predict_regions, MultiATGCN.collect_region_metrics, MultiATGCN.score_mc_regions):
        assert callable(fn)
    from multistgraph_amd import build
    assert "matgcn_regions.hip" in build.DEPS


def test_group_sums_arguments_are_checked_on_the_host(lib_built):
    lib = _lib().load()
    for name in ("values", "out", "scale", "groups"):
        assert _sums(lib, **{name: None}) == ERR_NULL, name
    for name in ("null_ptr", "null_dev", "null_node"):
        assert _sums(lib, **{name: True}) == ERR_NULL, name
    assert _sums(lib, scale="lone") == ERR_BAD_ARG                                   # a mean without its std
    for bad in (dict(rows=0), dict(rows=-3), dict(nodes=0), dict(nodes=-1), dict(od=0), dict(od=-2)):
        assert _sums(lib, **bad) == ERR_BAD_ARG, bad
    for bad in (dict(n_groups=0), dict(n_groups=-1), dict(n_members=-1),
                dict(ptr=(1, 2, 2, 5)),                                             # does not start at 0
                dict(ptr=(0, 3, 2, 5)),                                             # decreasing
                dict(ptr=(0, 2, 2, 5), n_members=4), dict(ptr=(0, 2, 2, 5), n_members=6)):   # the wrong end
        assert _sums(lib, **bad) == ERR_BAD_ARG, bad
    # rows * nodes * out_dim, then rows * n_groups * out_dim, leave int64
    assert _sums(lib, rows=2 ** 62, nodes=2 ** 20, od=2) == ERR_BAD_ARG
    assert _sums(lib, rows=2 ** 61, nodes=1, od=1, ptr=(0,) * 5) == ERR_BAD_ARG
    # a row no 32-bit index holds
    assert _sums(lib, rows=1, nodes=2 ** 30, od=2) == ERR_UNSUPPORTED
    assert _sums(lib, rows=1, nodes=2 ** 30, od=4) == ERR_UNSUPPORTED


def test_group_label_sums_arguments_are_checked_on_the_host(lib_built):
    lib = _lib().load()
    for name in ("y", "out", "scale", "groups"):
        assert _label_sums(lib, **{name: None}) == ERR_NULL, name
    for name in ("null_ptr", "null_dev", "null_node"):
        assert _label_sums(lib, **{name: True}) == ERR_NULL, name
    assert _label_sums(lib, scale="lone") == ERR_BAD_ARG
    for bad in (dict(b=0), dict(b=-1), dict(out_steps=0), dict(out_steps=-2), dict(nodes=0), dict(od=0), dict(y_steps=2),
                dict(y_steps=0), dict(y_feat=0), dict(y_start=-1), dict(y_start=1), dict(od=3)):
        assert _label_sums(lib, **bad) == ERR_BAD_ARG, bad
    for bad in (dict(n_groups=0), dict(n_members=-1), dict(ptr=(1, 2, 2, 5)), dict(ptr=(0, 3, 2, 5)),
                dict(ptr=(0, 2, 2, 5), n_members=4)):
        assert _label_sums(lib, **bad) == ERR_BAD_ARG, bad
    # batch * out_steps * nodes * out_dim leaves int64
    assert _label_sums(lib, b=2 ** 31 - 1, out_steps=2 ** 31 - 1, nodes=2 ** 20, od=2, y_steps=2 ** 31 - 1) == ERR_BAD_ARG
    assert _label_sums(lib, nodes=2 ** 30, od=2) == ERR_UNSUPPORTED


def test_an_empty_map_needs_no_member_arrays(lib_built):
    """n_members = 0 with a null node pointer passes every check but the one after it (a zero row count here)"""
    lib = _lib().load()
    assert _sums(lib, ptr=(0, 0, 0), null_node=True, rows=0) == ERR_BAD_ARG
    assert _sums(lib, ptr=(0, 0, 0), null_node=True, values=None) == ERR_NULL


# ---- RegionMap ------------------------------------------------------------------------------------------------------------
def test_region_map_construction_and_refusals():
    from multistgraph_amd.regions import RegionMap
    rm = RegionMap(7, groups=[[4, 1], [], [0, 1, 2, 3, 4, 5, 6], [6]], names=["a", "b", "all", "d"])
    assert (rm.num_nodes, rm.num_groups, rm.num_members, len(rm)) == (7, 4, 10, 4)
    assert rm.ptr == [0, 2, 2, 9, 10] and rm.node == [4, 1, 0, 1, 2, 3, 4, 5, 6, 6] and rm.weight is None
    assert rm.members(0) == [4, 1] and rm.members(1) == [] and rm.weights_of(0) is None
    for bad in (dict(groups=[[0, 7]]), dict(groups=[[-1]]), dict(groups=[]), dict(),
                dict(groups=[[0]], labels=[0] * 7), dict(labels=[0] * 6), dict(labels=[-1] * 7),
                dict(groups=[[0, 1]], weights=[[1.0]]), dict(groups=[[0, 1]], weights=[[1.0, 2.0], [1.0]]),
                dict(groups=[[0, 1]], weights=[[1.0, NAN]]), dict(groups=[[0, 1]], weights=[[1.0, float("inf")]]),
                dict(groups=[[0, 1]], weights=[[1.0, 1e39]]),       # infinite as a float32
                dict(groups=[[0, 1]], weights="median"), dict(groups=[[0]], names=["a", "b"]),
                dict(labels=[0] * 7, weights=[1.0] * 6)):
        with pytest.raises(ValueError):
            RegionMap(7, **bad)
    with pytest.raises(ValueError):
        RegionMap(0, groups=[[]])
    # a partition from labels is the same map as its index lists, members ascending, negative labels in no region
    labels = [2, 0, -1, 0, 2, 2, -5]
    by_label = RegionMap(7, labels=labels)
    by_list = RegionMap(7, groups=[[1, 3], [], [0, 4, 5]])
    assert by_label == by_list and by_label.ptr == [0, 2, 2, 5] and by_label.node == [1, 3, 0, 4, 5]
    assert by_label != RegionMap(7, groups=[[3, 1], [], [0, 4, 5]])           # the order of the members is part of the map
    assert by_label != RegionMap(8, groups=[[1, 3], [], [0, 4, 5]])
    # weights: per node with labels, per member with groups, "mean", rounded to float32 as the device holds them
    w = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7]
    weighted = RegionMap(7, labels=labels, weights=w)
    assert weighted == RegionMap(7, groups=[[1, 3], [], [0, 4, 5]], weights=[[0.2, 0.4], [], [0.1, 0.5, 0.6]])
    assert weighted.weight == [float(np.float32(v)) for v in (0.2, 0.4, 0.1, 0.5, 0.6)] and weighted != by_label
    mean = RegionMap(7, labels=labels, weights="mean")
    assert mean.weight == [0.5, 0.5] + [float(np.float32(1.0 / 3.0))] * 3
    assert RegionMap.singletons(4) == RegionMap(4, groups=[[0], [1], [2], [3]])
    assert RegionMap.total(3) == RegionMap(3, groups=[[0, 1, 2]]) and RegionMap.total(3).names == ["total"]
    # the device side is HIP only
    with pytest.raises(Exception):
        rm.groups_on("cpu")


def test_region_map_state_round_trip():
    import json
    from multistgraph_amd.regions import RegionMap
    rm = RegionMap(7, groups=[[4, 1], [], [0, 1, 2, 3, 4, 5, 6], [6]], weights=[[0.1, 3.0], [], [1.0] * 7, [-2.5]],
                   names=["a", "b", "all", "d"])
    state = rm.state_dict()
    assert all(isinstance(state[k], list) for k in ("ptr", "node", "weight", "names")) and state["num_nodes"] == 7
    again = RegionMap.from_state_dict(json.loads(json.dumps(state)))
    assert again == rm and again.names == rm.names and again.state_dict() == state
    other = RegionMap.total(2)
    assert other.load_state_dict(state) is other and other == rm and other.num_groups == 4
    plain = RegionMap(3, labels=[0, 1, 0])
    assert RegionMap.from_state_dict(plain.state_dict()) == plain and plain.state_dict()["weight"] is None
    for broken in (dict(state, ptr=[0, 2, 2, 9]), dict(state, ptr=[1, 2, 2, 9, 10]), dict(state, ptr=[0, 3, 2, 9, 10]),
                   dict(state, weight=[1.0]), dict(state, node=[9] * 10)):
        with pytest.raises(ValueError):
            RegionMap.from_state_dict(broken)


def test_calibrator_carries_and_compares_the_map(lib_built):
    from multistgraph_amd.evaluator import ConformalCalibrator
    from multistgraph_amd.regions import RegionMap
    rm, other = RegionMap(5, labels=[0, 0, 1, 1, 1]), RegionMap(5, labels=[0, 1, 1, 1, 1])
    cal = ConformalCalibrator({}, regions=rm, grouping="element")
    cal.margin = torch.zeros(2, 2, 1)
    cal.count = torch.ones(2, 2, 1, dtype=torch.int32)
    cal.affine = (1.0, 2.0)
    call = ((0.05, 0.5, 0.95), (1.0, 2.0), None, None, None)
    cal.check_call(*call, rm)
    cal.check_call(*call, RegionMap(5, groups=[[0, 1], [2, 3, 4]]))          # an equal map, not the same object
    for bad in (other, None, RegionMap(5, groups=[[1, 0], [2, 3, 4]])):
        with pytest.raises(ValueError):
            cal.check_call(*call, bad)
    loaded = ConformalCalibrator({})
    loaded.load_state_dict(cal.state_dict())
    assert loaded.regions == rm and loaded.state_dict()["regions"] == rm.state_dict()
    loaded.check_call(*call, rm)
    node_level = ConformalCalibrator({})
    node_level.margin, node_level.affine = torch.zeros(2), (1.0, 2.0)
    node_level.check_call(*call)
    with pytest.raises(ValueError):
        node_level.check_call(*call, rm)
    assert node_level.state_dict()["regions"] is None


# ---- the reference ----------------------------------------------------------------------------------------------------------
def test_the_order_of_a_chain_changes_its_bits():
    """Members (1, 2^60, -2^60), identity scale, weights 1.  In listed order the 1 is absorbed by 2^60 (half an ulp of
    2^60 in float64 is 2^7) and the total is 0; added last - descending magnitude - or in a pairwise tree, 1 + (2^60 - 2^60),
    it survives.  (Ascending magnitude IS the listed order for these values.)  So equality with the reference's bits on
    the GPU rules out a reordered sum."""
    x = np.array([[1.0], [2.0 ** 60], [-2.0 ** 60]], dtype=np.float32)       # (N = 3, od = 1)
    listed = G.group_sums(x, [0, 3], [0, 1, 2])
    assert listed.shape == (1, 1) and listed.dtype == np.float32 and listed[0, 0] == 0.0
    descending = G.chain(x, [0, 1, 2], order=[1, 2, 0])
    tree = G.pairwise(x[:, 0])
    assert descending[0] == 1.0 and tree == 1.0
    assert listed[0, 0] != descending[0] and listed[0, 0] != tree
    # the same members listed the other way round give the other bits: the map's order is the contract
    assert G.group_sums(x, [0, 3], [1, 2, 0])[0, 0] == 1.0
    # float64 matters too: in float32 arithmetic 2^24 + 1 + 1 stays 2^24
    y = np.array([[2.0 ** 24], [1.0], [1.0]], dtype=np.float32)
    assert G.group_sums(y, [0, 3], [0, 1, 2])[0, 0] == np.float32(2.0 ** 24 + 2.0)


def test_reference_on_singletons_is_descale_and_clamp():
    rng = np.random.default_rng(0)
    n, od = 21, 2
    x = (rng.standard_normal((3, 5, n, od)) * 4).astype(np.float32)
    x[0, 0, 3, 1] = NAN
    x[1, 2, 4, 0] = -0.0
    kw = dict(mean=rng.uniform(-2, 2, n).astype(np.float32), std=rng.uniform(0.5, 4, n).astype(np.float32),
              group_mean=rng.uniform(-1, 1, n).astype(np.float32), group_std=rng.uniform(0.5, 2, n).astype(np.float32))
    want = R.descale_nodes(x, **kw).copy()
    with np.errstate(invalid="ignore"):
        want[want < 0] = 0.0
    got = G.group_sums(x, list(range(n + 1)), list(range(n)), clamp_min=0.0, **kw)
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got.view(np.int32), want.view(np.int32)) and np.isnan(got[0, 0, 3, 1]) and (want == 0).any()
    # without any scale a chain of one member is the member (+0.0 for a member of -0.0: the chain starts from +0.0)
    plain = G.group_sums(x, list(range(n + 1)), list(range(n)))
    assert np.array_equal((x + np.float32(0.0)).view(np.int32), plain.view(np.int32))
    # an empty group is +0.0, a NaN member makes exactly its groups NaN, weights multiply in float64
    z = G.group_sums(x, [0, 0, 2, 4], [3, 5, 6, 7], weight=[0.1, 0.3, 1.0, 1.0])
    assert np.array_equal(z[..., 0, :].view(np.int32), np.zeros_like(z[..., 0, :]).view(np.int32))
    assert np.isnan(z[0, 0, 1, 1]) and np.isnan(z).sum() == 1
    one = np.float64(np.float32(0.1)) * np.float64(x[2, 2, 3, 0]) + np.float64(np.float32(0.3)) * np.float64(x[2, 2, 5, 0])
    assert z[2, 2, 1, 0] == np.float32(one)
    # labels: window geometry against series geometry
    series = rng.standard_normal((30, n, 3)).astype(np.float32)
    starts = np.array([0, 11, 26])
    windows = np.stack([series[t:t + 4] for t in starts], 0)
    a = G.group_label_sums(windows, [0, 3], [2, 0, 1], None, 3, 2, y_start=1)
    b = G.group_label_sums(series, [0, 3], [2, 0, 1], None, 3, 2, y_start=1, label_start=starts)
    assert a.shape == (3, 3, 1, 2) and np.array_equal(a.view(np.int32), b.view(np.int32))
