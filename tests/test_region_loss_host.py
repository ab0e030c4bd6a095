"""The region-level training loss on the host (matgcn_region_loss_bytes, matgcn_region_loss, matgcn_region_loss_grad;
include/matgcn.h): the transposed map of regions.RegionMap against brute force, the constructor's validation of the three
config keys, the numpy reference (region_loss_ref.py) against central differences of its own value - the reference is
checked before the kernel is held to it (tests/test_region_loss.py) -, symbols, header and binding, and every refusal of
the entry points that is made before a launch, so dummy pointers do.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import region_loss_ref as RL
from helpers import Case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_region_loss_bytes", "matgcn_region_loss", "matgcn_region_loss_grad")
OK, ERR_NULL, ERR_BAD_ARG, ERR_UNSUPPORTED, ERR_SMALL_BUFFER = 0, -1, -2, -3, -4
PTR = C.c_void_p(4096)     # a non-NULL, 8-byte aligned pointer nothing dereferences: every call below fails before its launch
NAN, INF = float("nan"), float("inf")
F32, F64 = np.float32, np.float64


def _lib():
    from multistgraph_amd import _lib
    return _lib


def _maps():
    from multistgraph_amd.regions import RegionMap
    rng = np.random.default_rng(5)
    overlapping = [[], list(range(12)), [3, 1, 2], [2, 3], [11, 0, 11], [], [3]]        # 11 twice in one group; 3 in 4
    w = [rng.choice([1.0, 0.5, 2.0], len(g)).tolist() for g in overlapping]
    return {
        "partition_with_a_node_left_out": RegionMap(7, labels=[0, 2, 2, -1, 0, 1, 2]),
        "overlapping": RegionMap(13, groups=overlapping),                               # node 12 in no group
        "overlapping_weighted": RegionMap(13, groups=overlapping, weights=w),
        "mean": RegionMap(9, groups=[[8, 7, 6, 5], [0, 1], [4]], weights="mean"),
        "descending": RegionMap(5, groups=[[4, 3, 2, 1, 0], [4, 0]], weights=[[1, 2, 3, 4, 5], [6, 7]]),
        "one_empty_group": RegionMap(3, groups=[[]]),
    }


# ---- the transposed map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(_maps()))
def test_transposed_map_against_brute_force(kind):
    rm = _maps()[kind]
    nptr, ngroup, nweight = rm.by_node()
    assert (nptr, ngroup, nweight) == RL.transpose_brute(rm.ptr, rm.node, rm.weight, rm.num_nodes)
    assert len(nptr) == rm.num_nodes + 1 and nptr[0] == 0 and nptr[-1] == rm.num_members == len(ngroup)
    # round trip: transposing once more gives the by-group map back, members of a group in ascending NODE order
    back = RL.transpose_brute(nptr, ngroup, nweight, rm.num_groups)
    assert back[0] == rm.ptr
    for g in range(rm.num_groups):
        got = list(zip(back[1][back[0][g]:back[0][g + 1]], (back[2] or rm.node)[back[0][g]:back[0][g + 1]]))
        want = sorted(zip(rm.members(g), rm.weights_of(g) or rm.members(g)), key=lambda t: t[0])
        assert [n for n, _ in got] == [n for n, _ in want]
        if rm.weight is not None:
            assert sorted(got) == sorted(want)
    assert rm.by_node()[0] is nptr                                   # derived once
    assert "by_node" not in rm.state_dict() and set(rm.state_dict()) == {"num_nodes", "ptr", "node", "weight", "names"}


def test_transposed_map_keeps_member_position():
    """a node's memberships stay in ascending member position of the by-group map - also where the group indices then
    descend, and for a node listed twice in one group (its two weights in listed order)"""
    from multistgraph_amd.regions import RegionMap
    rm = RegionMap(4, groups=[[2, 0], [0, 2, 0], [2]], weights=[[10, 11], [12, 13, 14], [15]])
    nptr, ngroup, nweight = rm.by_node()
    assert nptr == [0, 3, 3, 6, 6]                                   # nodes 1 and 3 in no group
    assert ngroup == [0, 1, 1, 0, 1, 2] and nweight == [11.0, 12.0, 14.0, 10.0, 13.0, 15.0]
    rm2 = RegionMap(3, groups=[[1], [], [1], [1]])                    # member positions 0, 1, 2 -> groups 0, 2, 3
    assert rm2.by_node() == ([0, 0, 3, 3], [0, 2, 3], None)
    rm2.load_state_dict(RegionMap(3, groups=[[0]]).state_dict())     # a reloaded map derives its transpose anew
    assert rm2.by_node() == ([0, 1, 1, 1], [0], None)


# ---- config ---------------------------------------------------------------------------------------------------------------
def test_constructor_validates_the_region_keys():
    from multistgraph_amd.model import MultiATGCN
    from multistgraph_amd.regions import RegionMap
    c = Case("tiny_multi_uni_c2")
    m = MultiATGCN(c.config(), c.data_feature)
    assert m.hip_train_regions is None and m.hip_region_loss_weight == 0.0 and m.hip_tract_loss_weight == 1.0
    keys = set(m.state_dict())
    labels = [n % 3 for n in range(c.n)]
    rm = RegionMap(c.n, labels=labels)
    for regions in (rm, rm.state_dict(), labels, np.asarray(labels)):
        mm = MultiATGCN(dict(c.config(), hip_train_regions=regions, hip_region_loss_weight=0.5,
                             hip_tract_loss_weight=2), c.data_feature)
        assert mm.hip_train_regions == rm and mm.hip_region_loss_weight == 0.5 and mm.hip_tract_loss_weight == 2.0
        assert set(mm.state_dict()) == keys                          # attributes: checkpoints unchanged
    assert MultiATGCN(dict(c.config(), hip_train_regions=rm), c.data_feature).hip_region_loss_weight == 0.0
    with pytest.raises(ValueError, match="nodes"):
        MultiATGCN(dict(c.config(), hip_train_regions=RegionMap(c.n + 1, labels=labels + [0])), c.data_feature)
    with pytest.raises(ValueError, match="nodes"):
        MultiATGCN(dict(c.config(), hip_train_regions=labels[:-1]), c.data_feature)
    for key in ("hip_region_loss_weight", "hip_tract_loss_weight"):
        for bad in (-0.5, NAN, INF, "much"):
            with pytest.raises(ValueError, match=key):
                MultiATGCN(dict(c.config(), hip_train_regions=rm, **{key: bad}), c.data_feature)
    with pytest.raises(ValueError, match="hip_train_regions"):
        MultiATGCN(dict(c.config(), hip_region_loss_weight=0.5), c.data_feature)
    for kw in (dict(region_weight=-1.0), dict(tract_weight=NAN), dict(regions=labels[:-1]),
               dict(region_weight=0.0, tract_weight=0.0)):
        with pytest.raises(ValueError):
            m.train_loss({}, "mse", **dict(dict(regions=rm), **kw))
    from multistgraph_amd import ops
    for tw, rw in ((0.0, 0.0), (-1.0, 1.0), (1.0, INF)):
        with pytest.raises(ValueError):
            ops.tract_region_loss(None, None, rm, 0, 0.0, 1.0, "mse", tract_weight=tw, region_weight=rw)


# ---- the reference against finite differences of its own value ------------------------------------------------------------
def _fd_case(whole=True):
    rng = np.random.default_rng(17)
    b, out, n = 2, 2, 9
    y = rng.standard_normal((b, out, n, 1))
    pred = y + 0.4 * rng.standard_normal((b, out, n, 1))
    groups = [[0, 1, 2, 3], [3, 4, 5], list(range(9)) if whole else [], [], [7, 3, 7]]  # overlap, whole, empty, twice
    weights = [rng.uniform(0.3, 1.5, len(g)).astype(F32).tolist() for g in groups]
    ptr = np.cumsum([0] + [len(g) for g in groups]).tolist()
    node = [k for g in groups for k in g]
    weight = [w for ws in weights for w in ws]
    return dict(pred=pred, y=y, y_start=0, mean=1.5, std=3.0), ptr, node, weight


@pytest.mark.parametrize("name", ["mse", "rmse", "logcosh", "huber"])
@pytest.mark.parametrize("weighted", [False, True], ids=["unit", "weighted"])
def test_reference_gradient_against_central_differences(name, weighted):
    """every smooth kind, in float64 on 2 x 2 x 9 x 1; huber away from its knee (|d| of every total at least 1e-3 from
    delta = 1, asserted)"""
    c, ptr, node, weight = _fd_case()
    weight = weight if weighted else None
    args = (c["y"], 0, c["mean"], c["std"], ptr, node, weight)
    r = RL.region_loss_ref(name, c["pred"], *args, upstream=1.0, dtype=F64)
    if name == "huber":
        assert np.abs(np.abs(r["P"] - r["L"]) - 1.0).min() > 1e-3
        assert (np.abs(r["P"] - r["L"]) < 1.0).any() and (np.abs(r["P"] - r["L"]) > 1.0).any()
    assert np.abs(r["grad"]).max() > 0 and (r["grad"][:, :, 8] != 0).all()             # node 8: the whole-graph group alone
    h = 1e-6
    fd = np.zeros_like(c["pred"])
    for idx in np.ndindex(*c["pred"].shape):
        up, dn = c["pred"].copy(), c["pred"].copy()
        up[idx] += h
        dn[idx] -= h
        fd[idx] = (RL.region_loss_ref(name, up, *args, dtype=F64)["value"]
                   - RL.region_loss_ref(name, dn, *args, dtype=F64)["value"]) / (2 * h)
    assert np.abs(fd - r["grad"]).max() <= 1e-7 * np.abs(r["grad"]).max(), (name, np.abs(fd - r["grad"]).max())
    # upstream and base enter linearly
    base = np.random.default_rng(3).standard_normal(c["pred"].shape).astype(F32)
    r2 = RL.region_loss_ref(name, c["pred"], *args, upstream=-2.0, base=base, dtype=F64)
    assert np.allclose(r2["grad"], base.astype(F64) - 2.0 * r["grad"], rtol=1e-13, atol=0)


def test_reference_float32_mode_follows_the_float64_function():
    """the reference the kernel is held to (float32 totals, elements and q) stays within float32 rounding of the float64
    function, and a node in no region gets exactly +0.0 or its base"""
    c, ptr, node, weight = _fd_case(whole=False)                     # nodes 6 and 8 in no region
    pred, y = c["pred"].astype(F32), c["y"].astype(F32)
    base = np.full(pred.shape, -0.0, dtype=F32)
    for name in ("mse", "rmse", "logcosh", "huber", "mae", "quantile"):
        r32 = RL.region_loss_ref(name, pred, y, 0, 1.5, 3.0, ptr, node, weight)
        r64 = RL.region_loss_ref(name, pred, y, 0, 1.5, 3.0, ptr, node, weight, dtype=F64)
        assert abs(r32["value"] - r64["value"]) <= 1e-5 * abs(r64["value"])
        if name not in ("mae", "quantile"):          # a sign can flip where a total's d rounds across 0; not on smooth kinds
            assert np.abs(r32["grad"] - r64["grad"]).max() <= 1e-5 * np.abs(r64["grad"]).max()
        outside = [6, 8]
        assert np.array_equal(r32["grad32"][:, :, outside].view(np.int32), np.zeros((2, 2, 2, 1), dtype=np.int32))
        rb = RL.region_loss_ref(name, pred, y, 0, 1.5, 3.0, ptr, node, weight, base=base)
        assert np.signbit(rb["grad32"][:, :, outside]).all() and (rb["grad32"][:, :, outside] == 0).all()


# ---- symbols, header, binding ---------------------------------------------------------------------------------------------
def test_symbols_header_and_binding(lib_built):
    lib = _lib().load()
    header = open(os.path.join(ROOT, "include", "matgcn.h")).read()
    for fn in NEW_FUNCTIONS:
        assert fn in _lib().EXPORTED_SYMBOLS and hasattr(lib, fn) and ("int %s(" % fn) in header
    assert lib.matgcn_abi_version() == 12
    from multistgraph_amd import build
    assert "matgcn_region_loss.hip" in build.DEPS
    capi = open(os.path.join(ROOT, "multistgraph_amd", "csrc", "matgcn_capi.hip")).read()
    assert capi.index('#include "matgcn_loss.hip"') < capi.index('#include "matgcn_region_loss.hip"')


# ---- the entry points' refusals -------------------------------------------------------------------------------------------
def _desc(kind=1, delta=0.0, mean=0.0, std=1.0, null_val=NAN, min_s=1e-4):
    return _lib().LossDesc(kind, mean, std, null_val, min_s, delta)


def _groups(ptr, null_ptr=False, null_dev=False, null_node=False, members=None):
    g = _lib().Groups()
    host = (C.c_int32 * len(ptr))(*ptr)
    g.ptr = None if null_ptr else C.cast(host, C.POINTER(C.c_int32))
    g.ptr_dev = None if null_dev else PTR
    g.node = None if null_node else PTR
    g.weight = None
    g.n_groups, g.n_members = len(ptr) - 1, ptr[-1] if members is None else members
    g._keep = host
    return g


N, BY_GROUP_PTR = 5, [0, 2, 2, 6]
BY_NODE_PTR = [0, 1, 2, 4, 5, 6]


def _call(lib, grad, pred=PTR, y=PTR, b=2, out=3, n=N, od=2, y_steps=3, y_feat=2, y_start=0, desc=None, null_desc=False,
          by_group=None, by_node=None, null_group=False, null_node=False, scratch=PTR, scratch_bytes=1 << 30, result=PTR,
          upstream=PTR, d_pred=PTR):
    d = _desc() if desc is None else desc
    bg = _groups(BY_GROUP_PTR) if by_group is None else by_group
    bn = _groups(BY_NODE_PTR) if by_node is None else by_node
    head = (pred, y, None, b, out, n, od, y_steps, y_feat, y_start, None if null_desc else C.byref(d),
            None if null_group else C.byref(bg))
    if grad:
        return lib.matgcn_region_loss_grad(*head, None if null_node else C.byref(bn), scratch, scratch_bytes, upstream,
                                           None, d_pred, None)
    return lib.matgcn_region_loss(*head, scratch, scratch_bytes, result, None)


def _bytes(lib, b, out, g, od):
    need = C.c_size_t(12345)
    return lib.matgcn_region_loss_bytes(b, out, g, od, C.byref(need)), need.value


def test_scratch_size(lib_built):
    """two float32 total tensors, matgcn_loss's scratch, the affine pair"""
    lib = _lib().load()
    for b, out, g, od in ((1, 1, 1, 1), (64, 24, 11, 1), (3, 64, 70, 2)):
        loss = C.c_size_t()
        assert lib.matgcn_loss_bytes(b, out, C.byref(loss)) == OK
        assert _bytes(lib, b, out, g, od) == (OK, 2 * 4 * b * out * g * od + loss.value + 8)
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 65, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (1, 1, -3, 1)):
        assert _bytes(lib, *bad)[0] == ERR_BAD_ARG, bad
    assert lib.matgcn_region_loss_bytes(1, 1, 1, 1, None) == ERR_NULL
    assert _bytes(lib, 1 << 30, 2, 1, 1)[0] == ERR_UNSUPPORTED
    assert _bytes(lib, 1, 1, 1 << 22, 2)[0] == ERR_UNSUPPORTED      # 256 * G * od of 2^31: as matgcn_group_sums


BAD_GEOMETRY = [dict(b=0), dict(out=0), dict(out=65), dict(n=0), dict(od=0), dict(y_steps=2), dict(y_start=-1),
                dict(y_start=1), dict(od=3)]
BAD_DESC = [dict(kind=-1), dict(kind=7), dict(kind=0, delta=NAN), dict(kind=5, delta=0.0), dict(kind=6, delta=1.5),
            dict(kind=6, delta=0.0)]


@pytest.mark.parametrize("grad", [False, True], ids=["value", "grad"])
def test_arguments_are_checked_on_the_host(lib_built, grad):
    lib = _lib().load()
    pointers = ("pred", "y", "scratch", "upstream", "d_pred") if grad else ("pred", "y", "scratch", "result")
    for name in pointers:
        assert _call(lib, grad, **{name: None}) == ERR_NULL, name
    assert _call(lib, grad, null_desc=True) == ERR_NULL and _call(lib, grad, null_group=True) == ERR_NULL
    for geometry in BAD_GEOMETRY:
        assert _call(lib, grad, **geometry) == ERR_BAD_ARG, geometry
    for fields in BAD_DESC:
        assert _call(lib, grad, desc=_desc(**fields)) == ERR_BAD_ARG, fields
    # the by-group map, as matgcn_group_sums checks it
    assert _call(lib, grad, by_group=_groups(BY_GROUP_PTR, null_ptr=True)) == ERR_NULL
    assert _call(lib, grad, by_group=_groups(BY_GROUP_PTR, null_dev=True)) == ERR_NULL
    assert _call(lib, grad, by_group=_groups(BY_GROUP_PTR, null_node=True)) == ERR_NULL
    for ptr in ([1, 2, 6], [0, 3, 2, 6]):
        assert _call(lib, grad, by_group=_groups(ptr)) == ERR_BAD_ARG, ptr
    assert _call(lib, grad, by_group=_groups(BY_GROUP_PTR, members=7)) == ERR_BAD_ARG
    need = _bytes(lib, 2, 3, 3, 2)[1]
    assert _call(lib, grad, scratch_bytes=need - 1) == ERR_SMALL_BUFFER
    assert _call(lib, grad, scratch_bytes=0) == ERR_SMALL_BUFFER
    assert _call(lib, grad, scratch=C.c_void_p(4100)) == ERR_BAD_ARG                      # not 8-byte aligned
    assert _call(lib, grad, n=1 << 16, od=1 << 15, y_feat=1 << 15) == ERR_UNSUPPORTED
    if grad:
        assert _call(lib, grad, null_node=True) == ERR_NULL
        assert _call(lib, grad, by_node=_groups(BY_NODE_PTR, null_ptr=True)) == ERR_NULL
        assert _call(lib, grad, by_node=_groups(BY_NODE_PTR[:-1] + [5])) == ERR_BAD_ARG    # another member count
        assert _call(lib, grad, by_node=_groups(BY_NODE_PTR + [6])) == ERR_BAD_ARG         # ptr over nodes + 1 nodes
        assert _call(lib, grad, by_node=_groups([0, 3, 2, 4, 5, 6])) == ERR_BAD_ARG        # decreasing
        assert _call(lib, grad, by_node=_groups(BY_NODE_PTR, members=7)) == ERR_BAD_ARG


def test_restated_caps_are_the_kernel_file_s():
    """region_loss_ref restates the constexpr the GPU tests place their shapes around"""
    import re
    src = open(os.path.join(ROOT, "multistgraph_amd", "csrc", "matgcn_region_loss.hip")).read()
    src += open(os.path.join(ROOT, "multistgraph_amd", "csrc", "matgcn_regions.hip")).read()
    const = dict(re.findall(r"constexpr int (\w+) = (\w+);", src))
    value = lambda k: int(const[k]) if const[k].isdigit() else value(const[k])
    for name in ("REGION_Q_FLOATS", "REGION_MAP_FLOATS", "REGION_TILE_ELEMS", "REGION_MAX_ROWS", "REGION_MIN_TILES",
                 "REGION_AHEAD"):
        assert value(name) == getattr(RL, name), name
    assert RL.rows_per_tile(64 * 24, 403, 1, 11) == 3 and RL.rows_per_tile(18, 257, 1, 70) == 1
    assert RL.rows_per_tile(1025, 5, 1, 2) == 2 and RL.rows_per_tile(4, 65, 1, 8193) is None
    assert RL.rows_per_tile(4, 65, 1, 8192) == 1
