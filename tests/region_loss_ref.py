"""numpy reference of matgcn_region_loss / matgcn_region_loss_grad (include/matgcn.h: "a training objective on region
totals"), built from regions_ref (the totals) and train_loss_ref (elements, terms and slopes).

Totals P, L: regions_ref.group_sums / group_label_sums with the scalar (mean, std) - float32, the bits of the kernels.
Value: the objective of train_loss_ref on (P, L) with an identity affine - masks act on totals.  The element values l, p
and d = p - l are formed in float32 like the kernel's, everything after them in float64.
Gradient: q = float32(slope * keep) per region element (rmse: divided by 2 rmse, all 0 when rmse == 0); per (row, node,
channel) one float64 chain over the node's memberships in ASCENDING MEMBER POSITION of the by-group map - start from 0.0,
add float64(weight[k]) * float64(q[group of k]) - then part = ((upstream * std) * acc) / cnt (cnt == 0: 0) and
d_pred = float32(part) or float32(float64(base) + part); a node in no region gets base, or +0.0."""
import numpy as np

import regions_ref as G
import train_loss_ref as T

F32, F64 = np.float32, np.float64
GRID_BITS = 5               # grid_case values (multiples of 2^-4, std 1 or 2) times weights in {1, 0.5, 2}: multiples of 2^-5

# the caps of csrc/matgcn_region_loss.hip, restated (tests/test_region_loss_host.py holds them to the source's constexpr)
REGION_Q_FLOATS = 8192      # coefficients of a tile in LDS; G * od above it: k_region_grad_walk
REGION_MAP_FLOATS = 4096    # a by-node map (group offsets, and weights if any) of up to this many floats is staged in LDS
REGION_TILE_ELEMS = 4096    # elements of d_pred in a tile of several rows
REGION_MAX_ROWS = 64        # rows of a tile
REGION_MIN_TILES = 512      # rows per tile are halved while fewer tiles than this would run
REGION_AHEAD = 8            # memberships of a chain fetched before they are added


def rows_per_tile(rows, n, od, n_groups):
    """R of k_region_grad_tile as matgcn_region_loss_grad chooses it (None: the walk kernel runs)"""
    gc = n_groups * od
    if gc > REGION_Q_FLOATS:
        return None
    r = max(1, min(REGION_Q_FLOATS // gc, REGION_TILE_ELEMS // (n * od), REGION_MAX_ROWS))
    while r > 1 and (rows + r - 1) // r < REGION_MIN_TILES:
        r = (r + 1) // 2
    return r


def group_of_members(ptr):
    """the group of every member position k of a by-group CSR map"""
    return [g for g in range(len(ptr) - 1) for _ in range(int(ptr[g + 1]) - int(ptr[g]))]


def transpose_brute(ptr, node, weight, num_nodes):
    """(nptr, ngroup, nweight) of the by-node map, by brute force: for every node, every member position in ascending
    order that names it"""
    group_of = group_of_members(ptr)
    nptr, ngroup, nweight = [0], [], []
    for n in range(num_nodes):
        for k in range(len(node)):
            if int(node[k]) == n:
                ngroup.append(group_of[k])
                nweight.append(None if weight is None else weight[k])
        nptr.append(len(ngroup))
    return nptr, ngroup, (None if weight is None else nweight)


def dense_membership(ptr, node, weight, num_nodes):
    """(G, N) float64: entry (g, n) the sum of the weights of n's memberships in g (weight None: their number)"""
    m = np.zeros((len(ptr) - 1, num_nodes), dtype=F64)
    for k, g in enumerate(group_of_members(ptr)):
        m[g, int(node[k])] += 1.0 if weight is None else F64(F32(weight[k]))
    return m


def totals(pred, y, y_start, mean, std, ptr, node, weight, label_start=None, dtype=F32):
    """(P, L) (B, out, G, od): float32 with the bits of the kernels, or - dtype float64 - the same sums in float64
    throughout (membership matrix times de-scaled values): the smooth function the finite differences are taken of"""
    _, out, n, od = np.asarray(pred).shape
    if dtype is F64:
        m = dense_membership(ptr, node, weight, n)
        labels = np.asarray(G.label_rows(y, out, y_start, od, label_start), dtype=F64)
        return (np.einsum("gn,bonc->bogc", m, np.asarray(pred, dtype=F64) * F64(std) + F64(mean)),
                np.einsum("gn,bonc->bogc", m, labels * F64(std) + F64(mean)))
    pred = np.asarray(pred, dtype=F32)
    P = G.group_sums(pred, ptr, node, weight, mean=mean, std=std)
    L = G.group_label_sums(y, ptr, node, weight, out, od, y_start, label_start, mean=mean, std=std)
    return P, L


def coefficients(name, P, L, delta=None, dtype=F32):
    """dict: values (1 + out,) float64, q (B, out, G, od) float64 BEFORE its rounding to float32, count.  l, p, d in
    ``dtype`` (float32: the kernel's), the rest in float64."""
    family, _, default_delta = T.LOSSES[name]
    delta = default_delta if delta is None else delta
    l, p, d, part = T.elements(name, P, L, 0, 0.0, 1.0, None, dtype)
    l, p, d = l.astype(F64), p.astype(F64), d.astype(F64)
    t, g = T.term_and_slope(family, l, p, d, float(F32(delta)), F64)
    if family in T.MASKED:
        live = part & ~np.isnan(t)
        t, g = np.where(live, t, 0.0), np.where(live, g, 0.0)
        cnt_h = part.sum(axis=(0, 2, 3)).astype(F64)
    else:
        cnt_h = np.full(t.shape[1], t.shape[0] * t.shape[2] * t.shape[3], dtype=F64)
    sum_h = t.sum(axis=(0, 2, 3))
    sums, cnts = np.concatenate([[sum_h.sum()], sum_h]), np.concatenate([[cnt_h.sum()], cnt_h])
    with np.errstate(invalid="ignore", divide="ignore"):
        vals = np.where(cnts > 0, sums / cnts, 0.0)
        if family == "rmse":
            vals = np.sqrt(vals)
            g = g / (2.0 * vals[0]) if vals[0] > 0 else np.zeros_like(g)
        if not cnts[0] > 0:
            g = np.zeros_like(g)
    return dict(values=vals, q=g, count=float(cnts[0]))


def region_loss_ref(name, pred, y, y_start, mean, std, ptr, node, weight, delta=None, label_start=None, upstream=1.0,
                    base=None, reverse=False, dtype=F32):
    """dict: values (1 + out,) float64 [all horizons, horizon 0 ..], grad (B, out, N, od) float64 = base + part before the
    last rounding, grad32 = the float32 the kernel stores, count, P, L.  ``reverse``: add the memberships of a node in
    descending member position instead - only for showing that the order matters.  dtype float64: no float32 rounding
    anywhere (totals, elements, q, upstream * std) - the mathematical function."""
    pred = np.asarray(pred, dtype=dtype)
    P, L = totals(pred, y, y_start, mean, std, ptr, node, weight, label_start, dtype)
    c = coefficients(name, P, L, delta, dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        q = c["q"].astype(F32).astype(F64) if dtype is F32 else c["q"]
    group_of = group_of_members(ptr)
    acc = np.zeros(pred.shape, dtype=F64)
    member = np.zeros(pred.shape[2], dtype=bool)
    ks = range(len(node) - 1, -1, -1) if reverse else range(len(node))
    with np.errstate(over="ignore", invalid="ignore"):
        for k in ks:
            w = F64(1.0) if weight is None else F64(F32(weight[k]))
            acc[:, :, int(node[k]), :] = acc[:, :, int(node[k]), :] + w * q[:, :, group_of[k], :]
            member[int(node[k])] = True
        scale = F64(F32(upstream)) * F64(F32(std)) if dtype is F32 else F64(upstream) * F64(std)
        part = (scale * acc) / c["count"] if c["count"] > 0 else np.zeros_like(acc)
        if base is None:
            grad = part
            grad32 = part.astype(F32)
            grad32[:, :, ~member, :] = F32(0.0)
        else:
            base = np.asarray(base, dtype=F32)
            grad = base.astype(F64) + part
            grad32 = grad.astype(F32)
            grad32[:, :, ~member, :] = base[:, :, ~member, :]
            grad[:, :, ~member, :] = base[:, :, ~member, :].astype(F64)
    return dict(values=c["values"], value=float(c["values"][0]), grad=grad, grad32=grad32, count=c["count"], P=P, L=L)


def assert_region_exact(name, c, ptr, node, weight, delta=None, label_start=None, grid_bits=GRID_BITS):
    """the condition of the bit-exact tests, on the reference alone: every product weight * member value is a multiple of
    2^-grid_bits and every total the same number however its chain is rounded (the float64 sum of a group is exact and
    needs fewer than 24 bits, so it fits float32); l, p, d and the mask of the totals are the same in float32 and float64
    arithmetic; the float64 terms stay on the grid of huber's 0.5 d^2, 2^-(2 grid_bits + 1) (mape's quotients aside), and
    their sum, in grid units, far below 2^53."""
    unit, term_grid = 2.0 ** grid_bits, 2.0 ** (2 * grid_bits + 1)
    family, _, default_delta = T.LOSSES[name]
    delta = default_delta if delta is None else delta
    pred = np.asarray(c["pred"], dtype=F32)
    _, out, _, od = pred.shape
    labels = G.label_rows(c["y"], out, c["y_start"], od, label_start)
    for x in (pred, labels):
        v = G.member_values(x, c["mean"], c["std"])
        v64 = np.asarray(x, dtype=F64) * F64(c["std"]) + F64(c["mean"])
        assert np.array_equal(v.astype(F64), v64, equal_nan=True), "the de-scale rounds"
        for g in range(len(ptr) - 1):
            nodes, w = G.members_of(ptr, node, weight, g)
            if not nodes:
                continue
            w = np.ones(len(nodes), dtype=F64) if w is None else w.astype(F64)
            prod = v64[..., nodes, :] * w[:, None]
            fin = np.isfinite(prod)
            assert bool((np.mod(prod[fin] * unit, 1.0) == 0).all()), "a member leaves the grid"
            total = np.where(fin, prod, 0.0).sum(axis=-2)                  # exact: grid multiples far below 2^53
            assert float(np.abs(np.where(fin, prod, 0.0)).sum(axis=-2).max()) * unit < 2.0 ** 24, "a total needs > 24 bits"
            assert np.array_equal(total.astype(F32).astype(F64), total)
    P, L = totals(pred, c["y"], c["y_start"], c["mean"], c["std"], ptr, node, weight, label_start)
    vals = {}
    for dtype in (F32, F64):
        l, p, d, part = T.elements(name, P, L, 0, 0.0, 1.0, None, dtype)
        vals[dtype] = [l, p, d, part]
    for a32, a64 in zip(vals[F32], vals[F64]):
        assert a32.dtype in (F32, bool), a32.dtype
        assert np.array_equal(a32.astype(F64), a64.astype(F64), equal_nan=True), "a float32 operation rounds: %s" % name
    if family != "mape":
        l, p, d, _ = (a.astype(F64) for a in vals[F64])
        t, _ = T.term_and_slope(family, l, p, d, delta, F64)
        fin = np.isfinite(t)
        assert bool((np.mod(t[fin] * term_grid, 1.0) == 0).all()), "terms leave their grid"
        assert float(np.abs(t[fin]).sum()) * term_grid < 2.0 ** 50
