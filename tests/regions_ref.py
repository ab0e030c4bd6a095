"""numpy reference of matgcn_group_sums / matgcn_group_label_sums (include/matgcn.h): the two float32 affines of
node_metrics_ref.descale_nodes, the clamp from below, then per (row, group, channel) one float64 chain over the group's
members IN LISTED ORDER - start from 0.0, add float64(weight) * float64(value) one member at a time - and one rounding to
float32 at the end.  The product of two float32 values is exact in float64, so the chain has one rounding per add whether or
not a multiply-add is fused: the kernels are held to these bits."""
import math

import numpy as np

import node_metrics_ref as R

F32, F64 = np.float32, np.float64
NAN = float("nan")


def members_of(ptr, node, weight, g):
    """(node indices, float32 weights or None) of group g of a CSR map"""
    lo, hi = int(ptr[g]), int(ptr[g + 1])
    return [int(n) for n in node[lo:hi]], None if weight is None else np.asarray(weight[lo:hi], dtype=F32)


def member_values(x, mean=None, std=None, group_mean=None, group_std=None, clamp_min=NAN):
    """x (..., N, od) float32 -> de-scaled and clamped from below (NaN: off), float32"""
    v = R.descale_nodes(x, mean, std, group_mean, group_std).copy()
    if not math.isnan(clamp_min):
        with np.errstate(invalid="ignore"):
            v[v < F32(clamp_min)] = F32(clamp_min)
    assert v.dtype == F32
    return v


def chain(values, nodes, weights=None, order=None):
    """values (..., N, od) float32 -> (..., od) float32: the float64 chain over ``nodes`` in listed order (``order``: a
    permutation of the member positions to add in instead - only for showing that the order matters)"""
    lead = values.shape[:-2] + values.shape[-1:]
    acc = np.zeros(lead, dtype=F64)
    ks = range(len(nodes)) if order is None else order
    with np.errstate(invalid="ignore", over="ignore"):
        for k in ks:
            w = F64(1.0) if weights is None else F64(F32(weights[k]))
            acc = acc + w * values[..., nodes[k], :].astype(F64)
        return acc.astype(F32)


def group_sums(x, ptr, node, weight=None, mean=None, std=None, group_mean=None, group_std=None, clamp_min=NAN):
    """x (..., N, od) -> (..., G, od) float32"""
    v = member_values(x, mean, std, group_mean, group_std, clamp_min)
    groups = len(ptr) - 1
    out = np.empty(v.shape[:-2] + (groups, v.shape[-1]), dtype=F32)
    for g in range(groups):
        nodes, w = members_of(ptr, node, weight, g)
        out[..., g, :] = chain(v, nodes, w)
    return out


def label_rows(y, out_steps, y_start, out_dim, label_start=None):
    """the labels a batch is scored against, (B, out, N, od): window labels (B, y_steps, N, F), or rows label_start[b] + o
    of the raw series (T, N, F)"""
    y = np.asarray(y, dtype=F32)
    if label_start is None:
        return y[:, :out_steps, :, y_start:y_start + out_dim]
    rows = np.asarray(label_start, dtype=np.int64)[:, None] + np.arange(out_steps)[None, :]
    return y[rows][..., y_start:y_start + out_dim]


def group_label_sums(y, ptr, node, weight, out_steps, out_dim, y_start=0, label_start=None, **scale):
    """(B, out, G, od) float32"""
    return group_sums(label_rows(y, out_steps, y_start, out_dim, label_start), ptr, node, weight, **scale)


def pairwise(values):
    """the float64 pairwise sum (halves split at len // 2, each summed the same way) of float32 values, rounded to float32
    once: a different order of the same adds"""
    def tree(vals):
        if len(vals) <= 1:
            return vals[0] if vals else F64(0.0)
        return tree(vals[:len(vals) // 2]) + tree(vals[len(vals) // 2:])
    return F32(tree([F64(F32(v)) for v in values]))
