"""Host-side handle on the HIP hot path: owns the device buffers and calls the C ABI.

``PathSpec`` describes one model configuration (everything in matgcn_dims except the batch size);
``HotPath`` binds a spec + batch size to a ``prepared`` and a ``workspace`` buffer and exposes one
method per entry point of include/matgcn.h.  Tensors go in and out as torch CUDA tensors; only raw
device pointers and the current HIP stream cross the boundary.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch

from . import _lib


@dataclass
class PathSpec:
    nodes: int
    out_window: int
    out_dim: int = 1
    start_dim: int = 0
    in_steps: int = 24
    x_steps: int = 96
    x_feat: int = 2
    hidden: int = 64
    layers: int = 2
    feat_in: int = 2
    embed_dim: int = 20
    adj_rank: int = 20
    adpadj: str = "unidirection"
    adjtype: str = "multi"
    cheb_k: int = 2
    n_static: int = 3
    head_begin: Sequence[int] = (0, 24, 48, 72)
    n_ts: int = 4
    ext_src: Sequence[int] = (1,)
    diag_static_mask: int = 0       # bit s: static support s is a diagonal matrix (folded, never mixed)
    gcn_off: bool = False           # ablation: dense GRU cells instead of graph cells (MultiATGCN.py:177-192)
    fnn_off: bool = False           # ablation: head over the last step only (:342-344,412)

    @property
    def scale_by_g(self) -> bool:
        return self.adjtype == "multi"

    @property
    def n_first(self) -> int:
        return (0 if self.adpadj == "none" else 1) + self.n_static

    @property
    def k_total(self) -> int:
        return 1 + self.n_first * (self.cheb_k - 1)

    def dims(self, batch: int) -> _lib.Dims:
        d = _lib.Dims()
        d.batch, d.nodes, d.in_steps, d.x_steps, d.x_feat = batch, self.nodes, self.in_steps, self.x_steps, self.x_feat
        d.out_channels, d.out_dim, d.start_dim = self.out_window * self.out_dim, self.out_dim, self.start_dim
        d.hidden, d.layers, d.feat_in = self.hidden, self.layers, self.feat_in
        d.embed_dim, d.adj_rank = self.embed_dim, self.adj_rank
        d.adp_mode = _lib.ADP_CODES[self.adpadj]
        d.n_static, d.cheb_k, d.scale_by_g = self.n_static, self.cheb_k, int(self.scale_by_g)
        d.n_heads, d.n_ts = len(self.head_begin), self.n_ts
        d.diag_static_mask = int(self.diag_static_mask)
        d.gcn_off, d.fnn_off = int(self.gcn_off), int(self.fnn_off)
        for i, v in enumerate(self.head_begin):
            d.head_begin[i] = int(v)
        for i, v in enumerate(self.ext_src):
            d.ext_src[i] = int(v)
        return d


def diagonal_mask(static_supports) -> int:
    """Bit s set when static support s (host array / CPU or GPU tensor, (S,N,N)) has no off-diagonal entry.
    Host-side check made once at model construction; such supports are folded into the weights."""
    if static_supports is None:
        return 0
    st = torch.as_tensor(static_supports).detach().cpu()
    mask = 0
    for i in range(st.shape[0]):
        m = st[i]
        if torch.count_nonzero(m - torch.diag(torch.diagonal(m))).item() == 0:
            mask |= 1 << i
    return mask


def spec_from_config(config, data_feature, num_nodes: int, adj_rank: int, n_static: int,
                     diag_static_mask: int = 0, hidden: Optional[int] = None) -> PathSpec:
    """Derive the path description from the reference's config / data_feature keys
    (MultiATGCN.py:224-235, 264-265, 310-332; head windows :371-393).  ``config`` only needs ``get`` (LibCity's
    ConfigParser has no ``keys()``, so it is never copied); ``hidden`` overrides ``rnn_units`` (the padded width the
    kernels run, hidden_pad.py)."""
    out_window = config.get("output_window", 1)
    start_dim, end_dim = config.get("start_dim", 0), config.get("end_dim", 1)
    od = end_dim - start_dim
    tid = 0
    if config.get("add_time_in_day", False):
        tid = 8 if config.get("add_day_in_week", False) else 1
    lc = data_feature.get("len_closeness", 0)
    lp = data_feature.get("len_period", 0)
    lt = data_feature.get("len_trend", 0)
    heads: List[int] = []
    for kk in range(lc // 24):
        heads.append(24 * kk)
    if lp > 0 and out_window >= 6:
        for kk in range(lp // 24):
            heads.append(lc + 24 * kk)
    if lt > 0 and out_window >= 6:
        for kk in range(lt // 24):
            heads.append(lc + lp)  # the reference never advances the trend window (:389-393)
    ext_dim = data_feature.get("ext_dim", 1)
    x_feat = int(data_feature.get("feature_dim", od + ext_dim))
    ext: List[int] = []
    if config.get("add_time_in_day", False):
        ext += [end_dim + j for j in range(tid)]
    if config.get("load_dynamic", False):
        ext += list(range(end_dim + tid, x_feat))
    feat_in = od + ext_dim  # feature_final (:321); must equal od + len(ext) for cat() to line up
    if feat_in != od + len(ext):
        raise ValueError("feature_final=%d but forward() concatenates %d channels" % (feat_in, od + len(ext)))
    node_specific_off = config.get("node_specific_off", False)
    return PathSpec(
        nodes=num_nodes, out_window=out_window, out_dim=od, start_dim=start_dim,
        in_steps=config.get("input_window", 1), x_steps=lc + lp + lt, x_feat=x_feat,
        hidden=config.get("rnn_units", 64) if hidden is None else hidden, layers=config.get("num_layers", 2), feat_in=feat_in,
        embed_dim=1 if node_specific_off else config.get("embed_dim_node", 10), adj_rank=adj_rank,
        adpadj=config.get("adpadj", "bidirection"), adjtype=config.get("adjtype", "od"),
        cheb_k=config.get("cheb_order", 2), n_static=n_static, head_begin=tuple(heads),
        n_ts=int((lp + lt + lc) / 24), ext_src=tuple(ext), diag_static_mask=diag_static_mask,
        gcn_off=bool(config.get("gcn_off", False)), fnn_off=bool(config.get("fnn_off", False)))


# ---- the shared pieces of every wrapper below ----------------------------------------------------------------------------
# _lib.call(name, *args) looks the entry point up, calls it and checks its status: the signature table converts plain ints
# (device pointers), floats and None (NULL).  _stream: the caller's stream.  _label_view: the label contract, once.
# _out_arg: the one check of a tensor the caller hands in to be written.  _scratch: the one get / clear-when-full / put of the scratch caches.
def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream(device) -> int:
    """torch's current HIP stream on ``device`` at call time, as the handle the C ABI takes"""
    return torch.cuda.current_stream(device).cuda_stream


def _check_tensor(t: torch.Tensor, name: str, shape=None) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.MatgcnError("%s must live on the GPU: the hot path is HIP-only (no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise _lib.MatgcnError("%s must be float32, got %s" % (name, t.dtype))
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise _lib.MatgcnError("%s has shape %s, expected %s" % (name, tuple(t.shape), tuple(shape)))
    return t.contiguous()


def _out_arg(t: Optional[torch.Tensor], shape, dtype, device, name: str):
    """(the tensor an entry point writes, whether the caller gave it): a fresh one, or the caller's own - running sums or
    counts to add to, a slice of a store to fill - after the one check there is: same device, exact dtype, exact shape,
    contiguous.  The library writes it as dense memory, so nothing here may be converted or copied."""
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device), False
    if tuple(t.shape) != shape or t.dtype != dtype or t.device != device or not t.is_contiguous():
        raise _lib.MatgcnError("%s must be a contiguous %s tensor of shape %s on %s" % (name, dtype, shape, device))
    return t, True


_mc_scratch: Dict[tuple, torch.Tensor] = {}     # (device, entry point, batch, out, nodes, od, S, levels) -> stage-1 partials
_norm_scratch: Dict[tuple, torch.Tensor] = {}   # (device, bytes) -> the per-chunk partials of matgcn_grad_norm
_SCRATCH_ENTRIES = 16                           # per cache


def _scratch(cache: Dict[tuple, torch.Tensor], key: tuple, nbytes: int, device) -> torch.Tensor:
    """fp64 scratch of ``nbytes`` (one element at least) that the calls of one ``key`` on one device share - a call writes
    it before it reads it, in stream order -, kept in ``cache``, which is cleared when it is full."""
    key = (device,) + key
    t = cache.get(key)
    if t is None:
        if len(cache) >= _SCRATCH_ENTRIES:
            cache.clear()
        t = cache[key] = torch.empty(max(1, nbytes // 8), dtype=torch.float64, device=device)
    return t


def debug_gemm(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor, desc, alpha=1.0, beta=0.0) -> None:
    """matgcn_debug_gemm on raw buffers (tests): desc = the 22 integers of include/matgcn.h."""
    arr = (C.c_int64 * 22)(*[int(v) for v in desc])
    _lib.call("matgcn_debug_gemm", a.data_ptr(), b.data_ptr(), c.data_ptr(), arr, float(alpha), float(beta),
              _stream(c.device))


class _LabelView(NamedTuple):
    """The label contract (include/matgcn.h) of one call, checked: the contiguous tensors and the geometry every
    label-reading entry point takes.  Built by _label_view; autograd functions keep it for their backward."""
    pred: Optional[torch.Tensor]    # (B, out, N, od), the samples (S, B, out, N, od), or None (built from a shape)
    y: torch.Tensor                 # (B, y_steps, N, F) windows, or the raw series (T, N, F)
    label_start: Optional[torch.Tensor]     # (B,) int32 with the series: rows label_start[b] .. + out are b's targets
    b: int
    out: int
    n: int
    od: int
    y_steps: int
    y_feat: int

    def save(self, ctx, *more) -> "_LabelView":
        """pred, y and ``more`` go through ctx.save_for_backward (released with the graph, as they always were); returns
        what an autograd function keeps on ctx beside them: the geometry and label_start"""
        ctx.save_for_backward(self.pred, self.y, *more)
        return self._replace(pred=None, y=None)

    def saved(self, ctx) -> list:
        """[the whole view again, *more] in backward"""
        pred, y, *more = ctx.saved_tensors
        return [self._replace(pred=pred, y=y)] + more

    def args(self, y_start) -> tuple:
        """the leading C arguments: [pred | samples, S], y, label_start, b, out, n, od, y_steps, y_feat, y_start"""
        p = self.pred
        lead = () if p is None else (p.data_ptr(),) if p.dim() == 4 else (p.data_ptr(), int(p.shape[0]))
        return lead + (self.y.data_ptr(), _ptr(self.label_start), self.b, self.out, self.n, self.od, self.y_steps,
                       self.y_feat, int(y_start))


def _label_view(pred, y, label_start, samples: bool = False) -> _LabelView:
    """``pred``: the prediction (B, out, N, od) - ``samples``: the ensemble (S, B, out, N, od) - or the bare shape
    (B, out, N, od) of an entry point that reads labels only.  ``y`` is (B, y_steps, N, F) windows, or - with label_start
    (B) int32 - the raw series (T, N, F).  Every refusal is a MatgcnError."""
    if isinstance(pred, torch.Tensor):
        pred = _check_tensor(pred, "samples" if samples else "pred")
        if pred.dim() != (5 if samples else 4):
            raise _lib.MatgcnError("%s has shape %s, expected %s" % (
                ("samples", tuple(pred.shape), "(S, B, out, N, od)") if samples else
                ("pred", tuple(pred.shape), "(B, out, N, od)")))
        shape = pred.shape[1:] if samples else pred.shape
    else:
        shape, pred = pred, None
    b, out, n, od = shape
    y = _check_tensor(y, "y")
    if label_start is None:
        if y.dim() != 4 or y.shape[0] != b or y.shape[2] != n:
            raise _lib.MatgcnError("y has shape %s, incompatible with pred %s" % (tuple(y.shape), (b, out, n, od)))
        return _LabelView(pred, y, None, b, out, n, od, int(y.shape[1]), int(y.shape[3]))
    if y.dim() != 3 or y.shape[1] != n:
        raise _lib.MatgcnError("series has shape %s, expected (T, %d, F)" % (tuple(y.shape), n))
    if not isinstance(label_start, torch.Tensor) or not label_start.is_cuda or label_start.dtype != torch.int32 or \
            tuple(label_start.shape) != (b,):
        raise _lib.MatgcnError("label_start must be a CUDA int32 tensor of shape (%d,)" % b)
    return _LabelView(pred, y, label_start.contiguous(), b, out, n, od, int(y.shape[0]), int(y.shape[2]))


def _mae_call(v: _LabelView, y_start, mean, std, null_val, min_s):
    """the value call: (partials - kept for the gradient -, result (1 + out,))"""
    dev = v.pred.device
    partials = torch.empty(2 * v.b * v.out + 1, dtype=torch.float32, device=dev)
    result = torch.empty(1 + v.out, dtype=torch.float32, device=dev)
    _lib.call("matgcn_masked_mae", *v.args(y_start), float(mean), float(std), float(null_val), float(min_s),
              partials.data_ptr(), result.data_ptr(), _stream(dev))
    return partials, result


def masked_mae_device(pred: torch.Tensor, y: torch.Tensor, y_start: int, mean: float, std: float,
                      null_val: float = float("nan"), min_s: float = 1e-4,
                      label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(1 + out,) tensor [masked-MAE over all horizons, MAE@1 .. MAE@out] computed on the device by
    matgcn_masked_mae (de-scale + mask + reduce; reference loss.py:17-29, traffic_state_evaluator.py:87-104).
    With label_start, y is the raw series and the targets are gathered on the device."""
    return _mae_call(_label_view(pred, y, label_start), y_start, mean, std, null_val, min_s)[1]


def _upstream(upstream: torch.Tensor) -> torch.Tensor:
    """the upstream gradient of a scalar loss as the (1,) float32 device tensor the gradient kernels read"""
    return upstream.detach().to(torch.float32).reshape(1).contiguous()


class _MaskedMAE(torch.autograd.Function):
    """calculate_loss on the device with its gradient (matgcn_masked_mae / matgcn_masked_mae_grad)."""

    @staticmethod
    def forward(ctx, pred, y, y_start, mean, std, null_val, min_s, label_start):
        v = _label_view(pred.detach(), y, label_start)
        ctx.args = (int(y_start), float(mean), float(std), float(null_val), float(min_s))
        partials, result = _mae_call(v, *ctx.args)
        ctx.view = v.save(ctx, partials)
        return result[0].clone()

    @staticmethod
    def backward(ctx, upstream):
        v, partials = ctx.view.saved(ctx)
        pred = v.pred
        d_pred = torch.empty_like(pred)
        up = _upstream(upstream)
        y_start, *scale = ctx.args
        _lib.call("matgcn_masked_mae_grad", *v.args(y_start), *scale, partials.data_ptr(), up.data_ptr(),
                  d_pred.data_ptr(), _stream(pred.device))
        return d_pred, None, None, None, None, None, None, None


def masked_mae_loss(pred: torch.Tensor, y: torch.Tensor, y_start: int, mean: float, std: float,
                    null_val: float = float("nan"), min_s: float = 1e-4,
                    label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The calculate_loss scalar with autograd support: the device reduction forward, matgcn_masked_mae_grad backward.
    With label_start, y is the raw series and the targets are gathered on the device."""
    return _MaskedMAE.apply(pred, y, y_start, mean, std, null_val, min_s, label_start)


# The executor's differentiable training objectives (TrafficStateExecutor._build_train_loss, traffic_state_executor.py:
# 200-250): name -> (kind, null_val, default delta).  mae / mse / rmse / mape are loss.masked_*_torch with their default
# null value NaN, the masked_* names the same functions with null_val = 0; logcosh / huber / quantile are plain means.
_NAN = float("nan")
TRAIN_LOSSES = {
    "mae": (_lib.LOSS_MAE, _NAN, 0.0), "mse": (_lib.LOSS_MSE, _NAN, 0.0), "rmse": (_lib.LOSS_RMSE, _NAN, 0.0),
    "mape": (_lib.LOSS_MAPE, _NAN, 0.0),
    "logcosh": (_lib.LOSS_LOGCOSH, _NAN, 0.0), "huber": (_lib.LOSS_HUBER, _NAN, 1.0),
    "quantile": (_lib.LOSS_QUANTILE, _NAN, 0.25),
    "masked_mae": (_lib.LOSS_MAE, 0.0, 0.0), "masked_mse": (_lib.LOSS_MSE, 0.0, 0.0),
    "masked_rmse": (_lib.LOSS_RMSE, 0.0, 0.0), "masked_mape": (_lib.LOSS_MAPE, 0.0, 0.0),
}
TRAIN_LOSS_MIN_S = 1e-4     # loss.masked_*_torch: |label| < min_s -> 0 (the unmasked kinds have no such rule)
NOT_DIFFERENTIABLE_LOSSES = ("r2", "evar")


def train_loss_desc(name: str, mean: float, std: float, delta=None) -> "_lib.LossDesc":
    """the matgcn_loss_desc of the executor's objective ``name`` (a key of TRAIN_LOSSES)"""
    key = str(name).lower()
    if key in NOT_DIFFERENTIABLE_LOSSES:
        raise ValueError("train loss %r is a CPU sklearn score in the reference (loss.r2_score_torch / "
                         "explained_variance_score_torch): it is not differentiable and cannot be trained on" % name)
    if key not in TRAIN_LOSSES:
        raise ValueError("train loss %r: expected one of %s" % (name, ", ".join(TRAIN_LOSSES)))
    kind, null_val, default_delta = TRAIN_LOSSES[key]
    masked = kind <= _lib.LOSS_MAPE
    delta = float(default_delta if delta is None else delta)
    if not math.isfinite(delta) or (kind == _lib.LOSS_HUBER and not delta > 0.0) or \
            (kind == _lib.LOSS_QUANTILE and not 0.0 < delta < 1.0):
        raise ValueError("train loss %r: delta = %r (huber needs delta > 0, quantile 0 < delta < 1)" % (name, delta))
    return _lib.LossDesc(kind, float(mean), float(std), null_val, TRAIN_LOSS_MIN_S if masked else 0.0, delta)


def _loss_call(v: _LabelView, y_start, desc):
    """the value call: (scratch - kept for the gradient, so per call -, result (1 + out,))"""
    dev = v.pred.device
    need = C.c_size_t()
    _lib.call("matgcn_loss_bytes", v.b, v.out, C.byref(need))
    scratch = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
    result = torch.empty(1 + v.out, dtype=torch.float32, device=dev)
    _lib.call("matgcn_loss", *v.args(y_start), C.byref(desc), scratch.data_ptr(), need.value, result.data_ptr(),
              _stream(dev))
    return scratch, result


def train_loss_device(pred: torch.Tensor, y: torch.Tensor, y_start: int, mean: float, std: float, name: str,
                      delta=None, label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(1 + out,) tensor [the executor's objective ``name`` over all horizons, the same per horizon] computed on the
    device by matgcn_loss (de-scale + mask + fixed-order reduction).  Geometry as masked_mae_device: ``y`` windows, or
    with label_start the raw series whose targets are gathered on the device."""
    return _loss_call(_label_view(pred, y, label_start), y_start, train_loss_desc(name, mean, std, delta))[1]


def train_loss(pred: torch.Tensor, y: torch.Tensor, y_start: int, mean: float, std: float, name: str, delta=None,
               label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scalar of the executor's objective ``name`` with autograd support: matgcn_loss forward, matgcn_loss_grad
    backward (the tract half of tract_region_loss alone).  With label_start, y is the raw series and the targets are
    gathered on the device."""
    return _TractRegionLoss.apply(pred, y, None, y_start, train_loss_desc(name, mean, std, delta), label_start, 1.0, 0.0)


_affine_uploads: Dict[tuple, torch.Tensor] = {}    # (device, the float32 bytes of a host-side affine) -> its device copy


def _affine_arg(v, n, device, name):
    """scalar or length-N vector -> (float32 device tensor, per_node flag).  A device tensor is used where it lies.  Host
    values (the scaler's numbers, a per-node numpy vector) are uploaded once per content and kept: a copy from pageable
    host memory makes the host wait until the CALLER'S STREAM has drained, so an upload per batch would put a device
    wait into every metric, score and region call of an evaluation pass (tests/test_stream_order.py).  The kept tensors
    are never written."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        t = v.detach().to(dtype=torch.float32).reshape(-1).to(device)
    else:
        host = torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).contiguous()
        device = torch.device(device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, host.numpy().tobytes())
        t = _affine_uploads.get(key)
        if t is None:
            if len(_affine_uploads) >= 64:
                _affine_uploads.clear()
            t = _affine_uploads[key] = host.to(device)
    if t.numel() not in (1, n):
        raise _lib.MatgcnError("%s has %d entries, expected 1 or %d (one per node)" % (name, t.numel(), n))
    return t.contiguous(), int(t.numel() == n and n > 1)


def _metric_scale(n, device, mean, std, group_mean, group_std, clamp_min, truth_min, min_s):
    """(matgcn_metric_scale, the device tensors its pointers refer to - hold them until the call is enqueued)"""
    sc = _lib.MetricScale()
    keep = []
    if (mean is None) != (std is None) or (group_mean is None) != (group_std is None):
        raise _lib.MatgcnError("mean / std (and group_mean / group_std) come in pairs")
    if mean is not None:
        m, pn = _affine_arg(mean, n, device, "mean")
        sd, pn2 = _affine_arg(std, n, device, "std")
        if pn != pn2:       # broadcast the scalar one
            m, sd = (m.expand(n).contiguous() if not pn else m), (sd.expand(n).contiguous() if not pn2 else sd)
        keep += [m, sd]
        sc.mean, sc.std, sc.per_node = m.data_ptr(), sd.data_ptr(), int(pn or pn2)
    if group_mean is not None:
        gm, _ = _affine_arg(group_mean, n, device, "group_mean")
        gs, _ = _affine_arg(group_std, n, device, "group_std")
        gm, gs = gm.expand(n).contiguous(), gs.expand(n).contiguous()
        keep += [gm, gs]
        sc.mean2, sc.std2 = gm.data_ptr(), gs.data_ptr()
    sc.clamp_min, sc.truth_min, sc.min_s = float(clamp_min), float(truth_min), float(min_s)
    return sc, keep


def metric_sums(pred: torch.Tensor, y: torch.Tensor, y_start: int = 0, mean=None, std=None, group_mean=None,
                group_std=None, clamp_min: float = float("nan"), truth_min: float = float("nan"), min_s: float = 1e-4,
                label_start: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(out, 14) float64 device tensor of the per-horizon sums the evaluator's metrics are ratios of
    (matgcn_metric_sums, include/matgcn.h): de-scale (mean / std: the scaler, scalar or per node; group_mean /
    group_std: the per-node group-std re-transform), clamp, select, zero tiny labels and reduce on the device.
    ``sums``: running sums of earlier batches to add to (several batches = one collect over their concatenation)."""
    v = _label_view(pred, y, label_start)
    dev = v.pred.device
    sc, _keep = _metric_scale(v.n, dev, mean, std, group_mean, group_std, clamp_min, truth_min, min_s)
    partials = torch.empty(v.b * v.out * _lib.METRIC_SUMS, dtype=torch.float64, device=dev)
    sums, given = _out_arg(sums, (v.out, _lib.METRIC_SUMS), torch.float64, dev, "sums")
    _lib.call("matgcn_metric_sums", *v.args(y_start), C.byref(sc), partials.data_ptr(), sums.data_ptr(), int(given),
              _stream(dev))
    return sums


def metric_table(sums: torch.Tensor, swap_r2: bool = False) -> torch.Tensor:
    """(2, out, 10) float64 device tensor from (accumulated) metric sums: [0] the evaluator's "single" mode, [1] its
    "average" mode; metric order _lib.METRICS (matgcn_metric_table)."""
    out = int(sums.shape[0])
    table = torch.empty(2, out, len(_lib.METRICS), dtype=torch.float64, device=sums.device)
    _lib.call("matgcn_metric_table", sums.data_ptr(), out, int(bool(swap_r2)), table.data_ptr(), _stream(sums.device))
    return table


def metric_sums_nodes(pred: torch.Tensor, y: torch.Tensor, y_start: int = 0, mean=None, std=None, group_mean=None,
                      group_std=None, clamp_min: float = float("nan"), truth_min: float = float("nan"),
                      min_s: float = 1e-4, label_start: Optional[torch.Tensor] = None,
                      sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(out, N, 14) float64 device tensor: the sums of ``metric_sums`` per horizon AND node (matgcn_metric_sums_nodes),
    every entry added up over batch and channel in a fixed order - feeding a test set batch by batch through ``sums``
    gives the bits of one call over all of it."""
    v = _label_view(pred, y, label_start)
    dev = v.pred.device
    sc, _keep = _metric_scale(v.n, dev, mean, std, group_mean, group_std, clamp_min, truth_min, min_s)
    need = C.c_size_t(0)
    _lib.call("matgcn_metric_sums_nodes_bytes", v.b, v.out, v.n, v.od, C.byref(need))
    scratch = torch.empty(need.value // 8, dtype=torch.float64, device=dev) if need.value else None
    sums, given = _out_arg(sums, (v.out, v.n, _lib.METRIC_SUMS), torch.float64, dev, "sums")
    _lib.call("matgcn_metric_sums_nodes", *v.args(y_start), C.byref(sc), _ptr(scratch), need.value, sums.data_ptr(),
              int(given), _stream(dev))
    return sums


def metric_table_rows(sums: torch.Tensor, fold: int = 1, swap_r2: bool = False) -> torch.Tensor:
    """(rows, 10) float64 device tensor from metric sums (..., 14) whose leading axes flatten to fold * rows: row r is
    the table of sum_{f < fold} sums[f * rows + r] (matgcn_metric_table_rows) - ``fold`` = 1 on (out, N, 14) sums: one
    row per (horizon, node); ``fold`` = out: one row per node over all horizons.  Metric order _lib.METRICS."""
    if not sums.is_cuda or sums.dtype != torch.float64 or sums.dim() < 2 or sums.shape[-1] != _lib.METRIC_SUMS:
        raise _lib.MatgcnError("sums must be a CUDA float64 tensor of shape (..., %d)" % _lib.METRIC_SUMS)
    sums = sums.contiguous()
    total, fold = sums.numel() // _lib.METRIC_SUMS, int(fold)
    if fold < 1 or total < 1 or total % fold:
        raise _lib.MatgcnError("fold = %d does not divide the %d rows of sums" % (fold, total))
    rows = total // fold
    table = torch.empty(rows, len(_lib.METRICS), dtype=torch.float64, device=sums.device)
    _lib.call("matgcn_metric_table_rows", sums.data_ptr(), rows, fold, int(bool(swap_r2)), table.data_ptr(),
              _stream(sums.device))
    return table


def _mc_probs(probs):
    """the quantile levels as the host float array the C ABI takes"""
    vals = [float(v) for v in probs]
    return (C.c_float * len(vals))(*vals), len(vals)


def _mc_samples(samples: torch.Tensor) -> torch.Tensor:
    samples = _check_tensor(samples, "samples")
    if samples.dim() < 2:
        raise _lib.MatgcnError("samples has shape %s, expected (S, ...): the sample axis first" % (tuple(samples.shape),))
    return samples


def mc_quantiles(samples: torch.Tensor, probs: Sequence[float], mean: float = 0.0, std: float = 1.0) -> torch.Tensor:
    """Empirical quantiles over the sample axis of the Monte-Carlo-dropout forecasts (matgcn_mc_quantiles):
    ``samples`` (S, ...) as HotPath.forward_mc(keep_samples=True) returns them, de-scaled as x*std + mean on load;
    ``probs`` up to 8 ascending levels in [0, 1].  Returns (len(probs), *samples.shape[1:]) - numpy's "linear" rule in
    float32, no sorted copy of the samples anywhere."""
    samples = _mc_samples(samples)
    levels, nq = _mc_probs(probs)
    s, elems = int(samples.shape[0]), samples[0].numel()
    out = torch.empty((nq,) + tuple(samples.shape[1:]), dtype=torch.float32, device=samples.device)
    _lib.call("matgcn_mc_quantiles", samples.data_ptr(), s, elems, levels, nq, float(mean), float(std), out.data_ptr(),
              _stream(samples.device))
    return out


def mc_scores(samples: torch.Tensor, y: torch.Tensor, probs: Sequence[float], y_start: int = 0, mean: float = 0.0,
              std: float = 1.0, null_val: float = 0.0, min_s: float = 1e-4, label_start: Optional[torch.Tensor] = None,
              sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(out, 5 + len(probs)) float64 device tensor of per-horizon sums [count, CRPS, covered, width, Winkler, pinball per
    level] of the ensemble ``samples`` (S, B, out, N, od) against the labels (matgcn_mc_scores, include/matgcn.h): labels,
    mask and geometry as masked_mae_device (``y`` windows, or with ``label_start`` the resident series), the interval is
    [first level, last level].  ``sums``: running sums of earlier batches to add to."""
    v = _label_view(samples, y, label_start, samples=True)
    dev, s = v.pred.device, int(v.pred.shape[0])
    levels, nq = _mc_probs(probs)
    need = C.c_size_t(0)
    _lib.call("matgcn_mc_scores_bytes", v.b, v.out, v.n, v.od, s, nq, C.byref(need))
    scratch = _scratch(_mc_scratch, ("mc_scores", v.b, v.out, v.n, v.od, s, nq), need.value, dev)
    sums, given = _out_arg(sums, (v.out, _lib.MC_SCORE_SUMS + nq), torch.float64, dev, "sums")
    _lib.call("matgcn_mc_scores", *v.args(y_start), float(mean), float(std), float(null_val), float(min_s), levels, nq,
              scratch.data_ptr(), scratch.numel() * 8, sums.data_ptr(), int(given), _stream(dev))
    return sums


def _crps_call(v: _LabelView, y_start, scale):
    """the value call on the samples of ``v``: (scratch - kept for the gradient, so per call -, result (1 + out,))"""
    dev = v.pred.device
    need = C.c_size_t()
    _lib.call("matgcn_crps_loss_bytes", v.b, v.out, C.byref(need))
    scratch = torch.empty(need.value // 8, dtype=torch.float64, device=dev)
    result = torch.empty(1 + v.out, dtype=torch.float32, device=dev)
    _lib.call("matgcn_crps_loss", *v.args(y_start), *scale, scratch.data_ptr(), need.value, result.data_ptr(), _stream(dev))
    return scratch, result


def crps_loss_device(samples: torch.Tensor, labels: torch.Tensor, y_start: int = 0, mean: float = 0.0, std: float = 1.0,
                     null_val: float = 0.0, min_s: float = 1e-4,
                     label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(1 + out,) tensor [the mean CRPS of the ensemble ``samples`` (S, B, out, N, od) over all unmasked elements, the same
    per horizon] (matgcn_crps_loss): ``labels`` (the label windows, or with label_start the raw series), mask and geometry
    as ``mc_scores``, whose CRPS sums it divides by their counts."""
    v = _label_view(samples, labels, label_start, samples=True)
    return _crps_call(v, y_start, (float(mean), float(std), float(null_val), float(min_s)))[1]


class _CrpsLoss(torch.autograd.Function):
    """the ensemble's mean CRPS with its gradient w.r.t. the samples (matgcn_crps_loss / matgcn_crps_loss_grad)"""

    @staticmethod
    def forward(ctx, samples, y, y_start, mean, std, null_val, min_s, label_start):
        v = _label_view(samples.detach(), y, label_start, samples=True)
        ctx.args = (int(y_start), (float(mean), float(std), float(null_val), float(min_s)))
        scratch, result = _crps_call(v, *ctx.args)
        ctx.view = v.save(ctx, scratch)
        return result[0].clone()

    @staticmethod
    def backward(ctx, upstream):
        v, scratch = ctx.view.saved(ctx)
        samples = v.pred
        y_start, scale = ctx.args
        # the gradient takes the place of the samples (a workgroup reads its tile completely before it writes it): no
        # second (S, B, out, N, od) tensor.  The samples were made for this objective and nothing else reads them.
        # (upstream stays on the device: reading it for the C argument would make the host wait for the stream)
        _lib.call("matgcn_crps_loss_grad", *v.args(y_start), *scale, scratch.data_ptr(), scratch.numel() * 8, 1.0,
                  samples.data_ptr(), _stream(samples.device))
        return samples.mul_(upstream.detach().to(torch.float32)), None, None, None, None, None, None, None


def crps_loss(samples: torch.Tensor, labels: torch.Tensor, y_start: int = 0, mean: float = 0.0, std: float = 1.0,
              null_val: float = 0.0, min_s: float = 1e-4, label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scalar mean CRPS of the ensemble ``samples`` (S, B, out, N, od) with autograd support over the samples:
    matgcn_crps_loss forward, matgcn_crps_loss_grad backward.  The backward writes the gradient IN PLACE of the samples
    tensor - after it the tensor no longer holds the forecasts.  ``labels``: the label windows, or with label_start the
    raw series."""
    return _CrpsLoss.apply(samples, labels, y_start, mean, std, null_val, min_s, label_start)


def mc_quantiles_scaled(samples: torch.Tensor, probs: Sequence[float], mean=None, std=None, group_mean=None,
                        group_std=None, clamp_min: float = float("nan")) -> torch.Tensor:
    """``mc_quantiles`` on the re-transformed scale (matgcn_mc_quantiles_scaled): ``samples`` (S, ..., N, od), every
    sample de-scaled by mean / std (scalars or one pair per node), then by the per-node group_mean / group_std, and set
    to ``clamp_min`` where below it, before the sort.  Returns (len(probs), *samples.shape[1:])."""
    samples = _mc_samples(samples)
    if samples.dim() < 3:
        raise _lib.MatgcnError("samples has shape %s, expected (S, ..., N, od)" % (tuple(samples.shape),))
    levels, nq = _mc_probs(probs)
    s, elems, n, od = int(samples.shape[0]), samples[0].numel(), int(samples.shape[-2]), int(samples.shape[-1])
    sc, _keep = _metric_scale(n, samples.device, mean, std, group_mean, group_std, clamp_min, float("nan"), -1.0)
    out = torch.empty((nq,) + tuple(samples.shape[1:]), dtype=torch.float32, device=samples.device)
    _lib.call("matgcn_mc_quantiles_scaled", samples.data_ptr(), s, elems, n, od, levels, nq, C.byref(sc), out.data_ptr(),
              _stream(samples.device))
    return out


def mc_scores_nodes(samples: torch.Tensor, y: torch.Tensor, probs: Sequence[float], y_start: int = 0, mean=None,
                    std=None, group_mean=None, group_std=None, clamp_min: float = float("nan"),
                    truth_min: float = float("nan"), null_val: float = 0.0, min_s: float = 1e-4,
                    label_start: Optional[torch.Tensor] = None, sums: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(out, N, 5 + len(probs)) float64 device tensor: the sums of ``mc_scores`` per horizon AND node, on the scale of
    ``metric_sums_nodes`` (matgcn_mc_scores_nodes) - samples and labels de-scaled by mean / std and the per-node
    group_mean / group_std, samples clamped from below before the sort, labels <= ``truth_min`` left out.  Fixed order
    of summation: feeding batches through ``sums`` gives the bits of one call over all of them."""
    v = _label_view(samples, y, label_start, samples=True)
    dev, s = v.pred.device, int(v.pred.shape[0])
    levels, nq = _mc_probs(probs)
    sc, _keep = _metric_scale(v.n, dev, mean, std, group_mean, group_std, clamp_min, truth_min, min_s)
    need = C.c_size_t(0)
    _lib.call("matgcn_mc_scores_nodes_bytes", v.b, v.out, v.n, v.od, s, nq, C.byref(need))
    scratch = _scratch(_mc_scratch, ("mc_scores_nodes", v.b, v.out, v.n, v.od, s, nq), need.value, dev)
    sums, given = _out_arg(sums, (v.out, v.n, _lib.MC_SCORE_SUMS + nq), torch.float64, dev, "sums")
    _lib.call("matgcn_mc_scores_nodes", *v.args(y_start), C.byref(sc), float(null_val), levels, nq, scratch.data_ptr(),
              scratch.numel() * 8, sums.data_ptr(), int(given), _stream(dev))
    return sums


def mc_conformity(samples: torch.Tensor, y: torch.Tensor, probs: Sequence[float], y_start: int = 0, mean=None, std=None,
                  group_mean=None, group_std=None, clamp_min: float = float("nan"), truth_min: float = float("nan"),
                  min_s: float = 1e-4, null_val: float = 0.0, label_start: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, out, N, od) float32 device tensor of conformity scores max(Q_first - l, l - Q_last) of the ensemble ``samples``
    (S, B, out, N, od) against the labels, on the scale and with the label filters of ``mc_scores_nodes``
    (matgcn_mc_conformity); NaN where the label is masked or filtered out.  ``probs``: at least two levels, the outer two
    are the band.  ``out``: the tensor to write - a slice of a caller's store of scores."""
    v = _label_view(samples, y, label_start, samples=True)
    dev = v.pred.device
    levels, nq = _mc_probs(probs)
    sc, _keep = _metric_scale(v.n, dev, mean, std, group_mean, group_std, clamp_min, truth_min, min_s)
    out, _ = _out_arg(out, (v.b, v.out, v.n, v.od), torch.float32, dev, "out")
    _lib.call("matgcn_mc_conformity", *v.args(y_start), C.byref(sc), float(null_val), levels, nq, out.data_ptr(),
              _stream(dev))
    return out


CONFORMAL_GROUPINGS = {"horizon": 0, "element": 1}


def _conformal_store(scores: torch.Tensor, rows: int, grouping):
    """(scores, rows, out, cols, grouping code, shape of a per-group result) of a store of scores (capacity, out, ...)"""
    scores = _check_tensor(scores, "scores")
    if scores.dim() < 3:
        raise _lib.MatgcnError("scores has shape %s, expected (rows, out, N, od)" % (tuple(scores.shape),))
    rows = int(rows)
    if not 1 <= rows <= int(scores.shape[0]):
        raise _lib.MatgcnError("rows = %d outside the store's 1 .. %d" % (rows, int(scores.shape[0])))
    code = CONFORMAL_GROUPINGS.get(grouping, grouping)
    if code not in (0, 1):
        raise _lib.MatgcnError("grouping must be 'horizon' (0) or 'element' (1), got %r" % (grouping,))
    steps = int(scores.shape[1])
    return scores, rows, steps, scores[0, 0].numel(), code, tuple(scores.shape[1:]) if code else (steps,)


def conformal_quantile(scores: torch.Tensor, rows: int, grouping, coverage: float):
    """(margin float32, count int32), device tensors of shape (out,) - ``grouping`` "horizon" / 0 - or (out, N, od) -
    "element" / 1 - from the first ``rows`` rows of a store of conformity scores (capacity, out, N, od): count = the non-NaN
    scores of the group, margin = their k-th smallest, k = max(1, ceil((count + 1) * coverage)), +inf where k > count
    (matgcn_conformal_quantile: an exact radix select on the device)."""
    scores, rows, steps, cols, code, shape = _conformal_store(scores, rows, grouping)
    margin = torch.empty(shape, dtype=torch.float32, device=scores.device)
    count = torch.empty(shape, dtype=torch.int32, device=scores.device)
    _lib.call("matgcn_conformal_quantile", scores.data_ptr(), rows, steps, cols, code, float(coverage),
              margin.data_ptr(), count.data_ptr(), _stream(scores.device))
    return margin, count


def conformal_coverage(scores: torch.Tensor, rows: int, grouping, margin: torch.Tensor,
                       counts: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(*group shape, 2) int64 device tensor [valid scores, valid scores <= margin] per group over the first ``rows``
    rows of ``scores`` (matgcn_conformal_coverage); ``counts`` from earlier batches is added to."""
    scores, rows, steps, cols, code, shape = _conformal_store(scores, rows, grouping)
    margin = _check_tensor(margin, "margin")
    if tuple(margin.shape) != shape:
        raise _lib.MatgcnError("margin has shape %s, expected %s" % (tuple(margin.shape), shape))
    counts, given = _out_arg(counts, shape + (2,), torch.int64, scores.device, "counts")
    _lib.call("matgcn_conformal_coverage", scores.data_ptr(), rows, steps, cols, code, margin.data_ptr(),
              counts.data_ptr(), int(given), _stream(scores.device))
    return counts


def _region_groups(regions, n: int, device):
    if regions.num_nodes != n:
        raise _lib.MatgcnError("the region map covers %d nodes, the tensor has %d" % (regions.num_nodes, n))
    return regions.groups_on(device)


def group_sums(values: torch.Tensor, regions, mean=None, std=None, group_mean=None, group_std=None,
               clamp_min: float = float("nan"), out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Region totals of ``values`` (..., N, od) -> (..., G, od) (matgcn_group_sums): every member de-scaled by mean / std
    (scalars or one pair per node), then by the per-node group_mean / group_std, set to ``clamp_min`` where below it, and
    added in the order ``regions`` (a regions.RegionMap) lists it - one fp64 chain per total, rounded to float32 once.
    Each row is read once; the same bits every run.  ``out``: the tensor to write (every element is written)."""
    values = _check_tensor(values, "values")
    if values.dim() < 2:
        raise _lib.MatgcnError("values has shape %s, expected (..., N, od)" % (tuple(values.shape),))
    n, od = int(values.shape[-2]), int(values.shape[-1])
    groups = _region_groups(regions, n, values.device)
    rows = values.numel() // (n * od) if n * od else 0
    sc, _keep = _metric_scale(n, values.device, mean, std, group_mean, group_std, clamp_min, float("nan"), -1.0)
    out, _ = _out_arg(out, tuple(values.shape[:-2]) + (regions.num_groups, od), torch.float32, values.device, "out")
    _lib.call("matgcn_group_sums", values.data_ptr(), rows, n, od, C.byref(sc), C.byref(groups), out.data_ptr(),
              _stream(values.device))
    return out


def group_label_sums(y: torch.Tensor, regions, out_steps: int, out_dim: int, y_start: int = 0, mean=None, std=None,
                     group_mean=None, group_std=None, clamp_min: float = float("nan"),
                     label_start: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(B, out_steps, G, out_dim) region totals of the labels of a batch (matgcn_group_label_sums): ``y`` windows
    (B, y_steps, N, F), or with ``label_start`` (B) the resident series (T, N, F); channels y_start .. y_start+out_dim-1;
    arithmetic and order as ``group_sums``.  A NaN label makes the totals of its regions NaN."""
    if y.dim() not in (3, 4):
        raise _lib.MatgcnError("y has shape %s, expected (B, y_steps, N, F) or the series (T, N, F)" % (tuple(y.shape),))
    b = int(y.shape[0]) if label_start is None else int(label_start.shape[0])
    v = _label_view((b, int(out_steps), int(y.shape[-2]), int(out_dim)), y, label_start)
    dev = v.y.device
    out, _ = _out_arg(out, (v.b, v.out, regions.num_groups, v.od), torch.float32, dev, "out")
    groups = _region_groups(regions, v.n, dev)
    sc, _keep = _metric_scale(v.n, dev, mean, std, group_mean, group_std, clamp_min, float("nan"), -1.0)
    _lib.call("matgcn_group_label_sums", *v.args(y_start), C.byref(sc), C.byref(groups), out.data_ptr(), _stream(dev))
    return out


# ---- a training objective on region totals (matgcn_region_loss / matgcn_region_loss_grad) ---------------------------------
def _region_loss_call(v: _LabelView, regions, y_start, desc):
    """the value call: (scratch - it holds the totals for the gradient, so per call -, result (1 + out,))"""
    dev = v.pred.device
    groups = _region_groups(regions, v.n, dev)
    need = C.c_size_t()
    _lib.call("matgcn_region_loss_bytes", v.b, v.out, regions.num_groups, v.od, C.byref(need))
    scratch = torch.empty((need.value + 7) // 8, dtype=torch.float64, device=dev)
    result = torch.empty(1 + v.out, dtype=torch.float32, device=dev)
    _lib.call("matgcn_region_loss", *v.args(y_start), C.byref(desc), C.byref(groups), scratch.data_ptr(),
              scratch.numel() * 8, result.data_ptr(), _stream(dev))
    return scratch, result


def _region_loss_grad_call(v: _LabelView, regions, y_start, desc, scratch, upstream, base, d_pred):
    """the gradient call into ``d_pred``; ``base`` None, ``d_pred`` itself or another tensor of its shape"""
    dev = v.pred.device
    by_group, by_node = regions.groups_on(dev), regions.node_groups_on(dev)
    _lib.call("matgcn_region_loss_grad", *v.args(y_start), C.byref(desc), C.byref(by_group), C.byref(by_node),
              scratch.data_ptr(), scratch.numel() * 8, upstream.data_ptr(), _ptr(base), d_pred.data_ptr(), _stream(dev))
    return d_pred


def region_loss_device(pred: torch.Tensor, y: torch.Tensor, regions, y_start: int, mean: float, std: float, name: str,
                       delta=None, label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(1 + out,) tensor [the executor's objective ``name`` of the REGION TOTALS over all horizons, the same per horizon]
    (matgcn_region_loss): totals of the de-scaled prediction and label per region of ``regions`` (a regions.RegionMap),
    then the objective on them - masks act on totals.  Bit for bit train_loss_device(group_sums(pred), group_label_sums(y))
    with an identity affine.  Geometry as train_loss_device."""
    return _region_loss_call(_label_view(pred, y, label_start), regions, y_start,
                             train_loss_desc(name, mean, std, delta))[1]


def _weight_arg(v, name):
    v = float(v)
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError("%s = %r: expected a finite weight >= 0" % (name, v))
    return v


class _TractRegionLoss(torch.autograd.Function):
    """tract_weight * L(tracts) + region_weight * L(region totals), one gradient tensor: matgcn_loss_grad writes the tract
    half, matgcn_region_loss_grad adds the region half onto it (base = d_pred) - no add kernel, no temporary.  A weight of
    0 skips its half (``regions`` may then be None); a weight of 1 costs no multiplication.  train_loss is the (1, 0)
    case, region_train_loss the (0, 1) case."""

    @staticmethod
    def forward(ctx, pred, y, regions, y_start, desc, label_start, tract_weight, region_weight):
        if not (tract_weight > 0.0 or region_weight > 0.0):
            raise ValueError("tract_region_loss: both weights are 0")
        v = _label_view(pred.detach(), y, label_start)
        value, scratches = None, []
        for weight, call in ((tract_weight, lambda: _loss_call(v, y_start, desc)),
                             (region_weight, lambda: _region_loss_call(v, regions, y_start, desc))):
            if weight > 0.0:
                scratch, result = call()
                scratches.append(scratch)
                part = result[0] * weight if weight != 1.0 else result[0].clone()
                value = part if value is None else value + part
        ctx.view = v.save(ctx, *scratches)
        ctx.y_start, ctx.desc, ctx.regions = int(y_start), desc, regions
        ctx.weights = (tract_weight, region_weight)
        return value

    @staticmethod
    def backward(ctx, upstream):
        v, *scratches = ctx.view.saved(ctx)
        pred, (tw, rw) = v.pred, ctx.weights
        d_pred = torch.empty_like(pred)
        up = _upstream(upstream)
        if tw > 0.0:
            t_scratch = scratches.pop(0)
            up_t = up * tw if tw != 1.0 else up
            _lib.call("matgcn_loss_grad", *v.args(ctx.y_start), C.byref(ctx.desc), t_scratch.data_ptr(),
                      t_scratch.numel() * 8, up_t.data_ptr(), d_pred.data_ptr(), _stream(pred.device))
        if rw > 0.0:
            up_r = up * rw if rw != 1.0 else up
            _region_loss_grad_call(v, ctx.regions, ctx.y_start, ctx.desc, scratches.pop(0), up_r,
                                   d_pred if tw > 0.0 else None, d_pred)
        return d_pred, None, None, None, None, None, None, None


def tract_region_loss(pred: torch.Tensor, y: torch.Tensor, regions, y_start: int, mean: float, std: float, name: str,
                      delta=None, label_start: Optional[torch.Tensor] = None, tract_weight: float = 1.0,
                      region_weight: float = 1.0) -> torch.Tensor:
    """The autograd scalar  tract_weight * L(tracts) + region_weight * L(region totals)  of the executor's objective
    ``name`` (float32 device arithmetic): matgcn_loss and matgcn_region_loss forward; backward matgcn_loss_grad with
    upstream * tract_weight into the gradient, then matgcn_region_loss_grad with upstream * region_weight and that gradient
    as its base.  Fixed summation orders throughout: the same bits every run.  A weight of 0 skips its half."""
    tw, rw = _weight_arg(tract_weight, "tract_weight"), _weight_arg(region_weight, "region_weight")
    if tw == 0.0 and rw == 0.0:
        raise ValueError("tract_region_loss: both weights are 0")
    return _TractRegionLoss.apply(pred, y, regions, y_start, train_loss_desc(name, mean, std, delta), label_start, tw, rw)


def region_train_loss(pred: torch.Tensor, y: torch.Tensor, regions, y_start: int, mean: float, std: float, name: str,
                      delta=None, label_start: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The scalar of the objective ``name`` on the region totals with autograd support: matgcn_region_loss forward,
    matgcn_region_loss_grad backward (the region half of tract_region_loss alone)."""
    return tract_region_loss(pred, y, regions, y_start, mean, std, name, delta, label_start, 0.0, 1.0)


def _opt_tensor(t, name: str) -> torch.Tensor:
    """an optimizer tensor as the C ABI wants it - the caller's own memory, so nothing is copied or converted here"""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a tensor, got %s" % (name, type(t).__name__))
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU: the optimizer step is HIP-only (no CPU fallback)" % name)
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, got %s" % (name, t.dtype))
    if t.layout != torch.strided or not t.is_contiguous():
        raise ValueError("%s must be contiguous: the kernels update it in place, a copy would be lost" % name)
    return t


_opt_tables: Dict[tuple, tuple] = {}    # the pointers of a tensor set -> its matgcn_opt_tensor array (a loop re-uses one)


def _opt_table(grads, params=None, exp_avgs=None, exp_avg_sqs=None):
    """(matgcn_opt_tensor array, n, device) of a checked tensor set; grads alone for the norm"""
    cols = [grads] if params is None else [params, grads, exp_avgs, exp_avg_sqs]
    n = len(grads)
    if n < 1 or any(len(c) != n for c in cols):
        raise ValueError("the optimizer step needs at least one tensor and lists of one length, got %s"
                         % [len(c) for c in cols])
    try:   # everything the checks below look at, so that a hit may skip them
        key = tuple((t.data_ptr(), t.numel(), t.dtype, t.is_contiguous()) for c in cols for t in c)
    except (AttributeError, RuntimeError):   # not a tensor, or one without storage (sparse): named by the checks
        key = None
    hit = _opt_tables.get(key)
    if hit is not None:
        return hit
    names = ("grads",) if params is None else ("params", "grads", "exp_avgs", "exp_avg_sqs")
    dev = grads[0].device if isinstance(grads[0], torch.Tensor) else None
    for nm, c in zip(names, cols):
        for i, t in enumerate(c):
            _opt_tensor(t, "%s[%d]" % (nm, i))
            if t.device != dev:
                raise ValueError("%s[%d] is on %s, grads[0] on %s" % (nm, i, t.device, dev))
            if t.numel() != grads[i].numel():
                raise ValueError("%s[%d] has %d elements, grads[%d] %d" % (nm, i, t.numel(), i, grads[i].numel()))
    arr = (_lib.OptTensor * n)()
    for i in range(n):
        if params is not None:
            arr[i].param, arr[i].exp_avg, arr[i].exp_avg_sq = (params[i].data_ptr(), exp_avgs[i].data_ptr(),
                                                                exp_avg_sqs[i].data_ptr())
        arr[i].grad, arr[i].numel = grads[i].data_ptr(), grads[i].numel()
    if len(_opt_tables) >= 64:
        _opt_tables.clear()
    hit = (arr, n, dev)
    if key is not None:
        _opt_tables[key] = hit
    return hit


def grad_norm(tensors: Sequence[torch.Tensor]) -> torch.Tensor:
    """The 2-norm over all elements of ``tensors`` as a 0-dim float32 device tensor (matgcn_grad_norm): what
    clip_grad_norm_ returns, summed in fp64 in a fixed order - two launches, no host synchronisation."""
    arr, n, dev = _opt_table(list(tensors))
    need = C.c_size_t(0)
    _lib.call("matgcn_grad_norm_bytes", arr, n, C.byref(need))
    scratch = _scratch(_norm_scratch, (need.value,), need.value, dev)     # the per-chunk partials
    out = torch.empty((), dtype=torch.float32, device=dev)
    _lib.call("matgcn_grad_norm", arr, n, scratch.data_ptr(), need.value, out.data_ptr(), _stream(dev))
    return out


def adam_step(params, grads, exp_avgs, exp_avg_sqs, *, lr, betas, eps, weight_decay, step, max_norm=None,
              total_norm: Optional[torch.Tensor] = None) -> None:
    """One Adam update of ``params`` in place (matgcn_adam_step; torch's _single_tensor_adam order in fp32), ``step`` the
    1-based count after this update, common to all tensors.  With ``max_norm`` the gradients are scaled, as they are read,
    by min(1, max_norm / (total_norm + 1e-6)) - ``total_norm`` is grad_norm() over every gradient of the model, not only
    over the ones of this call; the ``grads`` themselves are never written."""
    arr, n, dev = _opt_table(list(grads), list(params), list(exp_avgs), list(exp_avg_sqs))
    clip = max_norm is not None and float(max_norm) > 0
    if max_norm is not None and not clip and not float(max_norm) <= 0:
        raise ValueError("max_norm = %r" % (max_norm,))
    if clip:
        if total_norm is None:
            raise ValueError("max_norm without total_norm: pass grad_norm() over every gradient of the model")
        _opt_tensor(total_norm, "total_norm")
        if total_norm.numel() != 1 or total_norm.device != dev:
            raise ValueError("total_norm must be one float on %s" % (dev,))
    hp = _lib.Adam(float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay),
                   float(max_norm) if clip else 0.0, int(step))
    _lib.call("matgcn_adam_step", arr, n, C.byref(hp), total_norm.data_ptr() if clip else None, _stream(dev))


def _walk_params(s: PathSpec, p: "_lib.Params", ptr_of) -> None:
    """Every tensor field of a matgcn_params / matgcn_grads ``p`` of configuration ``s``: field = ptr_of(name in the
    reference's state dict, shape); None leaves the field NULL.  static_supports is no state-dict tensor and not set here."""
    n, d, h, kt = s.nodes, s.embed_dim, s.hidden, s.k_total
    p.node_emb = ptr_of("node_emb", (n, d))
    if s.adpadj == "unidirection":      # the only adaptive adjacency that reads the two factors
        p.node_vec1, p.node_vec2 = ptr_of("node_vec1", (n, s.adj_rank)), ptr_of("node_vec2", (s.adj_rank, n))
    else:
        p.node_vec1 = p.node_vec2 = None
    p.weights_gru = ptr_of("encoder.weights_gru", (s.layers, s.in_steps))
    p.weight_tsg = ptr_of("weight_tsg", (s.n_ts,))
    for i in range(len(s.head_begin)):
        p.weight_ts[i] = ptr_of("weight_ts.%d" % i, (1, 24, n, s.out_dim))
    for l in range(s.layers):
        cin = (s.feat_in if l == 0 else h) + h
        if not s.gcn_off:
            for nm, o, dst in (("gate", 2 * h, p.gate), ("update", h, p.update)):
                pre = "encoder.agru_cells.%d.%s." % (l, nm)
                dst[l].weights_g = ptr_of(pre + "weights_g", (kt, 1, 1))
                dst[l].weights_pool = ptr_of(pre + "weights_pool", (d, kt, cin, o))
                dst[l].bias_pool = ptr_of(pre + "bias_pool", (d, o))
        # gcn_off: encoder.agru_cells hold the dense GRU cells; they travel in the res_* fields
        cells = "encoder.agru_cells" if s.gcn_off else "encoder.res_cells"
        for nm, o, dst in (("gate", 2 * h, p.res_gate), ("update", h, p.res_update)):
            pre = "%s.%d.%s." % (cells, l, nm)
            dst[l].weight = ptr_of(pre + "weight", (o, cin))
            dst[l].bias = ptr_of(pre + "bias", (o,))
    p.end_conv_weight = ptr_of("end_conv.weight", (s.out_window * s.out_dim, 1 if s.fnn_off else s.in_steps, 1, h))
    p.end_conv_bias = ptr_of("end_conv.bias", (s.out_window * s.out_dim,))


class HotPath:
    """One (spec, batch) binding.  Not thread-safe; uses torch's current stream at call time."""

    def __init__(self, spec: PathSpec, batch: int, device: torch.device):
        self.lib = _lib.load()
        self.spec, self.batch, self.device = spec, batch, torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MatgcnError("HotPath needs a GPU device, got %s" % self.device)
        self.dims = spec.dims(batch)
        self.prepared = self._buffer(self._bytes("matgcn_prepared_bytes"))
        self.workspace = self._buffer(self._bytes("matgcn_workspace_bytes"))
        self.params = _lib.Params()
        self._static = None
        self._keep: List[torch.Tensor] = []
        self._prepared_ok = False
        self._train = None
        self.train_generation = 0
        self.grad_bucket: Optional[torch.Tensor] = None   # flat buffer the gradients of the LAST backward() are views of
        # precision mode of this binding's calls (1 bf16 graph mixes, 2 + bf16 node-wise contractions, 3 graph mixes of the
        # inference forwards from three bf16 pieces - the training setter reads it as 0 -, 0 fp32): the
        # library settings are process-global, so every call sets the one it needs and restores the previous value
        # (matgcn_set_mix_precision for the inference forwards, matgcn_set_train_precision for the training step).
        # None (default): the calls leave the settings as they are - whatever the process set, fp32 unless it did.
        self.precision: Optional[int] = None
        # deterministic backward (matgcn_set_deterministic): True / False are set around this binding's training calls
        # and restored afterwards - around forward_train too, which sizes the train buffer with the partial slabs of the
        # ordered reductions -, None (default) leaves the process-wide setting as it is
        self.deterministic: Optional[bool] = None
        # three-piece training (matgcn_set_train_bf16x3: the graph mixes of the training step, both directions, from three
        # bf16 pieces per operand - fp32 accuracy; an explicit bf16 training mode, precision 1 or 2, wins over it): True /
        # False are set around forward_train - which sizes both buffers with the mode's planes - and backward and
        # restored afterwards, None (default) leaves the process-wide setting as it is
        self.train_bf16x3: Optional[bool] = None

    # ---- plumbing ------------------------------------------------------------------------------
    def _stream(self) -> int:
        return _stream(self.device)

    def _bytes(self, name: str) -> int:
        """what matgcn_prepared_bytes / matgcn_workspace_bytes / matgcn_train_bytes report under the current settings"""
        nbytes = C.c_size_t()
        _lib.call(name, C.byref(self.dims), C.byref(nbytes))
        return nbytes.value

    def _buffer(self, nbytes: int) -> torch.Tensor:
        return torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)

    def _out(self) -> torch.Tensor:
        """a fresh forecast (B, out_window, N, out_dim)"""
        s = self.spec
        return torch.empty(self.batch, s.out_window, s.nodes, s.out_dim, dtype=torch.float32, device=self.device)

    def _ws(self):
        # every call that uses the workspace invalidates what an earlier forward_train left there for its backward
        self.train_generation += 1
        return self.workspace.data_ptr(), self.workspace.numel() * 4

    def _status(self, name: str, tail, ws, wsb, train: bool = False, prepared: bool = True) -> int:
        """The status of entry point ``name`` on (dims, params, prepared - where it takes one -, *tail, the workspace
        ``ws`` of ``wsb`` bytes, the train buffer and its bytes - train -, the current stream)."""
        head = (self.prepared.data_ptr(),) if prepared else ()
        tr = (self._train.data_ptr(), self._train.numel() * 4) if train else ()
        return getattr(self.lib, name)(C.byref(self.dims), C.byref(self.params), *head, *tail, ws, wsb, *tr,
                                       _stream(self.device))

    def _call(self, name: str, *tail, regrow: bool = False, train: bool = False, prepared: bool = True) -> None:
        """``_status`` checked; regrow: through _with_workspace, which re-sizes a buffer that the current library mode
        has outgrown and repeats the call (the forwards; the single-step entry points take the workspace as it is)."""
        if regrow:
            self._with_workspace(lambda ws, wsb: self._status(name, tail, ws, wsb, train, prepared), name, train=train)
        else:
            _lib.check(self._status(name, tail, *self._ws(), train, prepared), name)

    def _with_workspace(self, call, what: str, train: bool = False) -> None:
        """Run ``call(ws_ptr, ws_bytes)``; a workspace that is too small for the CURRENT library mode - precision mode 2
        or 3 was switched on after this binding sized it: the bf16 weight-stream copies (mode 2) and the three bf16 planes
        of the support stack (mode 3) are counted only while their mode is set - is re-sized once and the call repeated (train: the train buffer too - matgcn_train_bytes counts the bf16
        copies of the plain weights while training precision mode 2 is set, and the planes of the plain support stack
        while the three-piece training switch is the effective mode)."""
        ws, wsb = self._ws()
        status = call(ws, wsb)
        if status == -4:      # MATGCN_ERR_SMALL_BUFFER
            grown = False
            nbytes = self._bytes("matgcn_workspace_bytes")
            if nbytes > self.workspace.numel() * 4:
                self.workspace = self._buffer(nbytes)
                grown = True
            if train and self._train is not None:
                if self._bytes("matgcn_train_bytes") > self._train.numel() * 4:
                    self._train = None
                    self._train_buffer()
                    grown = True
            if grown:
                ws, wsb = self._ws()
                status = call(ws, wsb)
        _lib.check(status, what)

    @contextlib.contextmanager
    def _mode(self, setter):
        """the library setting ``setter`` at this binding's precision for the calls inside (None: untouched)"""
        if self.precision is None:
            yield
            return
        prev = setter(int(self.precision))
        try:
            yield
        finally:
            setter(prev)

    def _det(self):
        """the library's deterministic-backward setting at this binding's value for the calls inside (None: untouched)"""
        return self._switch(self.lib.matgcn_set_deterministic, self.deterministic)

    def _x3(self):
        """the library's three-piece training switch at this binding's value for the calls inside (None: untouched)"""
        return self._switch(self.lib.matgcn_set_train_bf16x3, self.train_bf16x3)

    @contextlib.contextmanager
    def _switch(self, setter, value: Optional[bool]):
        if value is None:
            yield
            return
        prev = setter(1 if value else 0)
        try:
            yield
        finally:
            setter(prev)

    def bind(self, state: Dict[str, torch.Tensor], static_supports: Optional[torch.Tensor]):
        """Point matgcn_params at the tensors of a reference-named state dict."""
        s, p = self.spec, self.params
        keep: List[torch.Tensor] = []

        def dev(name, shape):
            t = _check_tensor(state[name], name, shape)
            keep.append(t)
            return t.data_ptr()

        _walk_params(s, p, dev)
        if s.n_static > 0:
            st = _check_tensor(static_supports, "static_supports", (s.n_static, s.nodes, s.nodes))
            keep.append(st)
            self._static = st
            p.static_supports = st.data_ptr()
        else:
            p.static_supports = None
        self._keep = keep
        self._prepared_ok = False

    # ---- entry points --------------------------------------------------------------------------
    def prepare(self):
        self._call("matgcn_prepare", self.prepared.numel() * 4)
        self._prepared_ok = True

    def _need_prepared(self):
        if not self._prepared_ok:
            self.prepare()

    def prepare_join(self):
        """the current stream waits for whatever a lazy matgcn_prepare still writes (include/matgcn.h): needed only by
        code that reads ``self.prepared`` itself instead of through the library"""
        _lib.call("matgcn_prepare_join", self._stream())

    def __del__(self):
        # `prepared` goes back to torch's allocator when this object dies: nothing of the library may still write it.
        # The lazy prepare's events live per DEVICE (the library picks them by hipGetDevice()), and the allocator reuses
        # the block in order of the stream it was allocated on: join on this binding's device and on that stream, and
        # additionally tell the allocator about the joining stream when it is another one (a join issued
        # under another current device / stream context landed on the wrong ones).
        try:
            if self._prepared_ok and torch.cuda.is_available():
                with torch.cuda.device(self.device):
                    cur = torch.cuda.current_stream(self.device)
                    self.lib.matgcn_prepare_join(cur.cuda_stream)
                    self.prepared.record_stream(cur)
        except Exception as exc:   # interpreter shutdown: torch may already be gone - say so instead of hiding it
            try:
                import warnings
                warnings.warn("HotPath.__del__: matgcn_prepare_join failed (%r)" % (exc,), RuntimeWarning)
            except Exception:
                pass

    def _source(self, x):
        """The batch of a call: a windows tensor X (B, x_steps, N, F), or a (series, label_start, rel_steps) triple - the
        raw series (T, N, F) resident on the device, B int32 label starts, the x_steps row offsets.
        Returns (X pointer or None, reference to a matgcn_series or None, objects to keep alive: X, or the contiguous
        series, label_start, the C array of rel_steps and the matgcn_series)."""
        s = self.spec
        if isinstance(x, torch.Tensor):
            x = _check_tensor(x, "X", (self.batch, s.x_steps, s.nodes, s.x_feat))
            return x.data_ptr(), None, (x,)
        series, label_start, rel_steps = x
        if series.dim() != 3 or tuple(series.shape[1:]) != (s.nodes, s.x_feat):
            raise _lib.MatgcnError("series has shape %s, expected (T, %d, %d)" % (tuple(series.shape), s.nodes, s.x_feat))
        series = _check_tensor(series, "series")
        if not label_start.is_cuda or label_start.dtype != torch.int32 or tuple(label_start.shape) != (self.batch,):
            raise _lib.MatgcnError("label_start must be a CUDA int32 tensor of shape (%d,)" % self.batch)
        rel = [int(v) for v in rel_steps]
        if len(rel) != s.x_steps:
            raise _lib.MatgcnError("rel_steps has %d entries, x_steps is %d" % (len(rel), s.x_steps))
        label_start = label_start.contiguous()
        rel_c = (C.c_int32 * len(rel))(*rel)
        src = _lib.Series(series.data_ptr(), int(series.shape[0]), label_start.data_ptr(), rel_c)
        return None, C.byref(src), (series, label_start, rel_c, src)

    def _h0(self, h0):
        """initial encoder state (L, B, N, H) or None = zeros (MultiATGCN.py:405-409)"""
        if h0 is None:
            return None
        s = self.spec
        return _check_tensor(h0, "h0", (s.layers, self.batch, s.nodes, s.hidden))

    def forward(self, x: torch.Tensor, h0: Optional[torch.Tensor] = None) -> torch.Tensor:
        s = self.spec
        x = _check_tensor(x, "X", (self.batch, s.x_steps, s.nodes, s.x_feat))
        h0 = self._h0(h0)
        self._need_prepared()
        out = self._out()
        with self._mode(self.lib.matgcn_set_mix_precision):
            self._call("matgcn_forward", x.data_ptr(), _ptr(h0), out.data_ptr(), regrow=True)
        return out

    # ---- training step ---------------------------------------------------
    def _train_buffer(self) -> torch.Tensor:
        """The train buffer, at least as large as matgcn_train_bytes reports under the CURRENT library settings (it
        counts the deterministic backward's partial slabs and mode 2's bf16 copies only while they are set): a buffer
        sized before a setting was switched on is replaced.  Called in front of forward_train, never between it and
        its backward - a new buffer has none of the saved activations."""
        nbytes = self._bytes("matgcn_train_bytes")
        if self._train is None or nbytes > self._train.numel() * 4:
            self._train = self._buffer(nbytes)
        return self._train

    def _mask_shape(self):
        s = self.spec
        return (self.batch, 1 if s.fnn_off else s.in_steps, s.nodes, s.hidden)

    def _mask(self, drop_mask):
        return None if drop_mask is None else _check_tensor(drop_mask, "drop_mask", self._mask_shape())

    @staticmethod
    def _dropout(dropout, drop_mask=None) -> Optional[_lib.Dropout]:
        """(seed, offset, p) -> matgcn_dropout, or None.  The range of p is the library's to check."""
        if dropout is None:
            return None
        if drop_mask is not None:
            raise _lib.MatgcnError("drop_mask and dropout = (seed, offset, p) exclude each other")
        seed, offset, p = dropout
        return _lib.Dropout(int(seed) & (2 ** 64 - 1), int(offset) & (2 ** 64 - 1), float(p))

    def dropout_mask(self, seed: int, offset: int, p: float) -> torch.Tensor:
        """The (B, headT, N, 64) mask the descriptor (seed, offset, p) stands for, written out by matgcn_dropout_mask
        (tests, and callers that want to look at it: the training and MC entry points never materialise it)."""
        mask = torch.empty(self._mask_shape(), dtype=torch.float32, device=self.device)
        d = self._dropout((seed, offset, p))
        _lib.call("matgcn_dropout_mask", C.byref(self.dims), C.byref(d), mask.data_ptr(), self._stream())
        return mask

    @staticmethod
    def _drop_variant(name: str, seeded, drop_mask):
        """the two training entry points differ in one argument: the mask tensor, or the descriptor that stands for it"""
        return (name, _ptr(drop_mask)) if seeded is None else (name + "_seeded", C.byref(seeded))

    def forward_train(self, x, drop_mask: Optional[torch.Tensor] = None,
                      h0: Optional[torch.Tensor] = None, dropout=None) -> torch.Tensor:
        """matgcn_forward that keeps the activations the backward needs (in the train buffer and the workspace).
        x: the windows tensor X, or a (series, label_start, rel_steps) triple (see _source).
        drop_mask: the (B, T, N, H) multipliers of the dropout in front of end_conv (training mode) or None;
        dropout: (seed, offset, p) instead - the same dropout drawn on the device by matgcn_forward_train_seeded, no mask
        tensor (the matching backward must get the same triple);
        h0: initial encoder state (L, B, N, H) or None."""
        xp, src, _keep = self._source(x)
        drop_mask = self._mask(drop_mask)
        seeded = self._dropout(dropout, drop_mask)
        h0 = self._h0(h0)
        self._need_prepared()
        out = self._out()
        with self._mode(self.lib.matgcn_set_train_precision), self._x3(), self._det():
            self._train_buffer()
            name, drop = self._drop_variant("matgcn_forward_train", seeded, drop_mask)
            self._call(name, xp, src, _ptr(h0), drop, out.data_ptr(), regrow=True, train=True)
        return out

    def forward_mc(self, x, h0: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0, p: float = 0.1,
                   samples: int = 32, keep_samples: bool = False):
        """Monte-Carlo dropout (matgcn_forward_mc): the eval-mode encoder once, the head over ``samples`` masks - sample
        s draws with (seed, offset + s, p).  x: the windows tensor X or a (series, label_start, rel_steps) triple.
        Returns (mean, std) of shape (B, out, N, od) - the population standard deviation over the samples - and, with
        keep_samples, the (samples, B, out, N, od) forecasts as a third entry."""
        xp, src, _keep = self._source(x)
        h0 = self._h0(h0)
        d = self._dropout((seed, offset, p))
        self._need_prepared()
        mean, std = self._out(), self._out()
        kept = None
        if keep_samples and 1 <= int(samples) <= _lib.MAX_MC_SAMPLES:
            kept = torch.empty((int(samples),) + tuple(mean.shape), dtype=torch.float32, device=self.device)
        with self._mode(self.lib.matgcn_set_mix_precision):
            self._call("matgcn_forward_mc", xp, src, _ptr(h0), C.byref(d), int(samples), mean.data_ptr(), std.data_ptr(),
                       _ptr(kept), regrow=True)
        return (mean, std, kept) if keep_samples else (mean, std)

    def _train_mc_buffer(self, samples: int) -> torch.Tensor:
        """the train buffer of the ensemble step: matgcn_train_mc_bytes covers matgcn_train_bytes of every setting"""
        nbytes = C.c_size_t()
        _lib.call("matgcn_train_mc_bytes", C.byref(self.dims), int(samples), C.byref(nbytes))
        if self._train is None or nbytes.value > self._train.numel() * 4:
            self._train = self._buffer(nbytes.value)
        return self._train

    def forward_train_mc(self, x, dropout, samples: int, h0: Optional[torch.Tensor] = None,
                         keep_stats: bool = False):
        """matgcn_forward_train_mc: forward_train without dropout - the same saved activations - and the head over
        ``samples`` masks, sample s drawn with (seed, offset + s, p) of ``dropout``.  Returns the (samples, B, out, N, od)
        forecasts, with keep_stats (samples, mean, std).  The matching backward is backward_mc."""
        xp, src, _keep = self._source(x)
        h0 = self._h0(h0)
        d = self._dropout(dropout)
        if d is None:
            raise _lib.MatgcnError("forward_train_mc needs dropout = (seed, offset, p)")
        samples = int(samples)
        self._need_prepared()
        valid = 1 <= samples <= _lib.MAX_MC_SAMPLES      # (the library refuses the others; nothing is sized for them)
        s = self.spec
        kept = torch.empty((samples if valid else 1, self.batch, s.out_window, s.nodes, s.out_dim), dtype=torch.float32,
                           device=self.device)
        mean, std = (self._out(), self._out()) if keep_stats else (None, None)
        with self._mode(self.lib.matgcn_set_train_precision), self._x3(), self._det():
            if valid:
                self._train_mc_buffer(samples)
            else:
                self._train_buffer()
            self._call("matgcn_forward_train_mc", xp, src, _ptr(h0), C.byref(d), samples, _ptr(mean), _ptr(std),
                       _ptr(kept), regrow=True, train=True)
        return (kept, mean, std) if keep_stats else kept

    D_H0 = "__d_h0__"   # key of the initial-state gradient in backward()'s result

    def _grad_views(self, state: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """Every gradient matgcn_backward returns is a view of ONE flat fp32 buffer (``grad_bucket``, 15.5 MB at
        N = 403), so that the gradient exchange of data-parallel training is a single all-reduce of that buffer with no
        concatenation or copy-back (torch autograd adopts the views as ``p.grad``).  Every call gets a buffer of its
        own from torch's caching allocator - gradients handed out earlier stay valid for as long as somebody holds
        them (gradient accumulation, zero_grad(set_to_none=False), callers that compare two backward results), and
        once they are dropped the allocator hands the same block back, so a training loop reuses one block anyway."""
        names = [k for k in state if not k.startswith("static_initial")]
        offs, total = {}, 0
        for k in names:
            offs[k] = total
            total += (state[k].numel() + 63) // 64 * 64        # every view starts on a 256-byte boundary
        bucket = self.grad_bucket = torch.zeros(total, dtype=torch.float32, device=self.device)
        return {k: bucket[offs[k]:offs[k] + state[k].numel()].view(state[k].shape) for k in names}

    def backward(self, x, d_out: torch.Tensor, state: Dict[str, torch.Tensor],
                 drop_mask: Optional[torch.Tensor] = None, h0: Optional[torch.Tensor] = None,
                 dropout=None) -> Dict[str, torch.Tensor]:
        """Gradients of every tensor of `state` (the dict bind() saw) that the loss depends on, keyed by the same
        names; must directly follow the matching forward_train (same workspace, same train buffer).  With h0 (the
        tensor forward_train saw) the result also holds its gradient (L, B, N, H) under HotPath.D_H0.  The library runs
        the backward in the precision mode of the matching forward_train, whatever the settings are now.
        dropout: the (seed, offset, p) triple the matching forward_train got (matgcn_backward_seeded), in place of
        drop_mask."""
        s = self.spec
        xp, src, _keep = self._source(x)
        d_out = _check_tensor(d_out, "d_out", (self.batch, s.out_window, s.nodes, s.out_dim))
        drop_mask = self._mask(drop_mask)
        seeded = self._dropout(dropout, drop_mask)
        h0 = self._h0(h0)
        name, drop = self._drop_variant("matgcn_backward", seeded, drop_mask)
        return self._backward_call(name, (xp, src, _ptr(h0), drop, d_out.data_ptr()), state, h0)

    def backward_mc(self, x, d_samples: torch.Tensor, state: Dict[str, torch.Tensor], dropout,
                    h0: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
        """matgcn_backward_mc behind forward_train_mc (same x, dropout triple and h0): the gradients of ``backward`` summed
        over the samples, from ``d_samples`` (samples, B, out, N, od) - the encoder's backward runs once."""
        s = self.spec
        xp, src, _keep = self._source(x)
        if d_samples.dim() != 5:
            raise _lib.MatgcnError("d_samples has shape %s, expected (S, B, out, N, od)" % (tuple(d_samples.shape),))
        d_samples = _check_tensor(d_samples, "d_samples",
                                  (d_samples.shape[0], self.batch, s.out_window, s.nodes, s.out_dim))
        d = self._dropout(dropout)
        if d is None:
            raise _lib.MatgcnError("backward_mc needs the dropout = (seed, offset, p) of its forward_train_mc")
        h0 = self._h0(h0)
        return self._backward_call("matgcn_backward_mc", (xp, src, _ptr(h0), C.byref(d), int(d_samples.shape[0]),
                                                          d_samples.data_ptr()), state, h0)

    def _backward_call(self, entry: str, lead: tuple, state: Dict[str, torch.Tensor], h0) -> Dict[str, torch.Tensor]:
        """What backward and backward_mc share: the gradient views and their routing, the call - entry point ``entry`` on
        (*lead, grads, d_h0) - on the workspace and the train buffer as the forward left them."""
        s = self.spec
        d_h0 = torch.empty_like(h0) if h0 is not None else None
        grads: Dict[str, torch.Tensor] = {}
        g = _lib.Params()
        views = self._grad_views(state)
        # fields left NULL: under gcn_off what only the graph cells read, otherwise a node_emb that is a frozen Parameter
        if s.gcn_off:
            skip = ("node_emb", "node_vec1", "node_vec2", "encoder.weights_gru")
        else:
            emb = state["node_emb"]
            skip = () if emb.requires_grad or not isinstance(emb, torch.nn.Parameter) else ("node_emb",)

        def new(name, shape):
            if name in skip:
                return None
            grads[name] = views[name]
            return views[name].data_ptr()

        _walk_params(s, g, new)
        if not s.scale_by_g and not s.gcn_off:   # the stack is not scaled: weights_g does not reach the output
            for l in range(s.layers):
                for nm in ("gate", "update"):
                    grads["encoder.agru_cells.%d.%s.weights_g" % (l, nm)].zero_()
        for name, t in state.items():    # tensors the forward never reads (unused heads, node_vec* without
            if name.startswith("static_initial"):   # host-side torch layers (MultiATGCN.py:288-290, 336-338): not ours
                continue
            if name not in grads and (t.requires_grad or not isinstance(t, torch.nn.Parameter)):   # adaptive adjacency)
                grads[name] = views[name].zero_()
        if self._train is None:
            raise _lib.MatgcnError("backward() without a forward_train() before it")
        # the workspace and the train buffer as forward_train left them: no re-sizing here - a deterministic backward
        # behind a forward_train that ran without the setting reports MATGCN_ERR_SMALL_BUFFER
        with self._x3(), self._det():
            status = self._status(entry, lead + (C.byref(g), _ptr(d_h0)), *self._ws(), train=True)
        _lib.check(status, entry)
        if d_h0 is not None:
            grads[self.D_H0] = d_h0
        return grads

    def forward_series(self, series: torch.Tensor, label_start: torch.Tensor, rel_steps,
                       h0: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward fed from the device-resident series (T, N, F): sample b's window rows are gathered by the
        head-fusion prologue from series[label_start[b] + rel_steps[s]] (multistgraph_amd/windows.py)."""
        _, _, (series, label_start, rel_c, _src) = self._source((series, label_start, rel_steps))
        h0 = self._h0(h0)
        self._need_prepared()
        out = self._out()
        with self._mode(self.lib.matgcn_set_mix_precision):
            self._call("matgcn_forward_series", series.data_ptr(), int(series.shape[0]), label_start.data_ptr(), rel_c,
                       _ptr(h0), out.data_ptr(), regrow=True)
        return out

    def fuse_heads(self, x: torch.Tensor) -> torch.Tensor:
        s = self.spec
        x = _check_tensor(x, "X", (self.batch, s.x_steps, s.nodes, s.x_feat))
        out = torch.empty(self.batch, s.in_steps, s.nodes, s.feat_in, dtype=torch.float32, device=self.device)
        self._call("matgcn_fuse_heads", x.data_ptr(), out.data_ptr(), prepared=False)
        return out

    def _single(self, name, layer, x, h, out_cols):
        s = self.spec
        cl = s.feat_in if layer == 0 else s.hidden
        x = _check_tensor(x, "x", (self.batch, s.nodes, cl))
        h = _check_tensor(h, "h", (self.batch, s.nodes, s.hidden))
        self._need_prepared()
        out = torch.empty(self.batch, s.nodes, out_cols, dtype=torch.float32, device=self.device)
        self._call(name, layer, x.data_ptr(), h.data_ptr(), out.data_ptr())
        return out

    def agcn_gate(self, layer, x, h):
        return self._single("matgcn_agcn_gate_fwd", layer, x, h, 2 * self.spec.hidden)

    def atgru_cell(self, layer, x, h):
        return self._single("matgcn_atgru_cell_fwd", layer, x, h, self.spec.hidden)

    def res_cell(self, layer, x, h):
        return self._single("matgcn_res_cell_fwd", layer, x, h, self.spec.hidden)

    def encoder(self, x0: torch.Tensor, h0: Optional[torch.Tensor] = None):
        s = self.spec
        x0 = _check_tensor(x0, "x0", (self.batch, s.in_steps, s.nodes, s.feat_in))
        h0 = self._h0(h0)
        self._need_prepared()
        seq = torch.empty(self.batch, s.in_steps, s.nodes, s.hidden, dtype=torch.float32, device=self.device)
        fin = torch.empty(s.layers, self.batch, s.nodes, s.hidden, dtype=torch.float32, device=self.device)
        self._call("matgcn_encoder_fwd", x0.data_ptr(), _ptr(h0), seq.data_ptr(), fin.data_ptr())
        return seq, fin

    def output_head(self, seq: torch.Tensor) -> torch.Tensor:
        s = self.spec
        seq = _check_tensor(seq, "seq", (self.batch, s.in_steps, s.nodes, s.hidden))
        self._need_prepared()
        out = self._out()
        self._call("matgcn_output_head", seq.data_ptr(), out.data_ptr())
        return out

    def _layout(self, name: str, *which):
        """the four integers of matgcn_supports_layout / matgcn_weights_layout, behind a joined prepare"""
        self._need_prepared()
        self.prepare_join()
        lay = (C.c_int64 * 4)()
        _lib.call(name, C.byref(self.dims), *which, C.byref(lay))
        return (int(v) for v in lay)

    def supports(self) -> torch.Tensor:
        """(Ks, N, N): the DENSE non-identity slots of the support stack as matgcn_prepare built them, in stack order
        (tests).  Diagonal supports never reach the stack - they are folded into the identity slot of the node-adaptive
        weights (read those back with node_weights) -, and cheb_order = 1 holds the SUM of its dense supports."""
        off, ld, npad, ks = self._layout("matgcn_supports_layout")
        n = self.spec.nodes
        if ks == 0:
            return torch.empty(0, n, n, dtype=torch.float32, device=self.device)
        st = self.prepared[off:off + npad * ld].view(npad, ld)
        return torch.stack([st[:n, k * npad:k * npad + n].t() for k in range(ks)], 0).contiguous()

    def node_weights(self, layer: int, part: int) -> torch.Tensor:
        """(N, 1 + Ks, 64, O): the recurrent (hidden-channel) rows of the node-adaptive weights of
        agru_cells[layer].gate (part 0, O = 128) / .update (part 1, O = 64), decoded from the MFMA-fragment-ordered
        stream matgcn_prepare wrote into `prepared` (tests: softmax(weights_g) and the diagonal-support fold included)."""
        off, stride, groups, ot = self._layout("matgcn_weights_layout", layer, part)
        n, o_dim = self.spec.nodes, ot * 16
        idx = torch.arange(n, device=self.device)[:, None] * stride + off + \
            torch.arange(groups * ot * 256, device=self.device)[None, :]
        frag = self.prepared[idx].view(n, groups, ot, 4, 16, 4)      # [n][g][ct][kq][j][s]
        # row kk = 16 g + 4 kq + s, column o = 16 ct + j
        w = frag.permute(0, 1, 3, 5, 2, 4).reshape(n, groups * 16, o_dim)
        return w.view(n, groups // 4, 64, o_dim).contiguous()
