"""Drop-in ``MultiATGCN`` plugin whose forward runs on the HIP hot path (libmatgcn.so).

Mirrors the reference's model-plugin surface for this path - same class name, constructor
signature, config / data_feature keys, parameter names and shapes (= checkpoint ABI), and the
``forward / predict / calculate_loss`` methods the LibCity executor calls
(reference libcity/model/traffic_flow_prediction/MultiATGCN.py:221-430,
libcity/model/abstract_traffic_state_model.py:4-29).  The arithmetic of ``forward`` is NOT here:
it is one call into the C ABI (include/matgcn.h); this module only owns parameters and plumbing.

There is no CPU or PyTorch fallback: a CPU tensor, a missing library or an unsupported option
raises.  See INTEGRATION.md for the one-line change that makes the reference's registry resolve
this class.
"""
from __future__ import annotations

import math
from collections import OrderedDict
from logging import getLogger
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import graph_prep
from . import hidden_pad
from .ops import (HotPath, PathSpec, diagonal_mask, group_sums, masked_mae_device, masked_mae_loss, mc_quantiles,
                  mc_quantiles_scaled, mc_scores, spec_from_config, train_loss_desc, train_loss_device)
from .ops import tract_region_loss
from .ops import crps_loss, crps_loss_device
from ._lib import MAX_MC_SAMPLES
from .ops import train_loss as train_loss_autograd
from .regions import RegionMap

try:  # inside a LibCity checkout: subclass the real plugin base so isinstance checks hold
    from libcity.model.abstract_traffic_state_model import AbstractTrafficStateModel  # type: ignore
except Exception:  # standalone: same two-level base (abstract_model.py:4-7, abstract_traffic_state_model.py:4-9)
    class AbstractModel(nn.Module):
        def __init__(self, config, data_feature):
            nn.Module.__init__(self)

        def predict(self, batch):
            raise NotImplementedError

        def calculate_loss(self, batch):
            raise NotImplementedError

    class AbstractTrafficStateModel(AbstractModel):
        def __init__(self, config, data_feature):
            self.data_feature = data_feature
            super().__init__(config, data_feature)


def _train_regions(value, num_nodes: int) -> Optional[RegionMap]:
    """config['hip_train_regions'] as a RegionMap over the model's nodes: a RegionMap, its state_dict(), or one region
    label per node; None stays None"""
    if value is None:
        return None
    if isinstance(value, RegionMap):
        regions = value
    elif isinstance(value, dict):
        regions = RegionMap.from_state_dict(value)
    else:
        labels = list(value)
        if len(labels) != num_nodes:
            raise ValueError("hip_train_regions: %d labels for %d nodes" % (len(labels), num_nodes))
        regions = RegionMap(num_nodes, labels=labels)
    if regions.num_nodes != num_nodes:
        raise ValueError("hip_train_regions covers %d nodes, the model has %d" % (regions.num_nodes, num_nodes))
    return regions


def _loss_weight(value, key: str) -> float:
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise ValueError("%s = %r: expected a number" % (key, value)) from None
    if not (math.isfinite(v) and v >= 0.0):
        raise ValueError("%s = %r: expected a finite weight >= 0" % (key, value))
    return v


def masked_mae(preds: torch.Tensor, labels: torch.Tensor, null_val=float("nan"), min_s: float = 1e-4):
    """loss.masked_mae_torch (reference libcity/model/loss.py:17-29), including its in-place
    zeroing of small labels."""
    labels[torch.abs(labels) < min_s] = 0
    mask = ~torch.isnan(labels) if (isinstance(null_val, float) and math.isnan(null_val)) else labels.ne(null_val)
    mask = mask.float()
    mask = mask / torch.mean(mask)
    mask = torch.where(torch.isnan(mask), torch.zeros_like(mask), mask)
    loss = torch.abs(preds - labels) * mask
    loss = torch.where(torch.isnan(loss), torch.zeros_like(loss), loss)
    return torch.mean(loss)


class _GraphConvParams(nn.Module):
    """Parameter holder named like the reference AGCN (MultiATGCN.py:59-73)."""

    def __init__(self, dim_in, dim_out, k_total, embed_dim):
        super().__init__()
        self.weights_g = nn.Parameter(torch.empty(k_total, 1, 1))
        self.weights_pool = nn.Parameter(torch.empty(embed_dim, k_total, dim_in, dim_out))
        self.bias_pool = nn.Parameter(torch.empty(embed_dim, dim_out))


class _GraphCellParams(nn.Module):
    """ATGRUCell parameter tree: .gate / .update (MultiATGCN.py:112-118)."""

    def __init__(self, dim_in, hidden, k_total, embed_dim):
        super().__init__()
        self.gate = _GraphConvParams(dim_in + hidden, 2 * hidden, k_total, embed_dim)
        self.update = _GraphConvParams(dim_in + hidden, hidden, k_total, embed_dim)


class _DenseCellParams(nn.Module):
    """Residual GRUCell parameter tree: two nn.Linear (MultiATGCN.py:134-140)."""

    def __init__(self, dim_in, hidden):
        super().__init__()
        self.gate = nn.Linear(dim_in + hidden, 2 * hidden)
        self.update = nn.Linear(dim_in + hidden, hidden)


class _EncoderParams(nn.Module):
    """ATGRUEncoder parameter tree (MultiATGCN.py:156-186)."""

    def __init__(self, layers, in_steps, feat_in, hidden, k_total, embed_dim, gcn_off=False):
        super().__init__()
        self.agru_cells = nn.ModuleList()
        self.res_cells = nn.ModuleList()
        self.weights_gru = nn.Parameter(torch.empty(layers, in_steps))
        for l in range(layers):
            cin = feat_in if l == 0 else hidden
            if gcn_off:   # dense GRU cells take the place of the graph cells, no residual cells (:187-192)
                self.agru_cells.append(_DenseCellParams(cin, hidden))
            else:
                self.agru_cells.append(_GraphCellParams(cin, hidden, k_total, embed_dim))
                self.res_cells.append(_DenseCellParams(cin, hidden))


def _is_series_batch(batch) -> bool:
    """a batch of the resident-series loader (multistgraph_amd.dataset.ResidentBatch), or a plain dict with the same
    two entries: the device-resident raw series and B label starts instead of materialised windows.  (No ``in`` on
    foreign objects: the reference's Batch has no __contains__ and raises KeyError on the fallback protocol.)"""
    from .dataset import ResidentBatch
    if isinstance(batch, ResidentBatch):
        return True
    return isinstance(batch, dict) and "label_start" in batch and "series" in batch


# config['hip_precision'] -> matgcn_set_*_precision mode ("bf16x3": an inference mode - the training setting reads 3 as 0;
# "bf16x3_train": the same inference mode, and matgcn_set_train_bf16x3 around the training steps)
HIP_PRECISIONS = {"fp32": 0, "bf16_mix": 1, "bf16": 2, "bf16x3": 3, "bf16x3_train": 3}
HIP_TRAIN_BF16X3 = ("bf16x3_train",)


def _precision_mode(name) -> int:
    if name not in HIP_PRECISIONS:
        raise ValueError("hip_precision = %r: expected one of %s" % (name, ", ".join(sorted(HIP_PRECISIONS))))
    return HIP_PRECISIONS[name]


# config['hip_dropout']: where the training-mode dropout in front of end_conv (:416) is drawn
HIP_DROPOUTS = ("torch", "device")
DROPOUT_P = 0.1   # F.dropout(output, p=0.1) (:416): the reference hard-codes it


def _torch_deterministic() -> bool:
    return bool(torch.are_deterministic_algorithms_enabled())


class _TrainStep(torch.autograd.Function):
    """autograd node of one training-mode forward: matgcn_forward_train / matgcn_backward.
    The parameters ride along as inputs so that autograd routes their gradients; X gets none (the reference
    never differentiates w.r.t. the batch).  The backward runs in the precision mode of its forward (the library
    records it per train buffer)."""

    @staticmethod
    def forward(ctx, path, x, drop_mask, h0, names, *params):
        # drop_mask: the mask tensor torch drew, or - config['hip_dropout'] = "device" - the (seed, offset, p) triple the
        # kernels draw it from (the backward gets the same one), or None
        h0 = None if h0 is None else h0.detach()
        ctx.dropout = drop_mask if isinstance(drop_mask, tuple) else None
        if ctx.dropout is not None:
            drop_mask = None
        out = path.forward_train(x, drop_mask, h0, dropout=ctx.dropout)
        ctx.path, ctx.x, ctx.mask, ctx.names, ctx.h0 = path, x, drop_mask, names, h0
        ctx.params = params
        ctx.generation = path.train_generation
        return out

    @staticmethod
    def backward(ctx, d_out):
        path = ctx.path
        if path.train_generation != ctx.generation:
            raise RuntimeError("MultiATGCN backward: another forward ran on this model between this forward and its "
                               "backward; the saved activations live in the shared workspace (one graph at a time)")
        state = {k: p for k, p in zip(ctx.names, ctx.params)}
        # (no precision setting here: the library runs the backward in the mode its forward_train ran with)
        grads = path.backward(ctx.x, d_out.contiguous(), state, ctx.mask, ctx.h0, dropout=ctx.dropout)
        # the initial state (static features, :406-409) gets its gradient back: torch autograd carries it on through
        # expand() and static_initial_gru
        return (None, None, None, grads.get(path.D_H0), None) + tuple(grads.get(k) if p.requires_grad else None
                                                                      for k, p in zip(ctx.names, ctx.params))


class _TrainStepMc(torch.autograd.Function):
    """autograd node of one ensemble training forward, beside _TrainStep: matgcn_forward_train_mc returns the samples
    (S, B, out, N, od) drawn at offsets offset .. offset + S - 1 of the (seed, offset, p) triple, matgcn_backward_mc takes
    their gradient - the encoder runs once in both directions.  Generation check and parameter routing as _TrainStep."""

    @staticmethod
    def forward(ctx, path, x, dropout, samples, h0, names, *params):
        h0 = None if h0 is None else h0.detach()
        out = path.forward_train_mc(x, dropout, samples, h0)
        ctx.path, ctx.x, ctx.dropout, ctx.names, ctx.h0 = path, x, dropout, names, h0
        ctx.params = params
        ctx.generation = path.train_generation
        return out

    @staticmethod
    def backward(ctx, d_samples):
        path = ctx.path
        if path.train_generation != ctx.generation:
            raise RuntimeError("MultiATGCN backward: another forward ran on this model between this forward and its "
                               "backward; the saved activations live in the shared workspace (one graph at a time)")
        state = {k: p for k, p in zip(ctx.names, ctx.params)}
        grads = path.backward_mc(ctx.x, d_samples.contiguous(), state, ctx.dropout, ctx.h0)
        return (None, None, None, None, grads.get(path.D_H0), None) + tuple(grads.get(k) if p.requires_grad else None
                                                                            for k, p in zip(ctx.names, ctx.params))


CRPS_LOSS = "crps"          # config['hip_train_loss']: the CRPS of a Monte-Carlo-dropout ensemble (ops.crps_loss)
CRPS_NULL_VAL = 0.0         # its mask: calculate_loss's and score_mc's null value


def _train_samples(value, key: str = "hip_train_samples") -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 1 <= int(value) <= MAX_MC_SAMPLES:
        raise ValueError("%s = %r: expected an int from 1 to %d" % (key, value, MAX_MC_SAMPLES))
    return int(value)


class MultiATGCN(AbstractTrafficStateModel):
    def __init__(self, config, data_feature):
        super().__init__(config, data_feature)
        get = config.get
        self.num_nodes = data_feature.get("num_nodes", 1)
        self.input_window = get("input_window", 1)
        self.output_window = get("output_window", 1)
        self.add_time_in_day = get("add_time_in_day", False)
        self.add_day_in_week = get("add_day_in_week", False)
        self.node_specific_off = get("node_specific_off", False)
        self.fnn_off = get("fnn_off", False)
        self.gcn_off = get("gcn_off", False)
        # operand precision of the HIP kernels (not a reference key): "fp32" (default) | "bf16_mix" (bf16 operands for the
        # graph mixes) | "bf16" (also for the node-wise contractions) | "bf16x3" (the graph mixes of the inference forwards
        # from three bf16 pieces per operand: fp32 accuracy on the bf16 matrix instruction; training steps of such a model
        # run in fp32) | "bf16x3_train" (as "bf16x3", and the graph mixes of the training step - forward and transposed -
        # from three bf16 pieces as well); fp32 accumulation and fp32 state, parameters and gradients in every mode.  Applies to this model's
        # inference forwards and training steps; an attribute, so a model can train in bf16 and evaluate in fp32 by
        # reassigning it.
        self.hip_precision = get("hip_precision", "fp32")
        _precision_mode(self.hip_precision)
        # config['hip_deterministic']: bit-reproducible gradients on the HIP path (matgcn_set_deterministic: the backward's
        # sums in a fixed order instead of fp32 atomics).  None (default) follows torch.are_deterministic_algorithms_enabled()
        # at every training step; True / False force it.  An attribute, not a parameter: state_dict and checkpoints are
        # unchanged.
        self.hip_deterministic = get("hip_deterministic", None)
        if self.hip_deterministic not in (None, True, False):
            raise ValueError("hip_deterministic = %r: expected None, True or False" % (self.hip_deterministic,))
        # config['hip_dropout']: "torch" (default) - the training-mode dropout mask is a tensor F.dropout draws from torch's
        # generator; "device" - it is drawn inside the HIP kernels that apply it from a counter-based generator
        # (matgcn_forward_train_seeded / matgcn_backward_seeded): no mask tensor, nothing taken from torch's generator.
        # Seed: torch.initial_seed(); offset: a per-model counter that advances by one per training forward (and by
        # `samples` per predict_mc without an explicit seed), inside an initialised process group (rank << 40) | counter,
        # so ranks draw different masks.  An attribute like the two above: checkpoints are unchanged.
        self.hip_dropout = get("hip_dropout", "torch")
        if self.hip_dropout not in HIP_DROPOUTS:
            raise ValueError("hip_dropout = %r: expected one of %s" % (self.hip_dropout, ", ".join(HIP_DROPOUTS)))
        self._dropout_counter = 0
        # config['hip_train_loss']: "none" (default) - calculate_loss / calculate_loss_series are the reference's masked MAE;
        # one of the executor's eleven differentiable objectives (ops.TRAIN_LOSSES: mae, mse, rmse, mape, logcosh, huber,
        # quantile, masked_mae, masked_mse, masked_rmse, masked_mape) - both return that objective instead, value and
        # gradient on the device (matgcn_loss / matgcn_loss_grad), so the reference's executor with `train_loss: none` trains
        # on it unchanged.  config['hip_train_loss_delta']: huber's knee / quantile's level (None: the reference's defaults,
        # 1.0 and 0.25).  Attributes like the three above: checkpoints are unchanged.
        self.hip_train_loss = str(get("hip_train_loss", "none")).lower()
        self.hip_train_loss_delta = get("hip_train_loss_delta", None)
        if self.hip_train_loss not in ("none", CRPS_LOSS):
            train_loss_desc(self.hip_train_loss, 0.0, 1.0, self.hip_train_loss_delta)   # ValueError on a bad name or delta
        # "crps": calculate_loss / calculate_loss_series return the mean CRPS of an ensemble of config['hip_train_samples']
        # (1 .. 1024, default 16) dropout samples - one encoder pass in both directions, the head over the samples
        # (matgcn_forward_train_mc / matgcn_crps_loss / matgcn_backward_mc).  A step consumes that many dropout offsets.
        # The masks of S samples cannot come from torch's generator: "crps" needs hip_dropout = "device".
        self.hip_train_samples = _train_samples(get("hip_train_samples", 16))
        if self.hip_train_loss == CRPS_LOSS and self.hip_dropout != "device":
            raise ValueError("hip_train_loss = 'crps' needs hip_dropout = 'device' (a torch-drawn mask cannot serve "
                             "hip_train_samples samples), got hip_dropout = %r" % self.hip_dropout)
        # config['hip_train_regions']: a regions.RegionMap, its state_dict() or one region label per node;
        # config['hip_region_loss_weight'] (default 0.0 = off) and config['hip_tract_loss_weight'] (default 1.0): with a
        # region weight > 0 calculate_loss / calculate_loss_series return
        #   tract_weight * L(tracts) + region_weight * L(region totals)
        # with L = hip_train_loss ("none": masked_mae through matgcn_loss) on both levels, value and gradient on the device
        # (ops.tract_region_loss: matgcn_region_loss / matgcn_region_loss_grad).  Without the keys, or with weight 0,
        # calculate_loss and its gradients keep their bits.  Attributes like the ones above: checkpoints are unchanged.
        self.hip_train_regions = _train_regions(get("hip_train_regions", None), self.num_nodes)
        self.hip_region_loss_weight = _loss_weight(get("hip_region_loss_weight", 0.0), "hip_region_loss_weight")
        self.hip_tract_loss_weight = _loss_weight(get("hip_tract_loss_weight", 1.0), "hip_tract_loss_weight")
        if self.hip_train_loss == CRPS_LOSS and self.hip_train_regions is not None:
            raise NotImplementedError("hip_train_loss = 'crps' with hip_train_regions: the CRPS of region totals is not built")
        if self.hip_region_loss_weight > 0.0 and self.hip_train_regions is None:
            raise ValueError("hip_region_loss_weight = %r needs a region map: set hip_train_regions"
                             % self.hip_region_loss_weight)
        self.batch_size = get("batch_size", 64)
        self.device = get("device", torch.device("cpu"))
        config["num_nodes"] = self.num_nodes  # the reference writes this back (:233)
        self.embed_dim_node = get("embed_dim_node", 10)
        self.embed_dim_adj = get("embed_dim_adj", 10)
        self.adpadj = get("adpadj", "bidirection")
        self.adjtype = get("adjtype", "od")
        self.cheb_order = get("cheb_order", 2)
        self.start_dim = get("start_dim", 0)
        self.end_dim = get("end_dim", 1)
        self.load_dynamic = get("load_dynamic", False)
        self.hidden_dim = get("rnn_units", 64)
        if self.hidden_dim > hidden_pad.WIDTH:
            raise NotImplementedError("rnn_units = %d: the HIP kernels hold 64 hidden channels; narrower models run on "
                                      "them zero-padded (hidden_pad.py), wider ones are not built" % self.hidden_dim)
        self._padded = self.hidden_dim < hidden_pad.WIDTH   # parameters keep the reference's shapes; the kernels see 64
        self.num_layers = get("num_layers", 2)
        assert self.num_layers >= 1, "At least one recurrent layer in the encoder"
        if self.add_day_in_week and not self.add_time_in_day:
            raise ValueError("add_day_in_week without add_time_in_day is undefined in the reference (:313-318)")
        static = data_feature.get("static", None)
        if self.input_window != 24:
            raise ValueError("the reference fuses 24-step heads (:373-393): input_window must be 24")
        embed_dim_cfg = self.embed_dim_node
        if self.node_specific_off:
            self.embed_dim_node = 1     # what the encoder's AGCN pools see (:166); node_emb itself shrinks after init

        # ---- one-off host graph prep (:238-283) -> first-order static supports (fp32, host)
        mats = graph_prep.build_static_supports(data_feature.get("adj_mx"), data_feature.get("coordinate"),
                                                None if static is None else np.asarray(static), self.adjtype)
        use_static = self.adpadj == "none" or self.adjtype == "multi"  # (:87-93)
        self._static_host = torch.from_numpy(np.stack(mats, 0)) if use_static else None
        self._static_dev: Optional[torch.Tensor] = None

        # ---- parameters, registered in the reference's order with the reference's names (:285-344)
        n = self.num_nodes
        rank = min(n, self.embed_dim_adj)  # torch.svd(adj)[..][:, :embed_dim_adj] (:299-304)
        # Every step below that consumes torch's global RNG does so in the reference's order, so that the same
        # torch.manual_seed gives bit-identical initial weights: the randn of (:296) - drawn at the CONFIG width even
        # under node_specific_off (the reference shrinks its own embed_dim_node only at :351) -, the nn.Linear /
        # Conv2d constructors, then _init_parameters over parameters() in registration order.
        # With static features (add_static, :286-294): static_initial_node is registered first (it stays in the
        # state_dict although forward never uses it), torch.pca_lowrank draws from the generator, and node_emb starts
        # from static_initial_node(static @ v) - only to be re-initialised by _init_parameters like everything else.
        self._static_q = min(n, embed_dim_cfg)
        if static is not None:
            st = torch.as_tensor(np.asarray(static), dtype=torch.float32)
            self.register_buffer("static", st, persistent=False)   # follows model.to(device); not in the state_dict
            self.static_initial_node = nn.Sequential(OrderedDict(
                [("embd", nn.Linear(self._static_q, embed_dim_cfg, bias=True)), ("relu1", nn.ReLU())]))
            _, _, v = torch.pca_lowrank(st, q=self._static_q)
            with torch.no_grad():
                self.node_emb = nn.Parameter(self.static_initial_node(torch.matmul(st, v)))
        else:
            self.static = None
            self.node_emb = nn.Parameter(torch.randn(n, embed_dim_cfg))
        self.node_vec1 = nn.Parameter(torch.empty(n, rank))
        self.node_vec2 = nn.Parameter(torch.empty(rank, n))
        self.spec: PathSpec = spec_from_config(config, data_feature, n, rank, 0 if not use_static else len(mats),
                                               diagonal_mask(self._static_host), hidden=hidden_pad.WIDTH)
        self.output_dim = self.spec.out_dim
        self.feature_final = self.spec.feat_in
        self.len_ts = self.spec.n_ts
        self.weight_ts = nn.ParameterList(
            [nn.Parameter(torch.empty(1, 24, n, self.output_dim)) for _ in range(self.len_ts)])
        self.weight_tsg = nn.Parameter(torch.empty(self.len_ts))
        if static is not None:   # initial state of the encoder from the static features (:335-338)
            self.static_initial_gru = nn.Sequential(OrderedDict(
                [("embd", nn.Linear(self._static_q, self.hidden_dim, bias=True)), ("relu1", nn.ReLU())]))
        self.encoder = _EncoderParams(self.num_layers, self.input_window, self.feature_final, self.hidden_dim,
                                      self.spec.k_total, self.embed_dim_node, self.gcn_off)
        self.end_conv = nn.Conv2d(self.input_window, self.output_window * self.output_dim,
                                  kernel_size=(1, self.hidden_dim), bias=True)   # (:340-341)
        if self.fnn_off:   # the reference builds the full head first, then replaces it (:342-344): two sets of draws
            self.end_conv = nn.Conv2d(1, self.output_window * self.output_dim, kernel_size=(1, self.hidden_dim),
                                      bias=True)
        self._logger = getLogger()
        self._scaler = data_feature.get("scaler")
        self._init_parameters()
        if self.node_specific_off:  # (:350-354)
            self.node_emb = nn.Parameter(torch.ones(n, 1), requires_grad=False)
        self._paths: Dict[int, HotPath] = {}
        self._valid_label_tables = {}
        self._prepared_key = None
        self.cache_prepared = True

    def _init_parameters(self):
        """xavier_uniform on every >=2-D parameter, U(0,1) on every 1-D one (:356-361)."""
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)
            else:
                nn.init.uniform_(p)

    # ---- hot path plumbing ----------------------------------------------------------------------
    def _state(self) -> Dict[str, torch.Tensor]:
        state = {k: v.detach() for k, v in self.named_parameters()}
        return hidden_pad.pad_state(state, self.hidden_dim, self.feature_final) if self._padded else state

    def _initial_state(self, batch: int) -> Optional[torch.Tensor]:
        """(L, B, N, H) initial encoder state from the static features, or None (zeros): a PCA of the static table and
        one nn.Linear + ReLU, expanded over layers and samples (:405-409).  Host-side torch - tiny, and the PCA is
        torch.pca_lowrank exactly as in the reference (randomised: it draws from torch's generator on every forward)."""
        if self.static is None:
            return None
        _, _, v = torch.pca_lowrank(self.static, q=self._static_q)
        emb = self.static_initial_gru(torch.matmul(self.static, v))
        return emb.expand(self.num_layers, batch, -1, -1)

    def _deterministic(self) -> bool:
        """config['hip_deterministic'], None following torch.use_deterministic_algorithms"""
        return _torch_deterministic() if self.hip_deterministic is None else bool(self.hip_deterministic)

    def _dropout_offset(self, draws: int) -> int:
        """the offset of the next device-side dropout draw; advances the model's counter by ``draws``"""
        counter = self._dropout_counter
        self._dropout_counter += int(draws)
        rank = 0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            rank = torch.distributed.get_rank()
        return ((rank << 40) | (counter & ((1 << 40) - 1))) & (2 ** 64 - 1)

    def _params_key(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _path_for(self, x: torch.Tensor) -> HotPath:
        if not x.is_cuda:
            raise RuntimeError("MultiATGCN.forward runs on the HIP hot path only: batch['X'] is on %s. "
                               "Move the model and the batch to the GPU (config['device'])." % x.device)
        return self._path_for_batch(x.shape[0], x.device)

    def _path_for_batch(self, batch: int, device) -> HotPath:
        hp = self._paths.get(batch)
        if hp is None or hp.device != device:
            hp = HotPath(self.spec, batch, device)
            self._paths[batch] = hp
            self._prepared_key = None
        if self._static_host is not None and (self._static_dev is None or self._static_dev.device != device):
            self._static_dev = self._static_host.to(device).contiguous()
        # "fp32" leaves the library settings alone (process-wide matgcn_set_*_precision calls still apply, as before this
        # key existed); the bf16 modes are set around each of this model's library calls and restored afterwards
        mode = _precision_mode(self.hip_precision)
        hp.precision = mode if mode else None
        hp.train_bf16x3 = True if self.hip_precision in HIP_TRAIN_BF16X3 else None
        hp.deterministic = self._deterministic()
        key = (id(hp),) + self._params_key()
        if key != self._prepared_key or not self.cache_prepared:
            hp.bind(self._state(), self._static_dev)
            hp.prepare()
            self._prepared_key = key
        return hp

    # ---- the plugin surface the executor calls ---------------------------------------------------
    def _run(self, source, batch: int, device):
        """One forward on the HIP path.  source: the windows tensor X, or a (series, label_start, rel_steps) triple
        (device-resident raw series).  Inference under no_grad / eval; with gradients
        enabled the training form (activations kept, HIP backward behind torch autograd)."""
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        h0 = self._initial_state(batch)
        h0 = None if h0 is None else (hidden_pad.pad_last(h0) if self._padded else h0.contiguous())
        hp = self._path_for_batch(batch, device)
        if not needs_grad:
            if self.training:
                raise NotImplementedError("training-mode forward (dropout, :416) without autograd is not built: "
                                          "call model.eval() for inference")
            if isinstance(source, torch.Tensor):
                return hp.forward(source, h0)
            return hp.forward_series(source[0], source[1], source[2], h0)
        # training step: HIP forward that keeps its activations + HIP backward behind torch autograd
        mask = None
        if self.training and self.hip_dropout == "device":   # the same dropout, drawn by the kernels that apply it
            mask = (torch.initial_seed(), self._dropout_offset(1), DROPOUT_P)
        elif self.training:   # F.dropout(output, p=0.1) in front of end_conv (:416), drawn from torch's generator
            mask = nn.functional.dropout(torch.ones(batch, 1 if self.fnn_off else self.input_window,
                                                    self.num_nodes, self.hidden_dim, device=device),
                                         p=0.1, training=True)   # fnn_off keeps the last step only (:412)
            if self._padded:
                mask = hidden_pad.pad_last(mask)
        # static_initial_* are host-side torch layers: their gradients flow through h0, not through the HIP backward
        named = [(k, p) for k, p in self.named_parameters() if not k.startswith("static_initial")]
        if self._padded:   # differentiable zero-padding: autograd slices the gradients back into the real parameters
            padded = hidden_pad.pad_state(dict(named), self.hidden_dim, self.feature_final)
            named = [(k, padded[k]) for k, _ in named]
        return _TrainStep.apply(hp, source, mask, h0, tuple(k for k, _ in named), *[p for _, p in named])

    def _crps(self, source, batch: int, device, y, label_start, samples: int):
        """The mean CRPS of an ensemble of ``samples`` dropout samples against the labels (``y`` windows, or with
        label_start the resident series) - the composition of HotPath.forward_train_mc, ops.crps_loss and
        HotPath.backward_mc.  With gradients enabled the samples carry the graph (one encoder pass in both directions);
        without, they come from the inference forward (matgcn_forward_mc).  Consumes ``samples`` dropout offsets."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("the CRPS objective needs an affine scaler (StandardScaler / NoneScaler)")
        needs_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        h0 = self._initial_state(batch)
        h0 = None if h0 is None else (hidden_pad.pad_last(h0) if self._padded else h0.contiguous())
        hp = self._path_for_batch(batch, device)
        seed, offset = torch.initial_seed(), self._dropout_offset(samples)
        if not needs_grad:
            with torch.no_grad():
                kept = hp.forward_mc(source, h0, seed=seed, offset=offset, p=DROPOUT_P, samples=samples,
                                     keep_samples=True)[2]
            return crps_loss_device(kept, y, self.start_dim, affine[0], affine[1], CRPS_NULL_VAL,
                                    label_start=label_start)[0]
        named = [(k, p) for k, p in self.named_parameters() if not k.startswith("static_initial")]
        if self._padded:   # differentiable zero-padding, as in _run
            padded = hidden_pad.pad_state(dict(named), self.hidden_dim, self.feature_final)
            named = [(k, padded[k]) for k, _ in named]
        kept = _TrainStepMc.apply(hp, source, (seed, offset, DROPOUT_P), samples, h0, tuple(k for k, _ in named),
                                  *[p for _, p in named])
        return crps_loss(kept, y, self.start_dim, affine[0], affine[1], CRPS_NULL_VAL, label_start=label_start)

    def _crps_batch(self, batch, samples: int):
        """``_crps`` of a window batch (``X``, ``y``) or a resident-series batch"""
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            return self._crps(src, int(src[1].shape[0]), src[0].device, src[0], src[1], samples)
        x = batch["X"]
        assert x.shape[2] == self.num_nodes
        if not x.is_cuda:
            raise RuntimeError("MultiATGCN runs on the HIP hot path only: batch['X'] is on %s." % x.device)
        x = (x if x.dtype == torch.float32 else x.float()).contiguous()
        return self._crps(x, int(x.shape[0]), x.device, batch["y"], None, samples)

    def forward(self, batch):
        if _is_series_batch(batch):    # MTHDatasetResident: windows and labels are gathered on the device (f-2)
            src = self._batch_source(batch)
            return self._run(src, int(src[1].shape[0]), src[0].device)
        x = batch["X"]
        assert x.shape[2] == self.num_nodes  # (:195)
        if not x.is_cuda:
            raise RuntimeError("MultiATGCN.forward runs on the HIP hot path only: batch['X'] is on %s. "
                               "Move the model and the batch to the GPU (config['device'])." % x.device)
        if x.dtype != torch.float32:
            x = x.float()
        return self._run(x.contiguous(), int(x.shape[0]), x.device)

    def predict(self, batch):
        return self.forward(batch)

    def predict_mc(self, batch, samples: int = 32, seed: Optional[int] = None, keep_samples: bool = False):
        """Monte-Carlo-dropout forecast: ``samples`` stochastic forward passes with the training-mode dropout in front of
        end_conv (:416, p = 0.1) switched on, as (mean, std[, samples]) - std the population standard deviation over the
        samples, all (B, out, N, od); the samples (samples, B, out, N, od) with ``keep_samples``.  Dropout sits only in
        front of the head, so the encoder runs ONCE (in eval form) and the head ``samples`` times, in one kernel launch
        (matgcn_forward_mc).  Works in eval and in train mode (the mode is left as it was; no autograd graph is built)
        and with window and resident-series batches.  seed = None: the model's seed (torch.initial_seed()) and the next
        ``samples`` offsets of its dropout counter; an explicit seed draws at offsets 0 .. samples - 1 and leaves the
        counter alone, so the same call gives the same result."""
        if _is_series_batch(batch):
            source = self._batch_source(batch)
            nb, device = int(source[1].shape[0]), source[0].device
        else:
            x = batch["X"]
            assert x.shape[2] == self.num_nodes
            if not x.is_cuda:
                raise RuntimeError("MultiATGCN.predict_mc runs on the HIP hot path only: batch['X'] is on %s." % x.device)
            source = (x if x.dtype == torch.float32 else x.float()).contiguous()
            nb, device = int(x.shape[0]), x.device
        with torch.no_grad():
            h0 = self._initial_state(nb)
            h0 = None if h0 is None else (hidden_pad.pad_last(h0) if self._padded else h0.contiguous())
            hp = self._path_for_batch(nb, device)
            if seed is None:
                seed, offset = torch.initial_seed(), self._dropout_offset(samples)
            else:
                offset = 0
            return hp.forward_mc(source, h0, seed=seed, offset=offset, p=DROPOUT_P, samples=samples,
                                 keep_samples=keep_samples)

    def predict_interval(self, batch, samples: int = 32, probs=(0.05, 0.5, 0.95), seed: Optional[int] = None,
                         group_mean=None, group_std=None, clamp_min: Optional[float] = None, calibrator=None,
                         regions=None):
        """Monte-Carlo-dropout forecast with its empirical band: (mean, std, quantiles) in the units of ``predict`` -
        mean and std what ``predict_mc`` gives for the same seed, quantiles (len(probs), B, out, N, od) the levels
        ``probs`` (up to 8, ascending, in [0, 1]) of the ``samples`` forecasts per output element, numpy's "linear" rule
        (matgcn_mc_quantiles).  Window and resident-series batches; seed as in ``predict_mc``.
        With ``group_mean`` / ``group_std`` (one value per node, a pair) or ``clamp_min`` the band alone moves to the
        re-transformed scale: every sample goes through the scaler's inverse, then x * group_std + group_mean, and is
        set to ``clamp_min`` where below it, before the quantiles are taken (matgcn_mc_quantiles_scaled; needs an affine
        scaler) - the band in visits.
        ``calibrator`` (a fitted evaluator.ConformalCalibrator; None: the empirical band as it is): the outer two
        levels are widened by its margin (``calibrator.apply``).  Its levels and its scale must be those of this call
        - the scaler's affine (the identity for the band in the units of ``predict``), the group pair and the clamp -,
        anything else is a ValueError.
        ``regions`` (a regions.RegionMap): the forecast of the region TOTALS, (mean, std, quantiles) with G regions in
        place of the N nodes.  Every sample is summed per region first - members go through the scaler's inverse (always:
        a total is in visits; needs an affine scaler), then ``group_mean`` / ``group_std`` and ``clamp_min`` as above, and
        are added in the map's order (matgcn_group_sums: one read of the samples, the same bits every run) -, quantiles
        (len(probs), B, out, G, od) are matgcn_mc_quantiles of the summed samples (quantiles do not add), and mean and std
        (population) are taken over the summed samples with torch: that tensor is S*B*out*G*od floats, a few MB.  A
        ``calibrator`` must have been fitted on the same map (ConformalCalibrator(regions=...))."""
        if regions is not None:
            affine = self._affine_scaler()
            if affine is None:
                raise NotImplementedError("region totals need an affine scaler (StandardScaler / NoneScaler)")
            if calibrator is not None:
                if calibrator.margin is None:
                    raise ValueError("the calibrator is not fitted: call calibrate_mc over a held-out split, then fit()")
                calibrator.check_call(probs, affine, group_mean, group_std, clamp_min, regions)
            kept = self.predict_mc(batch, samples=samples, seed=seed, keep_samples=True)[2]
            totals = group_sums(kept, regions, affine[0], affine[1], group_mean, group_std,
                                float("nan") if clamp_min is None else clamp_min)
            band = mc_quantiles(totals, probs)
            return totals.mean(0), totals.std(0, unbiased=False), band if calibrator is None else calibrator.apply(band)
        plain = group_mean is None and group_std is None and clamp_min is None
        affine = None if plain else self._affine_scaler()
        if not plain and affine is None:
            raise NotImplementedError("a re-transformed band needs an affine scaler (StandardScaler / NoneScaler)")
        if calibrator is not None:
            if calibrator.margin is None:
                raise ValueError("the calibrator is not fitted: call calibrate_mc over a held-out split, then fit()")
            calibrator.check_call(probs, affine, group_mean, group_std, clamp_min)
        mean, std, kept = self.predict_mc(batch, samples=samples, seed=seed, keep_samples=True)
        if plain:
            band = mc_quantiles(kept, probs)
        else:
            band = mc_quantiles_scaled(kept, probs, affine[0], affine[1], group_mean, group_std,
                                       float("nan") if clamp_min is None else clamp_min)
        return mean, std, band if calibrator is None else calibrator.apply(band)

    def predict_regions(self, batch, regions, group_mean=None, group_std=None, clamp_min: Optional[float] = None):
        """The point forecast's region totals (B, out, G, od), in visits: ``predict``, then every member through the
        scaler's inverse, ``group_mean`` / ``group_std`` (one value per node, a pair) and ``clamp_min``, added in the
        order ``regions`` (a regions.RegionMap) lists them (matgcn_group_sums).  Needs an affine scaler."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("region totals need an affine scaler (StandardScaler / NoneScaler)")
        with torch.no_grad():
            pred = self.predict(batch)
        return group_sums(pred.detach(), regions, affine[0], affine[1], group_mean, group_std,
                          float("nan") if clamp_min is None else clamp_min)

    def score_mc(self, batch, samples: int = 32, probs=(0.05, 0.5, 0.95), seed: Optional[int] = None, sums=None):
        """The (out, 5 + len(probs)) float64 per-horizon sums [count, CRPS, covered, width, Winkler, pinball per level] of
        a Monte-Carlo-dropout ensemble against the batch's labels, on de-scaled values with the mask of calculate_loss
        (null value 0), without leaving the GPU (matgcn_mc_scores).  ``batch`` is a window batch (``X``, ``y``) or a
        resident-series batch; ``sums`` from an earlier batch is added to.  evaluator.ProbabilisticEvaluator turns the
        sums into CRPS / PICP / MPIW / Winkler / pinball tables."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("score_mc needs an affine scaler (StandardScaler / NoneScaler)")
        kept = self.predict_mc(batch, samples=samples, seed=seed, keep_samples=True)[2]
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            return mc_scores(kept, src[0], probs, self.start_dim, affine[0], affine[1], null_val=0.0,
                             label_start=src[1], sums=sums)
        return mc_scores(kept, batch["y"], probs, self.start_dim, affine[0], affine[1], null_val=0.0, sums=sums)

    def score_mc_nodes(self, batch, evaluator, samples: int = 32, seed: Optional[int] = None):
        """``score_mc`` per node: one Monte-Carlo-dropout ensemble of the batch reduced into ``evaluator``
        (evaluator.NodeEvaluator built with ``probs``) - its scores per (horizon, node), on the evaluator's scale
        (matgcn_mc_scores_nodes).  Window and resident-series batches.  Returns the samples (S, B, out, N, od), scaled."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("score_mc_nodes needs an affine scaler (StandardScaler / NoneScaler)")
        kept = self.predict_mc(batch, samples=samples, seed=seed, keep_samples=True)[2]
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            evaluator.collect_samples(kept, src[0], self.start_dim, affine[0], affine[1], label_start=src[1])
        else:
            evaluator.collect_samples(kept, batch["y"], self.start_dim, affine[0], affine[1])
        return kept

    def calibrate_mc(self, batch, calibrator, samples: int = 32, seed: Optional[int] = None, test: bool = False):
        """One Monte-Carlo-dropout ensemble of a held-out batch into ``calibrator`` (evaluator.ConformalCalibrator): its
        conformity scores join the calibration store (matgcn_mc_conformity), or - ``test`` - are counted against the
        fitted margin (matgcn_conformal_coverage).  Window and resident-series batches.  Returns the samples
        (S, B, out, N, od), scaled."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("calibrate_mc needs an affine scaler (StandardScaler / NoneScaler)")
        kept = self.predict_mc(batch, samples=samples, seed=seed, keep_samples=True)[2]
        collect = calibrator.collect_test_samples if test else calibrator.collect_samples
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            collect(kept, src[0], self.start_dim, affine[0], affine[1], label_start=src[1])
        else:
            collect(kept, batch["y"], self.start_dim, affine[0], affine[1])
        return kept

    # ---- the same surface fed from the device-resident raw series (no windows, no labels materialised) ----------
    def _batch_source(self, batch):
        """the (series, label_start, rel_steps) triple of a resident-series batch; its label starts were validated on
        the host when the loader's table was built (ResidentBatch.range_checked), a plain dict is checked here"""
        rel = batch.get("rel_steps") if hasattr(batch, "get") else None
        return self._series_source(batch["series"], batch["label_start"], rel,
                                   trusted=bool(getattr(batch, "range_checked", False)))

    def _series_source(self, series: torch.Tensor, label_start, rel_steps, trusted: bool = False):
        """(series, int32 device label starts, rel_steps), with the range contract of the series entry points checked
        on the host: every window row and every target row of every sample inside the series (windows.
        check_label_starts).  A host table (numpy / CPU tensor) is checked before it is uploaded; a device tensor costs
        one min / max read-back the first time it is seen (tables validated once - e.g. by MTHDatasetResident or
        windows.epoch_batches - are registered with ``mark_label_starts_valid`` and cost nothing per batch)."""
        from . import windows
        if rel_steps is None:
            rel_steps = windows.window_offsets(self.input_window)
        if not series.is_cuda:
            raise RuntimeError("the series must live on the GPU (HIP path only)")
        steps = int(series.shape[0])
        if not isinstance(label_start, torch.Tensor) or not label_start.is_cuda:
            host = np.asarray(label_start.cpu() if isinstance(label_start, torch.Tensor) else label_start)
            windows.check_label_starts(host, rel_steps, self.output_window, steps)
            return (series, torch.as_tensor(host.astype(np.int32)).to(series.device), rel_steps)
        ls = label_start.to(torch.int32)
        if trusted:
            return (series, ls, rel_steps)
        # Only tables that were registered as OBJECTS are trusted (a key built from data_ptr() survives
        # the tensor - the caching allocator hands the same address to the next batch, whose _version is 0 again - so a
        # later out-of-range batch could hit the stale key and skip the check).  A row of a registered table is a view of
        # it (``_base``); anything else - a fresh tensor per batch, the int32 copy of an int64 tensor - is checked on every
        # call (one min / max read-back).
        base = ls._base if ls._base is not None else ls
        rel_key = tuple(int(v) for v in (min(rel_steps), max(rel_steps)))
        if self._label_table_is_valid(base, steps, rel_key):
            return (series, ls, rel_steps)
        lo, hi = (int(v) for v in torch.aminmax(ls))
        windows.check_label_starts(np.array([lo, hi]), rel_steps, self.output_window, steps)
        if base is not ls:      # a view of a longer-lived table: validate the table once, then trust its other rows
            lo, hi = (int(v) for v in torch.aminmax(base))
            try:
                windows.check_label_starts(np.array([lo, hi]), rel_steps, self.output_window, steps)
                self.mark_label_starts_valid(base, steps, rel_steps)
            except ValueError:
                pass
        return (series, ls, rel_steps)

    def _label_table_is_valid(self, table: torch.Tensor, steps: int, rel_key) -> bool:
        ent = self._valid_label_tables.get(id(table))
        if ent is None:
            return False
        ref, version, st, rk = ent
        if ref() is not table:      # the id belongs to a dead tensor: forget it
            del self._valid_label_tables[id(table)]
            return False
        return version == table._version and st == steps and rk == rel_key

    def mark_label_starts_valid(self, table: torch.Tensor, series_steps: int, rel_steps) -> None:
        """Register a device table of label starts that has been validated on the host (windows.check_label_starts):
        batches that are views of it skip the per-call range check.  The table is remembered as an object (weak
        reference + ``_version``): writing into it, or its death, ends the trust."""
        import weakref
        if len(self._valid_label_tables) > 64:
            self._valid_label_tables = {k: v for k, v in self._valid_label_tables.items() if v[0]() is not None}
        self._valid_label_tables[id(table)] = (weakref.ref(table), table._version, int(series_steps),
                                               tuple(int(v) for v in (min(rel_steps), max(rel_steps))))

    def forward_series(self, series: torch.Tensor, label_start: torch.Tensor, rel_steps=None):
        """forward() without materialised windows: ``series`` (T, N, F) float32 resident on the GPU, ``label_start``
        (B) first-target indices; the window rows are gathered on the device (windows.window_offsets gives
        ``rel_steps``; the default is the reference's 2 x 24 h closeness + 1-week + 4-week heads).  Replaces
        MTHDataset._generate_input_data + the per-batch host copy (mth_dataset.py:110-160, data/utils.py:68-72,
        batch.py:43-57); trains like forward() when gradients are enabled."""
        src = self._series_source(series, label_start, rel_steps)
        return self._run(src, int(src[1].shape[0]), series.device)

    def predict_series(self, series: torch.Tensor, label_start: torch.Tensor, rel_steps=None):
        return self.forward_series(series, label_start, rel_steps)

    def calculate_loss_series(self, series: torch.Tensor, label_start: torch.Tensor, rel_steps=None, _checked=False):
        """calculate_loss (:422-427) of the batch given by ``label_start``: the prediction from the series-fed forward,
        the targets series[label_start[b] + o] gathered by the loss kernel on the device.  With gradients enabled this is
        the executor's training step (traffic_state_executor.py:411-422) without any host-side window or label."""
        src = self._series_source(series, label_start, rel_steps, trusted=_checked)
        if self.hip_train_loss == CRPS_LOSS:
            return self._crps(src, int(src[1].shape[0]), series.device, series, src[1], self.hip_train_samples)
        pred = self._run(src, int(src[1].shape[0]), series.device)
        ls = src[1]
        if self.hip_region_loss_weight > 0.0:
            return self._objective(pred, series, self._region_objective(), self.hip_train_loss_delta, ls,
                                   self.hip_train_regions, self.hip_region_loss_weight, self.hip_tract_loss_weight)
        if self.hip_train_loss != "none":
            return self._objective(pred, series, self.hip_train_loss, self.hip_train_loss_delta, ls)
        affine = self._affine_scaler()
        if affine is not None and series.dtype == torch.float32:
            if pred.requires_grad:
                return masked_mae_loss(pred, series, self.start_dim, affine[0], affine[1], null_val=0.0, label_start=ls)
            return masked_mae_device(pred, series, self.start_dim, affine[0], affine[1], null_val=0.0, label_start=ls)[0]
        rows = ls.long()[:, None] + torch.arange(self.output_window, device=series.device)[None, :]
        y_true = self._scaler.inverse_transform(series[rows][..., self.start_dim:self.end_dim].clone())
        return masked_mae(self._scaler.inverse_transform(pred), y_true, 0)

    def horizon_mae_series(self, series: torch.Tensor, label_start: torch.Tensor, rel_steps=None, _checked=False):
        """(out,) MAE@1..MAE@out of the batch given by ``label_start`` (evaluator "single" mode), all on the device."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("horizon_mae_series needs an affine scaler (StandardScaler / NoneScaler)")
        src = self._series_source(series, label_start, rel_steps, trusted=_checked)
        pred = self._run(src, int(src[1].shape[0]), series.device)
        return masked_mae_device(pred, series, self.start_dim, affine[0], affine[1], label_start=src[1])[1:]

    def collect_metrics(self, evaluator, batch):
        """One test batch of TrafficStateExecutor.evaluate (traffic_state_executor.py:264-273, 289) without leaving the
        GPU: predict, de-scale prediction and label with the scaler's affine inside the metric kernel, and reduce into
        ``evaluator`` (multistgraph_amd.evaluator.DeviceEvaluator).  ``batch`` is a window batch (``X``, ``y``) or a
        resident-series batch (``series``, ``label_start``: MTHDatasetResident).  Returns the prediction (scaled)."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("collect_metrics needs an affine scaler (StandardScaler / NoneScaler)")
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            pred = self._run(src, int(src[1].shape[0]), src[0].device)
            evaluator.collect_scaled(pred, src[0], self.start_dim, affine[0], affine[1], label_start=src[1])
        else:
            pred = self.predict(batch)
            evaluator.collect_scaled(pred, batch["y"], self.start_dim, affine[0], affine[1])
        return pred

    def collect_node_metrics(self, evaluator, batch):
        """``collect_metrics`` per node: the same batch reduced into an evaluator.NodeEvaluator - the ten metrics per
        (horizon, node) on its scale (matgcn_metric_sums_nodes).  Returns the prediction (scaled)."""
        return self.collect_metrics(evaluator, batch)

    def collect_region_metrics(self, evaluator, batch):
        """``collect_metrics`` per region: the same batch reduced into an evaluator.RegionEvaluator - the ten metrics of the
        region totals per (horizon, region).  Window and resident-series batches.  Returns the prediction (scaled)."""
        return self.collect_metrics(evaluator, batch)

    def score_mc_regions(self, batch, evaluator, samples: int = 32, seed: Optional[int] = None):
        """``score_mc_nodes`` per region: one Monte-Carlo-dropout ensemble of the batch, summed per region sample by sample
        and reduced into ``evaluator`` (evaluator.RegionEvaluator built with ``probs``).  Window and resident-series
        batches.  Returns the samples (S, B, out, N, od), scaled."""
        return self.score_mc_nodes(batch, evaluator, samples=samples, seed=seed)

    def gradient_exchange(self):
        """(bucket, leftovers) for the gradient exchange of data-parallel training after ``loss.backward()``:
        ``bucket`` = the flat fp32 buffer the gradients of the HIP-path parameters are views of (one all-reduce, no
        copy), or None when some of them live elsewhere (rnn_units < 64: autograd slices the padded gradients back
        into tensors of their own; gradients accumulated over several backward calls); ``leftovers`` = every other
        ``.grad`` that is not None - with a bucket these are the host-side ``static_initial_*`` layers of the
        static-feature path, whose gradients arrive through d_h0 and torch autograd, without one ALL gradients.
        sharding.allreduce_model_grads_(model) is the entry point that reduces both."""
        with_grad = [(k, p) for k, p in self.named_parameters() if p.requires_grad and p.grad is not None]
        for hp in self._paths.values():
            b = hp.grad_bucket
            if b is None:
                continue
            lo, hi = b.data_ptr(), b.data_ptr() + b.numel() * 4
            mine = [p for k, p in self.named_parameters() if p.requires_grad and not k.startswith("static_initial")]
            if mine and all(p.grad is not None and lo <= p.grad.data_ptr() < hi for p in mine):
                return b, [p.grad for _, p in with_grad if not lo <= p.grad.data_ptr() < hi]
        return None, [p.grad for _, p in with_grad]

    def gradient_bucket(self) -> Optional[torch.Tensor]:
        """The flat fp32 buffer that holds the gradient of EVERY parameter after ``loss.backward()`` (their ``.grad``
        are views of it) - or None as soon as any gradient lives outside it (static-feature layers, rnn_units < 64,
        accumulated gradients): reducing the buffer alone would then leave replicas diverging.  Data-parallel loops
        call sharding.allreduce_model_grads_(model), which handles both cases."""
        bucket, rest = self.gradient_exchange()
        return bucket if not rest else None

    def _affine_scaler(self):
        """(mean, std) when the scaler de-scales as x*std + mean with scalar parameters - LibCity's StandardScaler,
        NoneScaler, NormalScaler, MinMax01Scaler, MinMax11Scaler (libcity/utils/normalization.py:20-113) all do -,
        else None (LogScaler).  Found by probing inverse_transform at three points, so any scaler object works."""
        sc = self._scaler
        if sc is None:
            return None
        try:
            probe = sc.inverse_transform(torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64))
            f0, f1, f2 = (float(v) for v in probe)
        except Exception:
            return None
        mean, std = f0, f1 - f0
        if not all(math.isfinite(v) for v in (f0, f1, f2)) or abs(f2 - (mean + 2.0 * std)) > 1e-9 * max(1.0, abs(f2)):
            return None
        return mean, std

    def calculate_loss(self, batch):
        """de-scale prediction and label, masked MAE with null value 0 (:422-427).  With an affine scaler the
        de-scale + mask + reduction run fused on the device; any other scaler takes the reference's torch
        arithmetic on the HIP prediction."""
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            return self.calculate_loss_series(src[0], src[1], src[2], _checked=True)
        if self.hip_train_loss == CRPS_LOSS:
            return self._crps_batch(batch, self.hip_train_samples)
        y_true = batch["y"]
        y_predicted = self.predict(batch)
        if self.hip_region_loss_weight > 0.0:
            return self._objective(y_predicted, y_true, self._region_objective(), self.hip_train_loss_delta, None,
                                   self.hip_train_regions, self.hip_region_loss_weight, self.hip_tract_loss_weight)
        if self.hip_train_loss != "none":
            return self._objective(y_predicted, y_true, self.hip_train_loss, self.hip_train_loss_delta)
        affine = self._affine_scaler()
        if affine is not None and y_true.is_cuda and y_true.dtype == torch.float32 and y_predicted.requires_grad:
            return masked_mae_loss(y_predicted, y_true, self.start_dim, affine[0], affine[1], null_val=0.0)
        if affine is not None and y_true.is_cuda and y_true.dtype == torch.float32:
            return masked_mae_device(y_predicted, y_true, self.start_dim, affine[0], affine[1], null_val=0.0)[0]
        y_true = self._scaler.inverse_transform(y_true[..., self.start_dim:self.end_dim])
        y_predicted = self._scaler.inverse_transform(y_predicted)
        return masked_mae(y_predicted, y_true, 0)

    def _region_objective(self) -> str:
        """the objective of both levels when a region term is configured: hip_train_loss, "none" = masked_mae"""
        return "masked_mae" if self.hip_train_loss == "none" else self.hip_train_loss

    def _objective(self, pred, y, name, delta, label_start=None, regions=None, region_weight=0.0, tract_weight=1.0):
        """the executor's objective ``name`` of a prediction on the device: ``y`` the label windows, or with label_start
        the resident series; with autograd when the prediction carries a graph.  With ``regions``:
        tract_weight * L(tracts) + region_weight * L(region totals) (ops.tract_region_loss)."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("train_loss needs an affine scaler (StandardScaler / NoneScaler)")
        if regions is not None:
            return tract_region_loss(pred, y, regions, self.start_dim, affine[0], affine[1], name, delta, label_start,
                                     tract_weight, region_weight)
        fn = train_loss_autograd if pred.requires_grad else train_loss_device
        out = fn(pred, y, self.start_dim, affine[0], affine[1], name, delta, label_start)
        return out if pred.requires_grad else out[0]

    def train_loss(self, batch, name, delta=None, regions=None, region_weight=1.0, tract_weight=1.0, samples=None):
        """One of the executor's eleven differentiable training objectives (TrafficStateExecutor._build_train_loss,
        traffic_state_executor.py:200-250; ops.TRAIN_LOSSES) of a window batch (``X``, ``y``) or a resident-series batch
        (``series``, ``label_start``): predict, de-scale, mask and reduce in a fixed order on the device (matgcn_loss); with
        gradients enabled the result backpropagates through matgcn_loss_grad into the HIP backward.  ``delta``: huber's
        knee / quantile's level (None: 1.0 / 0.25, the reference's defaults).  The label channels start at ``start_dim``,
        as in calculate_loss.  ``regions`` (a regions.RegionMap, its state_dict() or one label per node; None: what
        this method always did): tract_weight * L(tracts) + region_weight * L(region totals) with the same objective on
        both levels (matgcn_region_loss / matgcn_region_loss_grad); a weight of 0 skips its half.
        ``name`` = "crps": the mean CRPS of an ensemble of ``samples`` dropout samples (None: hip_train_samples), what
        calculate_loss returns under hip_train_loss = "crps"; drawn on the device whatever hip_dropout says."""
        if str(name).lower() == CRPS_LOSS:
            if regions is not None:
                raise NotImplementedError("train_loss 'crps' with regions: the CRPS of region totals is not built")
            return self._crps_batch(batch, self.hip_train_samples if samples is None else _train_samples(samples, "samples"))
        train_loss_desc(name, 0.0, 1.0, delta)      # refuse a bad name or delta before any kernel runs
        if regions is not None:
            regions = _train_regions(regions, self.num_nodes)
            region_weight = _loss_weight(region_weight, "region_weight")
            tract_weight = _loss_weight(tract_weight, "tract_weight")
            if region_weight == 0.0 and tract_weight == 0.0:
                raise ValueError("train_loss: tract_weight and region_weight are both 0")
        if self._affine_scaler() is None:
            raise NotImplementedError("train_loss needs an affine scaler (StandardScaler / NoneScaler)")
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            pred = self._run(src, int(src[1].shape[0]), src[0].device)
            return self._objective(pred, src[0], name, delta, src[1], regions, region_weight, tract_weight)
        return self._objective(self.predict(batch), batch["y"], name, delta, None, regions, region_weight, tract_weight)

    def horizon_mae(self, batch):
        """(out,) device tensor MAE@1..MAE@out in the evaluator's "single" mode on de-scaled values
        (traffic_state_executor.py:268-273, traffic_state_evaluator.py:87-104), without leaving the GPU."""
        affine = self._affine_scaler()
        if affine is None:
            raise NotImplementedError("horizon_mae needs an affine scaler (StandardScaler / NoneScaler)")
        if _is_series_batch(batch):
            src = self._batch_source(batch)
            return self.horizon_mae_series(src[0], src[1], src[2], _checked=True)
        pred = self.predict(batch)
        return masked_mae_device(pred, batch["y"], self.start_dim, affine[0], affine[1])[1:]
