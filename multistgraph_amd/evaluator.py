"""The evaluator's metric table on the device.

``DeviceEvaluator`` mirrors the surface of the reference's ``TrafficStateEvaluator`` (libcity/evaluator/
traffic_state_evaluator.py:11-174: ``collect`` / ``evaluate`` / ``clear``, the ten metrics of TrafficStateEvaluator.json,
modes "single" and "average") but never copies predictions to the host: ``collect`` reduces a batch to 14 sums per
horizon on the device (matgcn_metric_sums), ``evaluate`` reads one small table back.  ``groupstd_table`` is the
per-horizon table TrafficStateExecutor.evaluate writes after re-transforming with the per-tract mean / std
(libcity/executor/traffic_state_executor.py:293-322).

``ProbabilisticEvaluator`` is its counterpart for a Monte-Carlo-dropout ensemble (model.predict_mc(keep_samples=True)):
CRPS, interval coverage and width, the interval (Winkler) score and pinball losses per horizon, accumulated over the
batches of a test set on the device (matgcn_mc_scores).  The reference has no such evaluator.

``ConformalCalibrator`` makes that ensemble's band mean what its levels say: split conformal calibration from the
conformity scores of a held-out split, kept, ranked and applied on the device (matgcn_mc_conformity,
matgcn_conformal_quantile, matgcn_conformal_coverage).

``RegionEvaluator`` is ``NodeEvaluator`` over the totals of groups of nodes (regions.RegionMap): predictions, samples and
labels are summed per region first (matgcn_group_sums / matgcn_group_label_sums), then scored with the same kernels;
``ConformalCalibrator(regions=...)`` calibrates the band of those totals.

HIP path only: CPU tensors raise.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import _lib
from .ops import (conformal_coverage, conformal_quantile, group_label_sums, group_sums, mc_conformity, mc_scores,
                  mc_scores_nodes, metric_sums, metric_sums_nodes, metric_table, metric_table_rows)

ALLOWED_METRICS = list(_lib.METRICS)


class DeviceEvaluator:
    """config keys as the reference: ``metrics`` (default ['MAE']), ``evaluator_mode`` ('single' | 'average'),
    ``min_s`` (1e-4).  Every ``collect`` call is one batch of the reference's evaluator (``evaluate`` averages the
    batches' metrics, :123-131); with ``streaming=True`` all calls accumulate into ONE batch - the executor collects
    the whole test set in one call (traffic_state_executor.py:289), and this is that call fed batch by batch."""

    def __init__(self, config, streaming: bool = False):
        self.metrics: List[str] = list(config.get("metrics", ["MAE"]))
        self.mode = str(config.get("evaluator_mode", "single")).lower()
        self.min_s = float(config.get("min_s", 1e-4))
        self.streaming = bool(streaming)
        if not isinstance(config.get("metrics", ["MAE"]), list):
            raise TypeError("Evaluator type is not list")
        for m in self.metrics:
            if m not in ALLOWED_METRICS:
                raise ValueError("the metric {} is not allowed in TrafficStateEvaluator".format(str(m)))
        if self.mode not in ("single", "average"):
            raise ValueError("Error parameter evaluator_mode={}, please set `single` or `average`.".format(self.mode))
        self.clear()

    def clear(self):
        self.result: Dict[str, float] = {}
        self._tables: List[torch.Tensor] = []      # one (2, out, 10) table per closed batch
        self._sums: Optional[torch.Tensor] = None  # streaming: the running sums
        self.len_timeslots = 0

    def collect(self, batch):
        """batch['y_true'], batch['y_pred']: (B, timeslots, N, od) CUDA float32, already de-scaled (what the executor
        hands over, traffic_state_executor.py:268-273)."""
        if not isinstance(batch, dict):
            raise TypeError("evaluator.collect input is not a dict of user")
        y_true, y_pred = batch["y_true"], batch["y_pred"]
        if y_true.shape != y_pred.shape:
            raise ValueError("batch['y_true'].shape is not equal to batch['y_pred'].shape")
        self.collect_scaled(y_pred, y_true)

    def collect_scaled(self, pred, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """The same from the model's raw output: ``pred`` (B, out, N, od) in scaled units, ``y`` the batch's labels
        (B, y_steps, N, F) - or, with ``label_start``, the device-resident series (T, N, F) -, de-scaled in the kernel
        by x*std + mean (the scaler's inverse_transform; scalar or one pair per node)."""
        self.len_timeslots = int(pred.shape[1])
        sums = metric_sums(pred, y, y_start, mean, std, min_s=self.min_s, label_start=label_start,
                           sums=self._sums if self.streaming else None)
        if self.streaming:
            self._sums = sums
        else:
            self._tables.append(metric_table(sums))

    def table(self) -> torch.Tensor:
        """(out, 10) float64 CPU tensor of the selected mode, metric order ``ALLOWED_METRICS``"""
        if self.streaming:
            if self._sums is None:
                raise RuntimeError("nothing collected")
            t = metric_table(self._sums)
        else:
            if not self._tables:
                raise RuntimeError("nothing collected")
            t = torch.stack(self._tables, 0).mean(0)   # the mean of the batches' metrics (:123-131)
        return t[0 if self.mode == "single" else 1].cpu()

    def evaluate(self) -> Dict[str, float]:
        t = self.table()
        for i in range(1, self.len_timeslots + 1):
            for m in self.metrics:
                self.result[m + "@" + str(i)] = float(t[i - 1, ALLOWED_METRICS.index(m)])
        return self.result


class ProbabilisticEvaluator:
    """Scores of the sample ensemble against the labels, per horizon, over every batch collected since ``clear``:
    ``CRPS@k`` (the ensemble CRPS mean|x - l| - mean|x - x'| / 2), ``PICP@k`` (the share of labels inside
    [first level, last level] of ``probs``), ``MPIW@k`` (the mean width of that interval), ``WINKLER@k`` (the interval
    score at alpha = 1 - (last - first)) and ``PINBALL_<q>@k`` per level - means over the unmasked labels (null value 0,
    |label| < ``min_s`` counted as 0: the convention of calculate_loss).  config keys: ``min_s`` (1e-4)."""

    def __init__(self, config, probs=(0.05, 0.5, 0.95)):
        self.probs = _check_probs(probs)
        self.min_s = float(config.get("min_s", 1e-4))
        self.columns: List[str] = ["CRPS", "PICP", "MPIW", "WINKLER"] + ["PINBALL_%g" % q for q in self.probs]
        self.clear()

    def clear(self):
        self.result: Dict[str, float] = {}
        self._sums: Optional[torch.Tensor] = None
        self.len_timeslots = 0

    def collect_samples(self, samples, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """One batch: ``samples`` (S, B, out, N, od) in scaled units, ``y`` the batch's labels (B, y_steps, N, F) - or,
        with ``label_start``, the device-resident series (T, N, F) -, both de-scaled in the kernel by x*std + mean
        (scalars; None = identity)."""
        if (mean is None) != (std is None):
            raise ValueError("mean and std come as a pair")
        self.len_timeslots = int(samples.shape[2])
        self._sums = mc_scores(samples, y, self.probs, y_start, 0.0 if mean is None else float(mean),
                               1.0 if std is None else float(std), null_val=0.0, min_s=self.min_s,
                               label_start=label_start, sums=self._sums)

    def table(self) -> torch.Tensor:
        """(out, 4 + levels) float64 CPU tensor, column order ``columns``; a horizon without an unmasked label is NaN"""
        if self._sums is None:
            raise RuntimeError("nothing collected")
        s = self._sums.cpu()
        count = s[:, :1]
        return torch.where(count > 0, s[:, 1:] / count, torch.full_like(s[:, 1:], float("nan")))

    def evaluate(self) -> Dict[str, float]:
        t = self.table()
        for i in range(1, self.len_timeslots + 1):
            for c, name in enumerate(self.columns):
                self.result[name + "@" + str(i)] = float(t[i - 1, c])
        return self.result


def _check_probs(probs):
    probs = tuple(float(q) for q in probs)
    if not 1 <= len(probs) <= _lib.MAX_MC_QUANTILES:
        raise ValueError("probs: 1 .. %d levels, got %d" % (_lib.MAX_MC_QUANTILES, len(probs)))
    if any(not 0.0 <= q <= 1.0 for q in probs) or any(a > b for a, b in zip(probs, probs[1:])):
        raise ValueError("probs must be ascending levels in [0, 1], got %s" % (probs,))
    return probs


class NodeEvaluator:
    """The tract-by-tract view of a test set (result_plot.py:102-134) without a row per prediction element: the sums of
    ``DeviceEvaluator(streaming=True)`` and of ``ProbabilisticEvaluator`` kept per (horizon, node) on the device
    (matgcn_metric_sums_nodes / matgcn_mc_scores_nodes), over every batch collected since ``clear``.  Batches add up in a
    fixed order: any split of the test set into batches gives the same bits.

    ``group_mean`` / ``group_std`` (one value per node, as a pair): the re-transform of traffic_state_executor.py:293-322
    - values go through x * All_std + All_m after the scaler, predictions and samples below 0 become 0, tiny labels are
    not zeroed, nothing is masked but NaN labels, and R2 / EVAR exchange prediction and truth as ``groupstd_table``
    does.  Without them: the conventions of the two per-horizon evaluators (``min_s`` of the config, null value 0 for the
    scores).  ``s_small``: only elements whose (re-transformed) truth exceeds it take part (None: all).  ``probs``: the
    levels of the probabilistic scores (None: ``collect_samples`` is not available)."""

    def __init__(self, config, probs=None, group_mean=None, group_std=None, s_small=None):
        if (group_mean is None) != (group_std is None):
            raise ValueError("group_mean and group_std come as a pair")
        self.probs = None if probs is None else _check_probs(probs)
        self.group = None if group_mean is None else (group_mean, group_std)
        self.truth_min = float("nan") if s_small is None else float(s_small)
        self.clamp_min = float("nan") if self.group is None else 0.0
        self.min_s = float(config.get("min_s", 1e-4)) if self.group is None else -1.0
        self.null_val = 0.0 if self.group is None else float("nan")
        self.swap_r2 = self.group is not None
        self.score_columns: List[str] = [] if self.probs is None else (
            ["CRPS", "PICP", "MPIW", "WINKLER"] + ["PINBALL_%g" % q for q in self.probs])
        self.clear()

    def clear(self):
        self._metric_sums: Optional[torch.Tensor] = None     # (out, N, 14)
        self._score_sums: Optional[torch.Tensor] = None      # (out, N, 5 + levels)

    def _scale(self, mean, std):
        if (mean is None) != (std is None):
            raise ValueError("mean and std come as a pair")
        gm, gs = self.group if self.group is not None else (None, None)
        return dict(mean=mean, std=std, group_mean=gm, group_std=gs, clamp_min=self.clamp_min, truth_min=self.truth_min,
                    min_s=self.min_s)

    def collect_scaled(self, pred, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """One batch of point forecasts: arguments as ``DeviceEvaluator.collect_scaled``."""
        self._metric_sums = metric_sums_nodes(pred, y, y_start, label_start=label_start, sums=self._metric_sums,
                                              **self._scale(mean, std))

    def collect_samples(self, samples, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """One batch of an ensemble: arguments as ``ProbabilisticEvaluator.collect_samples`` (mean / std may be per node)."""
        if self.probs is None:
            raise RuntimeError("this evaluator was built without probs: no probabilistic scores")
        self._score_sums = mc_scores_nodes(samples, y, self.probs, y_start, null_val=self.null_val,
                                           label_start=label_start, sums=self._score_sums, **self._scale(mean, std))

    def _need(self, sums, what):
        if sums is None:
            raise RuntimeError("nothing collected: call %s first" % what)
        return sums

    # ---- the ten metrics (column order ALLOWED_METRICS), float64 CPU tensors
    def node_horizon_table(self) -> torch.Tensor:
        """(out, N, 10)"""
        s = self._need(self._metric_sums, "collect_scaled")
        return metric_table_rows(s, 1, self.swap_r2).reshape(s.shape[0], s.shape[1], -1).cpu()

    def node_table(self) -> torch.Tensor:
        """(N, 10): every node over all horizons"""
        s = self._need(self._metric_sums, "collect_scaled")
        return metric_table_rows(s, int(s.shape[0]), self.swap_r2).cpu()

    def horizon_table(self) -> torch.Tensor:
        """(out, 10): every horizon over all nodes, the nodes' sums added in ascending node order"""
        s = self._need(self._metric_sums, "collect_scaled")
        return metric_table_rows(s.transpose(0, 1).contiguous(), int(s.shape[1]), self.swap_r2).cpu()

    # ---- the probabilistic scores (column order score_columns), float64 CPU tensors, NaN where nothing was counted
    @staticmethod
    def _ratios(s):
        count = s[..., :1]
        return torch.where(count > 0, s[..., 1:] / count, torch.full_like(s[..., 1:], float("nan")))

    def node_horizon_scores(self) -> torch.Tensor:
        """(out, N, 4 + levels)"""
        return self._ratios(self._need(self._score_sums, "collect_samples").cpu())

    def node_scores(self) -> torch.Tensor:
        """(N, 4 + levels)"""
        return self._ratios(self._need(self._score_sums, "collect_samples").cpu().sum(0))

    def horizon_scores(self) -> torch.Tensor:
        """(out, 4 + levels)"""
        return self._ratios(self._need(self._score_sums, "collect_samples").cpu().sum(1))

    def rank(self, metric: str = "MAPE") -> torch.Tensor:
        """Node indices by ``metric`` of ``node_table`` in ascending order (ties by index), nodes without a kept element
        - absent from the reference's groupby - and NaN values last: the ranking of result_plot.py:128."""
        if metric not in ALLOWED_METRICS:
            raise ValueError("the metric {} is not allowed in TrafficStateEvaluator".format(str(metric)))
        values = self.node_table()[:, ALLOWED_METRICS.index(metric)].clone()
        values[self._metric_sums[:, :, 0].cpu().sum(0) == 0] = float("nan")
        nan = torch.isnan(values)
        order = torch.argsort(torch.where(nan, torch.full_like(values, float("inf")), values), stable=True)
        return torch.cat([order[~nan[order]], order[nan[order]]])


def _region_totals(regions, values, y, y_start, mean, std, group, member_clamp, label_start):
    """(totals of ``values`` (..., out, N, od), totals of the labels (B, out, G, od)) on the re-transformed scale: members
    de-scaled by mean / std and the group pair; predictions and samples clamped at ``member_clamp``, labels never"""
    gm, gs = group if group is not None else (None, None)
    totals = group_sums(values, regions, mean, std, gm, gs, member_clamp)
    labels = group_label_sums(y, regions, int(values.shape[-3]), int(values.shape[-1]), y_start, mean, std, gm, gs,
                              label_start=label_start)
    return totals, labels


class RegionEvaluator(NodeEvaluator):
    """``NodeEvaluator`` with one row per region of ``regions`` (regions.RegionMap) in place of one per node: the error
    and the scores of a region TOTAL, which are not the sums of its tracts' (errors of opposite sign cancel in a total,
    and quantiles do not add).  Each batch is summed per region first - members de-scaled by the scaler and the
    ``group_mean`` / ``group_std`` pair, predictions and samples below 0 set to 0 when the pair is given, then added in
    the map's order (matgcn_group_sums, matgcn_group_label_sums) - and the totals go through matgcn_metric_sums_nodes /
    matgcn_mc_scores_nodes with an identity scale.  Region-level conventions: a NaN label is the only mask (it makes its
    regions' totals NaN), ``min_s`` is off, ``s_small`` filters on the region's true total, R2 / EVAR exchange prediction
    and truth as in the re-transform table.  Tables and ``rank`` are those of ``NodeEvaluator`` with G rows; any split
    of a test set into batches gives the same bits."""

    def __init__(self, config, regions, probs=None, group_mean=None, group_std=None, s_small=None):
        super().__init__(config, probs, group_mean, group_std, s_small)
        self.regions = regions
        self.member_clamp = self.clamp_min
        self.clamp_min, self.min_s, self.null_val, self.swap_r2 = float("nan"), -1.0, float("nan"), True

    def _level(self):
        return dict(clamp_min=float("nan"), truth_min=self.truth_min, min_s=-1.0)

    def collect_scaled(self, pred, y, y_start: int = 0, mean=None, std=None, label_start=None):
        if (mean is None) != (std is None):
            raise ValueError("mean and std come as a pair")
        totals, labels = _region_totals(self.regions, pred, y, y_start, mean, std, self.group, self.member_clamp,
                                        label_start)
        self._metric_sums = metric_sums_nodes(totals, labels, 0, sums=self._metric_sums, **self._level())

    def collect_samples(self, samples, y, y_start: int = 0, mean=None, std=None, label_start=None):
        if self.probs is None:
            raise RuntimeError("this evaluator was built without probs: no probabilistic scores")
        if (mean is None) != (std is None):
            raise ValueError("mean and std come as a pair")
        totals, labels = _region_totals(self.regions, samples, y, y_start, mean, std, self.group, self.member_clamp,
                                        label_start)
        self._score_sums = mc_scores_nodes(totals, labels, self.probs, 0, null_val=float("nan"), sums=self._score_sums,
                                           **self._level())


def _f32(v) -> float:
    """the double of the float32 nearest to v: what the kernels see of a level"""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _same_scalar(a, b) -> bool:
    """two optional floats, None and NaN both meaning "off" """
    a = float("nan") if a is None else float(a)
    b = float("nan") if b is None else float(b)
    return a == b or (a != a and b != b)


def _same_vector(a, b) -> bool:
    """two optional per-node (or scalar) float32 vectors"""
    if a is None or b is None:
        return a is None and b is None
    a, b = (torch.as_tensor(v, dtype=torch.float32).detach().reshape(-1).cpu() for v in (a, b))
    return a.shape == b.shape and torch.equal(a, b)


class ConformalCalibrator:
    """Split conformal calibration of the Monte-Carlo-dropout band [first level, last level] of ``probs``: conformity
    scores s = max(Q_first - l, l - Q_last) of a held-out split are collected into a store on the device
    (matgcn_mc_conformity), ``fit`` takes per group the k-th smallest of the n valid ones, k = ceil((n + 1) * coverage)
    with coverage = last level - first level (matgcn_conformal_quantile), and ``apply`` widens a band by that margin:
    on windows exchangeable with the calibration split the widened band covers with probability >= coverage.
    ``grouping``: "horizon" - one margin per horizon - or "element" - one per (horizon, node, channel).  A group with
    fewer than k valid scores gets the margin +inf (an honest "not enough data"; ``infinite_margins`` counts them).

    Scale as ``NodeEvaluator``: with ``group_mean`` / ``group_std`` the re-transform, clamp at 0, NaN null value, no
    ``min_s``; without them the config's ``min_s`` and null value 0.  ``s_small`` leaves out labels at or below it.  The
    scaler's affine is the one of the first ``collect_samples`` call; bands passed to ``apply`` must be on that scale.
    Only ``evaluate`` / ``coverage_table`` / ``state_dict`` read the device.

    ``regions`` (regions.RegionMap): the band of the region totals is calibrated instead - samples and labels are summed
    per region first, as ``RegionEvaluator`` does (NaN the only mask, no ``min_s``, ``s_small`` on the region's true
    total), "element" then means (horizon, region, channel), and ``apply`` takes bands (levels, ..., out, G, od)."""

    def __init__(self, config, probs=(0.05, 0.5, 0.95), grouping="horizon", group_mean=None, group_std=None, s_small=None,
                 capacity: int = 256, regions=None):
        if (group_mean is None) != (group_std is None):
            raise ValueError("group_mean and group_std come as a pair")
        self.probs = _check_probs(probs)
        if len(self.probs) < 2:
            raise ValueError("a band needs at least two levels, got %s" % (self.probs,))
        self.coverage = _f32(self.probs[-1]) - _f32(self.probs[0])
        if not 0.0 < self.coverage <= 1.0:
            raise ValueError("the outer levels %g, %g span no band" % (self.probs[0], self.probs[-1]))
        if grouping not in ("horizon", "element"):
            raise ValueError("grouping must be 'horizon' or 'element', got %r" % (grouping,))
        if int(capacity) < 1:
            raise ValueError("capacity must be at least 1 row")
        self.grouping = grouping
        self.capacity = int(capacity)
        self.group = None if group_mean is None else (group_mean, group_std)
        self.truth_min = float("nan") if s_small is None else float(s_small)
        self.clamp_min = float("nan") if self.group is None else 0.0
        self.min_s = float(config.get("min_s", 1e-4)) if self.group is None else -1.0
        self.null_val = 0.0 if self.group is None else float("nan")
        self.regions = regions
        self.affine = None                                    # (mean, std) of the scaler, set by the first batch
        self.margin: Optional[torch.Tensor] = None            # (out,) or (out, N, od) float32
        self.count: Optional[torch.Tensor] = None             # the same shape, int32
        self.clear()

    def clear(self):
        """forget the calibration scores and the test counts (a fitted margin stays)"""
        self.result: Dict[str, float] = {}
        self._store: Optional[torch.Tensor] = None            # (capacity, out, N, od) scores, rows 0 .. _rows - 1 filled
        self._rows = 0
        self._batch_scores: Optional[torch.Tensor] = None     # the scores of one test batch
        self._test_counts: Optional[torch.Tensor] = None      # (*group, 2) int64
        self.len_timeslots = 0

    def _scores(self, samples, y, y_start, mean, std, label_start, out):
        if (mean is None) != (std is None):
            raise ValueError("mean and std come as a pair")
        on_device = any(isinstance(v, torch.Tensor) and v.is_cuda for v in (mean, std) + tuple(self.affine or ()))
        if self.affine is None:
            self.affine = (mean, std)
        elif not on_device and not (_same_vector(self.affine[0], mean) and _same_vector(self.affine[1], std)):
            # (device tensors are taken on trust here: comparing them would read the device on every batch)
            raise ValueError("this calibrator collects on the scale mean, std = %s, got %s" % (self.affine, (mean, std)))
        if self.regions is not None:
            totals, labels = _region_totals(self.regions, samples, y, y_start, mean, std, self.group, self.clamp_min,
                                            label_start)
            return mc_conformity(totals, labels, self.probs, 0, clamp_min=float("nan"), truth_min=self.truth_min,
                                 min_s=-1.0, null_val=float("nan"), out=out)
        gm, gs = self.group if self.group is not None else (None, None)
        return mc_conformity(samples, y, self.probs, y_start, mean, std, gm, gs, self.clamp_min, self.truth_min,
                             self.min_s, self.null_val, label_start, out=out)

    def _score_shape(self, samples, lead: int):
        """the shape of the scores of a batch of samples (S, B, out, N, od) from axis ``lead`` on"""
        shape = [int(v) for v in samples.shape]
        if self.regions is not None:
            shape[3] = self.regions.num_groups
        return tuple(shape[lead:])

    def collect_samples(self, samples, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """One calibration batch: arguments as ``NodeEvaluator.collect_samples``.  Appends its B rows of scores to the
        store, which doubles its capacity when full."""
        b, shape = int(samples.shape[1]), self._score_shape(samples, 2)
        if self._store is not None and tuple(self._store.shape[1:]) != shape:
            raise ValueError("batch of shape %s after batches of shape %s" % (shape, tuple(self._store.shape[1:])))
        need, have = self._rows + b, 0 if self._store is None else int(self._store.shape[0])
        if need > have:
            grown = max(have, self.capacity)
            while grown < need:
                grown *= 2
            store = torch.empty((grown,) + shape, dtype=torch.float32, device=samples.device)
            if self._rows:
                store[:self._rows].copy_(self._store[:self._rows])
            self._store = store
        self._scores(samples, y, y_start, mean, std, label_start, self._store[self._rows:need])
        self._rows = need
        self.len_timeslots = shape[0]

    def fit(self):
        """margin and count per group from the scores collected so far, as device tensors"""
        if self._store is None:
            raise RuntimeError("nothing collected: call collect_samples first")
        self.margin, self.count = conformal_quantile(self._store, self._rows, self.grouping, self.coverage)
        self._test_counts = None
        return self.margin, self.count

    def _fitted(self):
        if self.margin is None:
            raise RuntimeError("not fitted: call fit (or load_state_dict) first")
        return self.margin

    def apply(self, quantiles: torch.Tensor) -> torch.Tensor:
        """A copy of ``quantiles`` (levels, ..., out, N, od) with the first level lowered and the last raised by the
        margin (one float32 rounding each; inner levels untouched), the two then held at the calibrator's clamp."""
        margin = self._fitted().to(quantiles.device)
        if quantiles.shape[0] != len(self.probs) or quantiles.dim() < 4:
            raise ValueError("quantiles of shape %s are not %d levels of (..., out, N, od)" % (tuple(quantiles.shape),
                                                                                               len(self.probs)))
        m = margin.reshape(-1, 1, 1) if self.grouping == "horizon" else margin
        out = quantiles.clone()
        out[0] = quantiles[0] - m
        out[-1] = quantiles[-1] + m
        if self.clamp_min == self.clamp_min:
            out[0].clamp_(min=self.clamp_min)
            out[-1].clamp_(min=self.clamp_min)
        return out

    def check_call(self, probs, affine, group_mean, group_std, clamp_min, regions=None):
        """ValueError unless a band of levels ``probs`` on the scale (affine, group pair, clamp), of the totals of
        ``regions`` (None: per node), is one this calibrator's margin applies to"""
        if (self.regions is None) != (regions is None) or (regions is not None and self.regions != regions):
            raise ValueError("the calibrator was fitted on %s, the call asks for %s"
                             % ("nodes" if self.regions is None else self.regions, "nodes" if regions is None else regions))
        if _check_probs(probs) != self.probs:
            raise ValueError("the calibrator was built for the levels %s, the call asks for %s" % (self.probs, tuple(probs)))
        mine = self.affine if self.affine is not None else (None, None)
        theirs = affine if affine is not None else (None, None)
        ident = lambda pair: (0.0, 1.0) if pair[0] is None else pair
        if not (_same_vector(ident(mine)[0], ident(theirs)[0]) and _same_vector(ident(mine)[1], ident(theirs)[1])):
            raise ValueError("the calibrator's scores are on the scale mean, std = %s, the band on %s" % (mine, theirs))
        gm, gs = self.group if self.group is not None else (None, None)
        if not (_same_vector(gm, group_mean) and _same_vector(gs, group_std) and _same_scalar(self.clamp_min, clamp_min)):
            raise ValueError("the calibrator's re-transform (group_mean / group_std, clamp_min = %s) differs from the call's"
                             % (self.clamp_min,))

    def collect_test_samples(self, samples, y, y_start: int = 0, mean=None, std=None, label_start=None):
        """One test batch: counts per group how many of its valid scores the fitted margin covers."""
        margin = self._fitted().to(samples.device)
        shape = self._score_shape(samples, 1)
        if self._batch_scores is None or tuple(self._batch_scores.shape) != shape:
            self._batch_scores = torch.empty(shape, dtype=torch.float32, device=samples.device)
        scores = self._scores(samples, y, y_start, mean, std, label_start, self._batch_scores)
        self._test_counts = conformal_coverage(scores, shape[0], self.grouping, margin.contiguous(), self._test_counts)
        self.len_timeslots = shape[1]

    def coverage_table(self) -> torch.Tensor:
        """PICP of the calibrated band per group, (out,) or (out, N, od) float64 on the CPU; NaN without a valid label"""
        if self._test_counts is None:
            raise RuntimeError("nothing collected: call collect_test_samples first")
        c = self._test_counts.cpu().double()
        return torch.where(c[..., 0] > 0, c[..., 1] / c[..., 0], torch.full_like(c[..., 0], float("nan")))

    def infinite_margins(self) -> torch.Tensor:
        """(out,) int64 on the CPU: the groups of each horizon whose margin is +inf (k > n)"""
        inf = torch.isinf(self._fitted()).cpu()
        return inf.reshape(inf.shape[0], -1).sum(1)

    def evaluate(self) -> Dict[str, float]:
        """``PICP@k`` of the calibrated band per horizon (element groups pooled) and ``INF_MARGINS@k``"""
        if self._test_counts is None:
            raise RuntimeError("nothing collected: call collect_test_samples first")
        c = self._test_counts.cpu()
        c = c.reshape(c.shape[0], -1, 2).sum(1).double()
        inf = self.infinite_margins()
        for i in range(c.shape[0]):
            self.result["PICP@%d" % (i + 1)] = float(c[i, 1] / c[i, 0]) if c[i, 0] > 0 else float("nan")
            self.result["INF_MARGINS@%d" % (i + 1)] = int(inf[i])
        return self.result

    def state_dict(self) -> Dict[str, object]:
        cpu = lambda v: None if v is None else torch.as_tensor(v, dtype=torch.float32).detach().cpu().clone()
        gm, gs = self.group if self.group is not None else (None, None)
        am, asd = self.affine if self.affine is not None else (None, None)
        return {"margin": None if self.margin is None else self.margin.detach().cpu().clone(),
                "count": None if self.count is None else self.count.detach().cpu().clone(),
                "probs": tuple(self.probs), "grouping": self.grouping,
                "regions": None if self.regions is None else self.regions.state_dict(),
                "scale": {"mean": cpu(am), "std": cpu(asd), "group_mean": cpu(gm), "group_std": cpu(gs),
                          "clamp_min": self.clamp_min, "truth_min": self.truth_min, "min_s": self.min_s,
                          "null_val": self.null_val}}

    def load_state_dict(self, state):
        probs = _check_probs(state["probs"])
        if len(probs) < 2 or state["grouping"] not in ("horizon", "element"):
            raise ValueError("not a calibrator state: probs %s, grouping %r" % (probs, state["grouping"]))
        sc = state["scale"]
        self.probs, self.grouping = probs, state["grouping"]
        self.coverage = _f32(probs[-1]) - _f32(probs[0])
        self.group = None if sc["group_mean"] is None else (sc["group_mean"], sc["group_std"])
        self.affine = None if sc["mean"] is None else (sc["mean"], sc["std"])
        self.clamp_min, self.truth_min = float(sc["clamp_min"]), float(sc["truth_min"])
        self.min_s, self.null_val = float(sc["min_s"]), float(sc["null_val"])
        if state.get("regions") is None:
            self.regions = None
        else:
            from .regions import RegionMap
            self.regions = RegionMap.from_state_dict(state["regions"])
        self.margin = None if state["margin"] is None else state["margin"].clone()
        self.count = None if state["count"] is None else state["count"].clone()
        self.clear()


def groupstd_table(pred, y, group_mean, group_std, y_start: int = 0, mean=None, std=None, label_start=None,
                   s_small: float = 10.0, sums: Optional[torch.Tensor] = None):
    """The per-horizon table of the group-std re-transform (traffic_state_executor.py:293-322): values de-scaled by
    the scaler (mean / std), re-transformed per node (x * All_std + All_m, :307-308), predictions below 0 set to 0
    (:312), only elements with truth_t > s_small kept (:316-317), then MAE / MSE / RMSE (loss.masked_*_np with their
    default NaN null value: plain means), R2 / EVAR with prediction and truth EXCHANGED as the reference passes them to
    sklearn (:318-319), MAPE.  Returns (columns dict of (out,) float64 CPU tensors, the running sums to pass back in
    for the next batch)."""
    sums = metric_sums(pred, y, y_start, mean, std, group_mean, group_std, clamp_min=0.0, truth_min=s_small, min_s=-1.0,
                       label_start=label_start, sums=sums)
    t = metric_table(sums, swap_r2=True)[0].cpu()
    col = ALLOWED_METRICS.index
    return {"MAE": t[:, col("MAE")], "MSE": t[:, col("MSE")], "RMSE": t[:, col("RMSE")], "R2": t[:, col("R2")],
            "EVAR": t[:, col("EVAR")], "MAPE": t[:, col("MAPE")]}, sums
