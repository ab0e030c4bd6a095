#!/usr/bin/env python3
"""Training-objective fixtures produced by THE REFERENCE'S OWN loss functions:

    PYTHONPATH=<reference checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_train_loss_golden.py

The eleven differentiable closures of TrafficStateExecutor._build_train_loss (libcity/executor/
traffic_state_executor.py:200-250) on small continuous inputs, each in float64 and in float32: value and autograd
gradient w.r.t. the scaled prediction.  The executor module cannot be imported without ray / tensorboard (as in
make_metrics_golden.py), so ``closure`` below repeats what its ``func`` does - inverse_transform of label and prediction
with a StandardScaler's affine, then the function of libcity.model.loss that the name selects, with the null value the
executor binds - around the reference's own loss functions.
Stored: the inputs and, per name, value and gradient - arrays only -> train_loss_small.npz.
"""
import os
from functools import partial

import numpy as np
import torch

from libcity.model import loss

HERE = os.path.dirname(os.path.abspath(__file__))
SELECT = {
    "mae": loss.masked_mae_torch, "mse": loss.masked_mse_torch, "rmse": loss.masked_rmse_torch,
    "mape": loss.masked_mape_torch, "logcosh": loss.log_cosh_loss, "huber": loss.huber_loss,
    "quantile": loss.quantile_loss,
    "masked_mae": partial(loss.masked_mae_torch, null_val=0), "masked_mse": partial(loss.masked_mse_torch, null_val=0),
    "masked_rmse": partial(loss.masked_rmse_torch, null_val=0), "masked_mape": partial(loss.masked_mape_torch, null_val=0),
}
ZERO_FREE = ("mape", "logcosh", "huber", "quantile")     # labels without zeros: an unmasked zero label makes mape inf
B, OUT, N = 3, 4, 37
MEAN, STD = 14.41, 29.3


def closure(name, pred, y, dtype):
    """(value, d value / d pred) of the executor's closure for ``name`` in ``dtype``"""
    p = torch.tensor(pred, dtype=dtype, requires_grad=True)
    y_true = torch.tensor(y, dtype=dtype) * STD + MEAN         # StandardScaler.inverse_transform
    y_pred = p * STD + MEAN
    v = SELECT[name](y_pred, y_true)
    v.backward()
    return v.detach().numpy(), p.grad.numpy()


def main():
    rng = np.random.default_rng(23)
    y = rng.standard_normal((B, OUT, N, 1)).astype(np.float32)
    pred = (y + 0.3 * rng.standard_normal((B, OUT, N, 1))).astype(np.float32)
    yz = y.copy()
    yz[0, :, :3, 0] = np.float32(-MEAN / STD)                  # de-scales to (almost) exactly 0: zeroed by min_s
    yz[1, 2, 5, 0] = np.float32((5e-5 - MEAN) / STD)           # |label| < min_s after de-scaling
    pz = pred.copy()
    pz[1, 3, 7, 0] = yz[1, 3, 7, 0]                            # p == l
    d = (pred.astype(np.float64) - y.astype(np.float64)) * STD
    assert np.abs(d).max() < 80.0, "the reference's float32 log(cosh(d)) must stay finite"
    out = dict(pred=pred, y=y, pred_z=pz, y_z=yz, mean=np.float64(MEAN), std=np.float64(STD))
    for name in SELECT:
        a, b = (pred, y) if name in ZERO_FREE else (pz, yz)
        v64, g64 = closure(name, a, b, torch.float64)
        v32, g32 = closure(name, a, b, torch.float32)
        assert np.isfinite(v64) and np.isfinite(v32), name
        out[name + "_value64"], out[name + "_grad64"] = np.float64(v64), g64.astype(np.float64)
        out[name + "_value32"], out[name + "_grad32"] = np.float32(v32), g32.astype(np.float32)
        print("%-12s %.12g  (float32 %.9g)  finite gradients %d / %d" % (name, v64, v32, np.isfinite(g64).sum(), g64.size))
    path = os.path.join(HERE, "train_loss_small.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
