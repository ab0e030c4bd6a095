"""The optimizer step of the training recipe on the HIP path: ``clip_grad_norm_`` + ``torch.optim.Adam`` as one
``step()`` of three launches (matgcn_grad_norm, matgcn_adam_step; include/matgcn.h).

    optimizer = ClipAdam(model.parameters(), lr=0.003, max_grad_norm=5)      # in place of torch.optim.Adam(...)
    loss = model.calculate_loss(batch); loss.backward(); optimizer.step()    # no clip_grad_norm_ call in between

The state (``step``, ``exp_avg``, ``exp_avg_sq``) and the param groups are torch.optim.Adam's: a ``state_dict()`` of one
loads into the other, and schedulers that edit ``group['lr']`` work unchanged.  Unlike ``clip_grad_norm_`` the step leaves
``p.grad`` as the backward wrote it: the clip coefficient is applied while the gradients are read.
"""
from __future__ import annotations

import torch

from . import ops

try:
    _set_versions = torch._C._autograd._unsafe_set_version_counter
except AttributeError:   # an older torch: an in-place no-op through torch bumps the counters as well
    _set_versions = None


def _bump_versions(params) -> None:
    """The kernels write the parameters behind torch's back; everything that detects an update from ``p._version``
    (MultiATGCN._params_key, autograd's saved-tensor check) has to see one, as after torch's own in-place step."""
    if _set_versions is not None:
        _set_versions(tuple(params), tuple(p._version + 1 for p in params))
    else:
        torch._foreach_mul_(list(params), 1.0)


class ClipAdam(torch.optim.Optimizer):
    """torch.optim.Adam (L2 weight decay, no amsgrad, no maximize) with the global-norm clip in front of it, on the device.

    ``max_grad_norm``: None - plain Adam, one launch per 64 tensors (for a loop that still calls ``clip_grad_norm_``
    itself); a positive number - the gradients of every parameter with a gradient, over all groups, are clipped to this
    2-norm as ``clip_grad_norm_(model.parameters(), max_grad_norm)`` would, and ``last_grad_norm`` holds the norm before
    clipping as a 0-dim device tensor (nothing is synchronised to read it)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, max_grad_norm=None, *,
                 amsgrad=False, maximize=False):
        if isinstance(lr, torch.Tensor):
            raise ValueError("ClipAdam: lr must be a number (a tensor lr would have to be read back every step)")
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: %r" % (lr,))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: %r" % (eps,))
        if len(betas) != 2 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameters: %r" % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError("Invalid weight_decay value: %r" % (weight_decay,))
        if amsgrad or maximize:
            raise ValueError("ClipAdam: amsgrad and maximize are not built (DESIGN.md section 7); use torch.optim.Adam")
        if max_grad_norm is not None and not float(max_grad_norm) > 0:
            raise ValueError("Invalid max_grad_norm: %r (None switches the clip off)" % (max_grad_norm,))
        # the keys of torch.optim.Adam's groups, so that the two optimizers read each other's state_dict()
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.last_grad_norm = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        buckets = {}     # (group index, step count) -> params, grads, exp_avgs, exp_avg_sqs, step tensors
        all_grads = []
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("decoupled_weight_decay"):
                raise ValueError("ClipAdam: amsgrad, maximize and decoupled weight decay are not built")
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                if g.is_sparse:
                    raise ValueError("ClipAdam does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = torch.tensor(0.0, dtype=torch.float32)      # as torch.optim.Adam stores it
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                b = buckets.setdefault((gi, int(state["step"].item()) + 1), ([], [], [], [], []))
                b[0].append(p); b[1].append(g); b[2].append(state["exp_avg"]); b[3].append(state["exp_avg_sq"])
                b[4].append(state["step"])
                all_grads.append(g)
        if not all_grads:
            return loss
        norm = None
        if self.max_grad_norm is not None:
            norm = self.last_grad_norm = ops.grad_norm(all_grads)
        updated = []
        for (gi, step), (params, grads, exp_avgs, exp_avg_sqs, steps) in buckets.items():
            group = self.param_groups[gi]
            ops.adam_step(params, grads, exp_avgs, exp_avg_sqs, lr=group["lr"], betas=group["betas"], eps=group["eps"],
                          weight_decay=group["weight_decay"], step=step, max_norm=self.max_grad_norm, total_norm=norm)
            torch._foreach_add_(steps, 1)
            updated += params
        _bump_versions(updated)
        return loss


def build_optimizer(config, model) -> ClipAdam:
    """ClipAdam from the executor's config keys, with the executor's defaults: ``learner`` (only 'adam'),
    ``learning_rate`` (0.01), ``lr_beta1`` / ``lr_beta2`` (0.9, 0.999), ``lr_epsilon`` (1e-8), ``weight_decay`` (0),
    ``clip_grad_norm`` (False) and ``max_grad_norm`` (1.0).  ``config`` only needs ``get``."""
    learner = str(config.get("learner", "adam")).lower()
    if learner != "adam":
        raise ValueError("learner = %r: only 'adam' has a device-side step (DESIGN.md section 7)" % (learner,))
    clip = config.get("max_grad_norm", 1.0) if config.get("clip_grad_norm", False) else None
    return ClipAdam(model.parameters(), lr=config.get("learning_rate", 0.01),
                    betas=(config.get("lr_beta1", 0.9), config.get("lr_beta2", 0.999)), eps=config.get("lr_epsilon", 1e-8),
                    weight_decay=config.get("weight_decay", 0), max_grad_norm=clip)
