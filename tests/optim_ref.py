"""Reference of the device-side optimizer step (matgcn_grad_norm / matgcn_adam_step, multistgraph_amd.optim.ClipAdam):
torch's own ``clip_grad_norm_`` + ``torch.optim.Adam`` on the CPU (single-tensor code path, foreach off), in float64 and in
float32, fed the same fp32 starting values and gradients.

The tolerance of the GPU tests is measured with it, not fixed: G = the largest absolute gap of the float32 run to the
float64 run, separately for ``param``, ``exp_avg`` and ``exp_avg_sq``; the fused result has to lie within 2 G of the
float64 run, element-wise - the margin tests/test_bf16x3.py gives a differently ordered but equally rounded computation.
A missed or doubly updated element is off by about lr, a thousand times more."""
import numpy as np
import torch

KINDS = ("param", "exp_avg", "exp_avg_sq")
HP = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)     # the recipe's Adam


def make_set(shapes, seed, scale=1.0, grad_scale=1.0):
    """fp32 starting values and one gradient per shape from a seeded generator"""
    rng = np.random.default_rng(seed)
    params = [(scale * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    grads = [(grad_scale * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    return params, grads


def make_state(shapes, seed):
    """a plausible mid-training state: exp_avg of either sign, exp_avg_sq positive"""
    rng = np.random.default_rng(seed)
    m = [(0.3 * rng.standard_normal(s)).astype(np.float32) for s in shapes]
    v = [(0.1 * rng.random(s) + 1e-3).astype(np.float32) for s in shapes]
    return m, v


def run(params, grad_steps, dtype, *, lr=HP["lr"], betas=HP["betas"], eps=HP["eps"], weight_decay=0.0, max_norm=None,
        exp_avg=None, exp_avg_sq=None, step0=0, milestones=None, gamma=None):
    """``len(grad_steps)`` steps of clip_grad_norm_(max_norm) + torch.optim.Adam in ``dtype`` on the CPU.
    params: list of fp32 arrays; grad_steps: per step a list with one fp32 array (or None: no gradient) per parameter;
    exp_avg / exp_avg_sq / step0: the state to start from (default: none, as a new optimizer).
    Returns dict(param, exp_avg, exp_avg_sq: lists of float64 arrays (None where no state arose), norms: float64 list)."""
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(p, copy=True)).to(dtype)) for p in params]   # never the caller's memory
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    if exp_avg is not None:
        for p, m, v in zip(ps, exp_avg, exp_avg_sq):
            opt.state[p] = dict(step=torch.tensor(float(step0)), exp_avg=torch.from_numpy(m.copy()).to(dtype),
                                exp_avg_sq=torch.from_numpy(v.copy()).to(dtype))
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones, gamma) if milestones else None
    norms = []
    for grads in grad_steps:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g.copy()).to(dtype)
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False).double()))
        opt.step()
        if sched is not None:
            sched.step()
    out = dict(norms=norms, param=[p.detach().double().numpy() for p in ps])
    for kind in KINDS[1:]:
        out[kind] = [opt.state[p][kind].double().numpy() if kind in opt.state[p] else None for p in ps]
    return out


def norm64(grads):
    """the float64 2-norm over every element of the fp32 arrays"""
    return float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads if g is not None)))


def gaps(ref32, ref64):
    """G per kind: the largest absolute gap of the float32 run to the float64 run"""
    out = {}
    for kind in KINDS:
        worst = 0.0
        for a, b in zip(ref32[kind], ref64[kind]):
            if b is not None and b.size:
                worst = max(worst, float(np.abs(a - b).max()))
        out[kind] = worst
    return out


def reference(params, grad_steps, **kw):
    """(float64 run, G per kind) of one case"""
    ref64 = run(params, grad_steps, torch.float64, **kw)
    ref32 = run(params, grad_steps, torch.float32, **kw)
    return ref64, gaps(ref32, ref64)


def worst_excess(got, ref64, G):
    """per kind: max over the elements of |got - float64| / (2 G) (<= 1 passes); ``got``: dict kind -> list of arrays.
    With G = 0 (nothing moved in either reference run) the result must be exact: 0 if it is, inf if not."""
    out = {}
    for kind in KINDS:
        worst = 0.0
        for a, b in zip(got[kind], ref64[kind]):
            if b is None or not b.size:
                continue
            err = float(np.abs(np.asarray(a, dtype=np.float64) - b).max())
            if not np.isfinite(err):
                worst = float("inf")
            elif err > 0:
                worst = max(worst, err / (2 * G[kind]) if G[kind] > 0 else float("inf"))
        out[kind] = worst
    return out
