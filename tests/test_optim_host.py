"""The device-side optimizer step on the host: the library surface (symbols, header, binding), every argument check of the
three entry points - they run before any launch, so they need no GPU -, the argument errors of ClipAdam / build_optimizer
and of the ops wrappers, and the reference against itself: torch's float32 CPU run against its float64 run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import optim_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("matgcn_grad_norm_bytes", "matgcn_grad_norm", "matgcn_adam_step")
OK, ERR_NULL, ERR_BAD_ARG, ERR_SMALL_BUFFER = 0, -1, -2, -4
PTR = 4096     # a non-NULL pointer nothing dereferences: every call below fails before its launch
NAN = float("nan")


def _table(numels, **null):
    """matgcn_opt_tensor array with dummy pointers; null = field -> index of the tensor that gets NULL there"""
    from multistgraph_amd import _lib
    arr = (_lib.OptTensor * max(1, len(numels)))()
    for i, n in enumerate(numels):
        arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq, arr[i].numel = PTR, PTR, PTR, PTR, n
    for field, i in null.items():
        setattr(arr[i], field, None)
    return arr


def _hp(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=5.0, step=1):
    from multistgraph_amd import _lib
    return _lib.Adam(lr, beta1, beta2, eps, weight_decay, max_norm, step)


def test_library_exports_and_binding(lib_built):
    from multistgraph_amd import _lib, ops, optim
    with open(os.path.join(ROOT, "include", "matgcn.h")) as fh:
        header = fh.read()
    lib = _lib.load()
    for name in NEW_FUNCTIONS:
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name
        assert "int %s(" % name in header, name
    assert "} matgcn_opt_tensor;" in header and "} matgcn_adam;" in header
    assert "Still ABI 12: new names only" in header
    assert "`grad` is NEVER written" in header
    assert "#define MATGCN_ABI_VERSION 12" in header and lib.matgcn_abi_version() == 12 == _lib.ABI_VERSION
    assert C.sizeof(_lib.OptTensor) == 40 and C.sizeof(_lib.Adam) == 32
    assert [f[0] for f in _lib.OptTensor._fields_] == ["param", "grad", "exp_avg", "exp_avg_sq", "numel"]
    assert [f[0] for f in _lib.Adam._fields_] == ["lr", "beta1", "beta2", "eps", "weight_decay", "max_norm", "step"]
    assert _lib.OPT_CHUNK == 4096 and _lib.OPT_MAX_TENSORS == 64
    assert callable(ops.grad_norm) and callable(ops.adam_step)
    assert issubclass(optim.ClipAdam, torch.optim.Optimizer) and callable(optim.build_optimizer)
    with open(os.path.join(ROOT, "multistgraph_amd", "build.py")) as fh:
        assert '"matgcn_optim.hip"' in fh.read()


def _bytes(lib, numels):
    need = C.c_size_t(0)
    return lib.matgcn_grad_norm_bytes(_table(numels), len(numels), C.byref(need)), need.value


def test_scratch_size(lib_built):
    """8 bytes per chunk of 4096 elements; every tensor is rounded up to whole chunks, an empty one has none"""
    from multistgraph_amd import _lib
    lib = _lib.load()
    for numel, chunks in ((0, 0), (1, 1), (4096, 1), (4097, 2)):
        assert _bytes(lib, [numel]) == (OK, 8 * chunks), numel
    assert _bytes(lib, [1] * 65) == (OK, 8 * 65)
    assert _bytes(lib, [4097, 0, 1, 8192, 8193]) == (OK, 8 * (2 + 0 + 1 + 2 + 3))
    assert lib.matgcn_grad_norm_bytes(_table([5]), 1, None) == ERR_NULL
    assert lib.matgcn_grad_norm_bytes(None, 1, C.byref(C.c_size_t(0))) == ERR_NULL
    for n in (0, -1):
        assert lib.matgcn_grad_norm_bytes(_table([5]), n, C.byref(C.c_size_t(0))) == ERR_BAD_ARG
    assert _bytes(lib, [5, -1])[0] == ERR_BAD_ARG
    need = C.c_size_t(0)
    assert lib.matgcn_grad_norm_bytes(_table([5, 7], grad=1), 2, C.byref(need)) == ERR_NULL
    # the norm reads grad and numel only
    assert lib.matgcn_grad_norm_bytes(_table([5, 7], param=0, exp_avg=1, exp_avg_sq=1), 2, C.byref(need)) == OK


def test_norm_arguments_are_checked_on_the_host(lib_built):
    from multistgraph_amd import _lib
    lib = _lib.load()

    def norm(t=None, n=2, scratch=PTR, scratch_bytes=1 << 40, total=PTR, numels=(5000, 3)):
        t = _table(numels) if t is None else t
        return lib.matgcn_grad_norm(t, n, scratch, scratch_bytes, total, None)

    assert lib.matgcn_grad_norm(None, 2, PTR, 1 << 40, PTR, None) == ERR_NULL
    assert norm(total=None) == ERR_NULL
    assert norm(scratch=None) == ERR_NULL
    assert norm(t=_table([5000, 3], grad=0)) == ERR_NULL
    for n in (0, -3):
        assert norm(n=n) == ERR_BAD_ARG, n
    assert norm(numels=(5000, -1)) == ERR_BAD_ARG
    assert norm(scratch_bytes=8 * 3 - 1) == ERR_SMALL_BUFFER     # 2 + 1 chunks
    assert norm(scratch_bytes=0) == ERR_SMALL_BUFFER


def test_adam_arguments_are_checked_on_the_host(lib_built):
    from multistgraph_amd import _lib
    lib = _lib.load()

    def adam(t=None, n=2, hp=None, total=PTR, numels=(5000, 3), **kw):
        t = _table(numels) if t is None else t
        hp = _hp(**kw) if hp is None else hp
        return lib.matgcn_adam_step(t, n, C.byref(hp), total, None)

    assert lib.matgcn_adam_step(None, 2, C.byref(_hp()), PTR, None) == ERR_NULL
    assert lib.matgcn_adam_step(_table([5]), 1, None, PTR, None) == ERR_NULL
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert adam(t=_table([5000, 3], **{field: 1})) == ERR_NULL, field
    for n in (0, -1):
        assert adam(n=n) == ERR_BAD_ARG, n
    assert adam(numels=(5000, -1)) == ERR_BAD_ARG
    for bad in (dict(lr=-1e-3), dict(lr=NAN), dict(eps=-1e-8), dict(eps=NAN), dict(weight_decay=-0.01),
                dict(weight_decay=NAN), dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=NAN), dict(beta2=-0.1),
                dict(beta2=1.0), dict(beta2=1.5), dict(beta2=NAN), dict(step=0), dict(step=-4), dict(max_norm=NAN)):
        assert adam(**bad) == ERR_BAD_ARG, bad
    assert adam(total=None, max_norm=5.0) == ERR_NULL
    # (max_norm <= 0 with total_norm NULL, and a table of empty tensors with NULL pointers, are valid calls: they launch,
    # so the GPU tests make them)


def _param(n=4, **kw):
    return torch.nn.Parameter(torch.zeros(n, **kw))


def test_clipadam_argument_errors(lib_built):
    from multistgraph_amd.optim import ClipAdam
    p = _param()
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(betas=(0.9,)),
                dict(weight_decay=-0.1), dict(max_grad_norm=0), dict(max_grad_norm=-5), dict(max_grad_norm=NAN),
                dict(amsgrad=True), dict(maximize=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            ClipAdam([p], **bad)
    opt = ClipAdam([{"params": [p], "lr": 0.5}, {"params": [_param()]}], lr=3e-3, max_grad_norm=5)
    assert opt.param_groups[0]["lr"] == 0.5 and opt.param_groups[1]["lr"] == 3e-3 and opt.max_grad_norm == 5.0
    assert opt.last_grad_norm is None
    assert set(opt.param_groups[0]) == set(torch.optim.Adam([_param()]).param_groups[0])
    assert opt.step() is None and len(opt.state) == 0            # no gradient anywhere: nothing to do, nothing launched
    # CPU tensors, other dtypes, sparse gradients and options a loaded state_dict switched on are refused, never emulated
    p.grad = torch.ones(4)
    with pytest.raises(ValueError, match="GPU"):
        opt.step()
    q = _param()
    q.grad = torch.sparse_coo_tensor([[1]], [1.0], (4,))
    with pytest.raises(ValueError, match="sparse"):
        ClipAdam([q]).step()
    for key in ("amsgrad", "maximize"):
        o = ClipAdam([p])
        o.param_groups[0][key] = True
        with pytest.raises(ValueError):
            o.step()


def test_ops_argument_errors(lib_built):
    from multistgraph_amd import ops
    cpu = torch.zeros(8)
    with pytest.raises(ValueError, match="GPU"):
        ops.grad_norm([cpu])
    with pytest.raises(ValueError):
        ops.grad_norm([])
    with pytest.raises(ValueError):
        ops.grad_norm([np.zeros(3, np.float32)])
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, step=1)
    with pytest.raises(ValueError, match="GPU"):
        ops.adam_step([cpu], [cpu], [cpu], [cpu], **kw)
    with pytest.raises(ValueError):
        ops.adam_step([cpu, cpu], [cpu], [cpu], [cpu], **kw)


class _Config:
    """LibCity's ConfigParser offers get() and no keys()"""

    def __init__(self, **kw):
        self._kw = kw

    def get(self, key, default=None):
        return self._kw.get(key, default)


def test_build_optimizer(lib_built):
    from multistgraph_amd.optim import ClipAdam, build_optimizer
    model = torch.nn.Linear(3, 2)
    opt = build_optimizer(_Config(), model)       # the executor's defaults (traffic_state_executor.py:50-70)
    g = opt.param_groups[0]
    assert isinstance(opt, ClipAdam) and opt.max_grad_norm is None
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (0.01, (0.9, 0.999), 1e-8, 0)
    assert len(g["params"]) == 2
    assert build_optimizer(_Config(clip_grad_norm=True), model).max_grad_norm == 1.0
    assert build_optimizer(_Config(clip_grad_norm=False, max_grad_norm=5), model).max_grad_norm is None
    opt = build_optimizer(_Config(learner="Adam", learning_rate=0.003, lr_beta1=0.8, lr_beta2=0.99, lr_epsilon=1e-6,
                                  weight_decay=0.01, clip_grad_norm=True, max_grad_norm=5), model)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], opt.max_grad_norm) == (0.003, (0.8, 0.99), 1e-6, 0.01, 5.0)
    for learner in ("sgd", "adagrad", "rmsprop", "sparse_adam", "adamw"):
        with pytest.raises(ValueError):
            build_optimizer(_Config(learner=learner), model)


def test_state_dict_exchange_with_torch_adam(lib_built):
    """the formats only (no step runs here): a ClipAdam state_dict loads into torch.optim.Adam and back"""
    from multistgraph_amd.optim import ClipAdam
    ps = [_param(3), _param(5)]
    adam = torch.optim.Adam(ps, lr=0.003)
    for p in ps:
        p.grad = torch.ones_like(p)
    adam.step()
    mine = ClipAdam(ps, lr=0.5, max_grad_norm=5)
    mine.load_state_dict(adam.state_dict())
    assert mine.param_groups[0]["lr"] == 0.003 and float(mine.state[ps[1]]["step"]) == 1.0
    assert torch.equal(mine.state[ps[0]]["exp_avg"], adam.state[ps[0]]["exp_avg"])
    back = torch.optim.Adam(ps, lr=0.7)
    back.load_state_dict(mine.state_dict())
    back.step()
    assert back.param_groups[0]["lr"] == 0.003 and float(back.state[ps[0]]["step"]) == 2.0


@pytest.mark.parametrize("max_norm", [None, 5.0])
def test_float32_reference_against_float64(max_norm):
    """the reference against itself: 20 steps at the recipe's settings, the float32 run stays within a few ulp of the
    float64 run, and the gap is not 0 (it is the unit of the GPU tolerance)"""
    shapes = [(1,), (3,), (1023,), (1025,)]
    params, _ = R.make_set(shapes, 7)
    rng = np.random.default_rng(8)
    steps = [[((30.0 if s % 2 else 0.05) * rng.standard_normal(sh)).astype(np.float32) for sh in shapes] for s in range(20)]
    kept = [p.copy() for p in params]
    ref64, G = R.reference(params, steps, max_norm=max_norm, **R.HP)
    assert all(np.array_equal(a, b) for a, b in zip(params, kept))      # the runs work on copies of their inputs
    print("max_norm %s: G param %.3e, exp_avg %.3e, exp_avg_sq %.3e; largest |param| %.2f, clipped steps %d"
          % (max_norm, G["param"], G["exp_avg"], G["exp_avg_sq"], max(float(np.abs(p).max()) for p in ref64["param"]),
             sum(n > max_norm for n in ref64["norms"]) if max_norm else 0))
    for kind in R.KINDS:
        scale = max(float(np.abs(a).max()) for a in ref64[kind])
        assert 0 < G[kind] <= 64 * np.finfo(np.float32).eps * scale, kind
    if max_norm:
        assert any(n > max_norm for n in ref64["norms"]) and any(n < max_norm for n in ref64["norms"])
        for got, grads in zip(ref64["norms"], steps):
            assert abs(got - R.norm64(grads)) <= 1e-12 * got
