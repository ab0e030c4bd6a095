"""The device-side optimizer step on the GPU: matgcn_grad_norm / matgcn_adam_step through ops.grad_norm / ops.adam_step and
multistgraph_amd.optim.ClipAdam, against torch's own clip_grad_norm_ + torch.optim.Adam on the CPU (tests/optim_ref.py).

Tolerance, measured per case and printed: G = the largest absolute gap of torch's float32 CPU run to its float64 run,
separately for param, exp_avg and exp_avg_sq; the fused result lies within 2 G of the float64 run, element-wise.  Every
case holds a tensor of at least 1024 elements and asserts G > 0 for each kind - except the one case in which nothing may
move at all (all-zero gradients on a new state), where G = 0 and the result has to be exact.  total_norm lies within one
fp32 ulp (np.spacing) of the float64 norm.  Every case is a few thousand elements and a handful of launches; the twenty
steps run 172 k elements."""
import ctypes as C

import numpy as np
import pytest
import torch

import optim_ref as R
from helpers import Case

pytestmark = pytest.mark.gpu

ERR_SMALL_BUFFER = -4
GUARD = 8                 # floats in front of and behind every buffer (a multiple of 4: the view's offset is its alignment)
SENTINEL = 12345.678


def _dev():
    return torch.device("cuda:0")


class _Guarded:
    """a device tensor of the values ``a`` as a view ``off`` floats into an aligned allocation, guard floats around it"""

    def __init__(self, a, off=0):
        n = a.size
        self.buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, dtype=torch.float32, device=_dev())
        assert self.buf.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.t = self.buf[self.lo:self.hi].view(a.shape)
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert self.t.is_contiguous() and (n == 0 or self.t.data_ptr() % 16 == 4 * (off % 4))

    def guards_intact(self):
        b = self.buf.cpu().numpy().view(np.int32)
        want = np.full(1, SENTINEL, np.float32).view(np.int32)[0]
        return np.array_equal(b[:self.lo], np.full(self.lo, want)) and np.array_equal(b[self.hi:], np.full(GUARD, want))

    def numpy(self):
        return self.t.cpu().numpy()


def _fused(params, grads, exp_avg, exp_avg_sq, step, max_norm, offs=(0, 0, 0, 0), **hp):
    """one fused step on guarded device copies -> (dict kind -> list of arrays, total_norm or None)"""
    from multistgraph_amd import ops
    P, G_, M, V = ([_Guarded(a, off) for a in arrs] for arrs, off in zip((params, grads, exp_avg, exp_avg_sq), offs))
    norm = ops.grad_norm([g.t for g in G_]) if max_norm is not None else None
    ops.adam_step([x.t for x in P], [x.t for x in G_], [x.t for x in M], [x.t for x in V], step=step, max_norm=max_norm,
                  total_norm=norm, **hp)
    torch.cuda.synchronize()
    for x in P + G_ + M + V:
        assert x.guards_intact()
    for g, a in zip(G_, grads):
        assert np.array_equal(g.numpy().view(np.int32), a.view(np.int32))     # grad is never written
    got = dict(param=[x.numpy() for x in P], exp_avg=[x.numpy() for x in M], exp_avg_sq=[x.numpy() for x in V])
    return got, (None if norm is None else float(norm.item()))


def _check(tag, got, ref64, G, exact=False):
    assert any(p.size >= 1024 for p in ref64["param"])
    ex = R.worst_excess(got, ref64, G)
    print("%s: G param %.3e exp_avg %.3e exp_avg_sq %.3e; |fused - fp64| / 2G: %.3f %.3f %.3f"
          % (tag, G["param"], G["exp_avg"], G["exp_avg_sq"], ex["param"], ex["exp_avg"], ex["exp_avg_sq"]))
    for kind in R.KINDS:
        if not exact:
            assert G[kind] > 0, kind
        assert ex[kind] <= 1.0, (kind, ex[kind], G[kind])


def _check_norm(got, grads):
    want = R.norm64(grads)
    print("total_norm %.9g, float64 %.17g, ulp %.3g" % (got, want, float(np.spacing(np.float32(want)))))
    assert abs(float(got) - want) <= float(np.spacing(np.float32(want)))


def _one_step(tag, shapes, seed, *, step=1, max_norm=5.0, grad_scale=1.0, offs=(0, 0, 0, 0), weight_decay=0.0):
    params, grads = R.make_set(shapes, seed, grad_scale=grad_scale)
    if step > 1:
        m, v = R.make_state(shapes, seed + 1)
    else:
        m, v = [np.zeros(s, np.float32) for s in shapes], [np.zeros(s, np.float32) for s in shapes]
    hp = dict(R.HP, weight_decay=weight_decay)
    ref64, G = R.reference(params, [grads], max_norm=max_norm, exp_avg=m, exp_avg_sq=v, step0=step - 1, **hp)
    got, norm = _fused(params, grads, m, v, step, max_norm, offs, **hp)
    _check(tag, got, ref64, G)
    if max_norm is not None:
        _check_norm(norm, grads)
    return ref64


# ---- shape edges -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 4096, 4097, 8193])
def test_single_tensor_sizes(n, lib_built):
    """a chunk's float4 body and scalar tail, one element short of / at / one past a chunk, three chunks"""
    _one_step("numel %d" % n, [(n,), (1024,)], 100 + n % 97, grad_scale=3.0)


TINY_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65)


@pytest.mark.parametrize("count", [1, 64, 65, 130])
def test_tensor_counts(count, lib_built):
    """one launch, a full table, one tensor past it, three launches"""
    shapes = [(TINY_SIZES[i % len(TINY_SIZES)],) for i in range(count)]
    shapes[count // 2] = (1024,)
    _one_step("%d tensors" % count, shapes, 200 + count, grad_scale=3.0)


def test_empty_tensors_are_skipped(lib_built):
    shapes = [(0,), (5,), (0,), (1024,), (3,), (0,)]
    ref64 = _one_step("with empty tensors", shapes, 300, grad_scale=3.0)
    assert ref64["param"][0].size == 0


# ---- alignment ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [1, 2, 3])
@pytest.mark.parametrize("which", range(4), ids=["param", "grad", "exp_avg", "exp_avg_sq"])
def test_views_at_any_float_offset(which, off, lib_built):
    """one of the four tensors of every entry starts ``off`` floats into its allocation: the scalar path, same result,
    and the guard floats around every buffer keep their bits (_fused checks them)"""
    offs = [0, 0, 0, 0]
    offs[which] = off
    _one_step("offset %d on %d" % (off, which), [(4099,), (1024,), (7,)], 400 + 4 * which + off, step=2, offs=tuple(offs),
              grad_scale=3.0)


def test_norm_does_not_depend_on_alignment(lib_built):
    from multistgraph_amd import ops
    _, grads = R.make_set([(4099,), (1024,), (7,)], 450)
    norms = []
    for off in (0, 1, 2, 3):
        g = [_Guarded(a, off) for a in grads]
        norms.append(ops.grad_norm([x.t for x in g]).cpu().numpy().view(np.int32).item())
        assert all(x.guards_intact() for x in g)
    assert len(set(norms)) == 1


# ---- clip regimes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("regime", ["below", "above", "off"])
def test_clip_regimes(regime, step, weight_decay, lib_built):
    shapes = [(1500,), (33,)]
    max_norm, scale = {"below": (5.0, 1e-3), "above": (5.0, 100.0), "off": (None, 1.0)}[regime]
    ref64 = _one_step("%s step %d wd %g" % (regime, step, weight_decay), shapes, 500 + step % 7, step=step, max_norm=max_norm,
                      grad_scale=scale, weight_decay=weight_decay)
    if regime == "below":
        assert ref64["norms"][0] < 0.1
    if regime == "above":
        assert ref64["norms"][0] > 1000


@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("step", [1, 2, 1000])
def test_zero_gradients(step, weight_decay, lib_built):
    """norm exactly 0; on a new state without weight decay nothing moves (G = 0: exact), otherwise the state and the
    decay move the parameters as torch moves them"""
    shapes = [(1500,), (33,)]
    params, _ = R.make_set(shapes, 600)
    grads = [np.zeros(s, np.float32) for s in shapes]
    m, v = R.make_state(shapes, 601) if step > 1 else ([np.zeros(s, np.float32) for s in shapes] for _ in range(2))
    hp = dict(R.HP, weight_decay=weight_decay)
    ref64, G = R.reference(params, [grads], max_norm=5.0, exp_avg=m, exp_avg_sq=v, step0=step - 1, **hp)
    got, norm = _fused(params, grads, m, v, step, 5.0, **hp)
    still = step == 1 and weight_decay == 0
    _check("zero gradients step %d wd %g" % (step, weight_decay), got, ref64, G, exact=still)
    assert norm == 0.0
    if still:
        assert G == dict(param=0.0, exp_avg=0.0, exp_avg_sq=0.0)
        for a, b, mm in zip(got["param"], params, got["exp_avg"]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)) and not mm.any()


# ---- scratch and untouched tensors -------------------------------------------------------------------------------------
def _raw_norm(grads, scratch, scratch_bytes, out):
    from multistgraph_amd import _lib
    lib = _lib.load()
    arr = (_lib.OptTensor * len(grads))()
    for i, g in enumerate(grads):
        arr[i].grad, arr[i].numel = g.data_ptr(), g.numel()
    need = C.c_size_t(0)
    assert lib.matgcn_grad_norm_bytes(arr, len(grads), C.byref(need)) == 0
    stream = C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)
    rc = lib.matgcn_grad_norm(arr, len(grads), C.c_void_p(scratch.data_ptr()),
                              C.c_size_t(need.value if scratch_bytes is None else need.value + scratch_bytes),
                              C.c_void_p(out.data_ptr()), stream)
    torch.cuda.synchronize()
    return rc, need.value


def test_scratch_contents_and_size(lib_built):
    from multistgraph_amd import ops
    _, grads = R.make_set([(4097,), (1024,), (3,)], 700, grad_scale=3.0)
    dev = [torch.from_numpy(g).to(_dev()) for g in grads]
    want = ops.grad_norm(dev)
    _check_norm(float(want.item()), grads)
    scratch = torch.full((4 + 2,), float("nan"), dtype=torch.float64, device=_dev())     # 4 chunks and two guards
    out = torch.full((3,), SENTINEL, dtype=torch.float32, device=_dev())
    rc, need = _raw_norm(dev, scratch[1:], None, out[1:])
    assert rc == 0 and need == 8 * 4
    assert out[1].item() == want.item()                         # NaN in the scratch reaches nothing
    assert out[0].item() == np.float32(SENTINEL) and out[2].item() == np.float32(SENTINEL)
    assert torch.isnan(scratch[0]) and torch.isnan(scratch[5]) and not torch.isnan(scratch[1:5]).any()
    # one byte short: refused on the host, nothing written
    scratch.fill_(float("nan"))
    out.fill_(SENTINEL)
    rc, _ = _raw_norm(dev, scratch[1:], -1, out[1:])
    assert rc == ERR_SMALL_BUFFER
    assert torch.isnan(scratch).all() and bool((out == np.float32(SENTINEL)).all())


def test_parameter_without_gradient(lib_built):
    from multistgraph_amd.optim import ClipAdam
    shapes = [(1025,), (40,), (7,)]
    params, grads = R.make_set(shapes, 710, grad_scale=3.0)
    grads[1] = None
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(_dev())) for p in params]
    opt = ClipAdam(ps, max_grad_norm=5, **R.HP)
    for p, g in zip(ps, grads):
        p.grad = None if g is None else torch.from_numpy(g).to(_dev())
    before = [p._version for p in ps]
    opt.step()
    assert [p._version - b for p, b in zip(ps, before)] == [1, 0, 1]
    assert ps[1] not in opt.state and np.array_equal(ps[1].detach().cpu().numpy().view(np.int32), params[1].view(np.int32))
    ref64, G = R.reference(params, [grads], max_norm=5.0, **R.HP)
    got = {k: [None if g is None else opt.state[p][k].cpu().numpy() for p, g in zip(ps, grads)] for k in R.KINDS[1:]}
    got["param"] = [p.detach().cpu().numpy() for p in ps]
    _check("parameter without gradient", got, ref64, G)
    _check_norm(float(opt.last_grad_norm.item()), grads)
    assert [float(opt.state[p]["step"]) for p in (ps[0], ps[2])] == [1.0, 1.0]


def test_step_counts_that_differ_go_in_separate_launches(lib_built):
    """a parameter that joins later (no gradient in the first step) has its own bias correction, as in torch"""
    from multistgraph_amd.optim import ClipAdam
    shapes = [(1025,), (40,)]
    params, g1 = R.make_set(shapes, 720, grad_scale=3.0)
    _, g2 = R.make_set(shapes, 721, grad_scale=0.01)
    steps = [[g1[0], None], g2]
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(_dev())) for p in params]
    opt = ClipAdam(ps, max_grad_norm=5, **R.HP)
    for grads in steps:
        for p, g in zip(ps, grads):
            p.grad = None if g is None else torch.from_numpy(g).to(_dev())
        opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [2.0, 1.0]
    ref64, G = R.reference(params, steps, max_norm=5.0, **R.HP)
    got = {k: [opt.state[p][k].cpu().numpy() for p in ps] for k in R.KINDS[1:]}
    got["param"] = [p.detach().cpu().numpy() for p in ps]
    _check("differing step counts", got, ref64, G)


def test_ops_refuse_what_they_cannot_update_in_place(lib_built):
    """float32, contiguous, on the device - anything else is a ValueError, never a converted copy"""
    from multistgraph_amd import ops
    good = [torch.zeros(8, device=_dev()) for _ in range(4)]
    kw = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, step=1)
    for bad in (torch.zeros(8, dtype=torch.float64, device=_dev()), torch.zeros(8, dtype=torch.bfloat16, device=_dev()),
                torch.zeros(16, device=_dev())[::2], torch.zeros(4, 4, device=_dev()).t(), torch.zeros(8)):
        with pytest.raises(ValueError):
            ops.grad_norm([good[0], bad])
        for slot in range(4):
            lists = [[t] for t in good]
            lists[slot] = [bad]
            with pytest.raises(ValueError):
                ops.adam_step(*lists, **kw)
    with pytest.raises(ValueError):
        ops.adam_step([good[0]], [torch.zeros(9, device=_dev())], [good[2]], [good[3]], **kw)      # sizes differ
    with pytest.raises(ValueError):
        ops.adam_step(*[[t] for t in good], max_norm=5.0, **kw)                                    # clip without a norm
    assert all(not t.any() for t in good)


# ---- twenty steps ------------------------------------------------------------------------------------------------------
TWENTY_SHAPES = [(1,), (3,), (1023,), (1025,), (10, 2, 130, 64), (403, 10)]


def _twenty_gradients():
    rng = np.random.default_rng(800)
    steps = []
    for s in range(20):
        grads = [((2.0 if s % 2 else 2e-3) * rng.standard_normal(sh)).astype(np.float32) for sh in TWENTY_SHAPES]
        grads[4][3:7] = 0.0                       # a block nothing flows into (an unused head)
        grads[4][:, 1][rng.random((10, 130, 64)) < 0.5] = 0.0
        steps.append(grads)
    return steps


def _run_clipadam(params, steps, **kw):
    from multistgraph_amd.optim import ClipAdam
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(_dev())) for p in params]
    opt = ClipAdam(ps, **kw)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, [5, 10], 0.75)
    norms = []
    for grads in steps:
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(_dev())
        opt.step()
        sched.step()
        norms.append(opt.last_grad_norm)
    got = {k: [opt.state[p][k].cpu().numpy() for p in ps] for k in R.KINDS[1:]}
    got["param"] = [p.detach().cpu().numpy() for p in ps]
    return got, [float(n.item()) for n in norms], opt


def test_twenty_steps(lib_built):
    params, _ = R.make_set(TWENTY_SHAPES, 801)
    steps = _twenty_gradients()
    ref64, G = R.reference(params, steps, max_norm=5.0, milestones=[5, 10], gamma=0.75, **R.HP)
    clipped = sum(n > 5.0 for n in ref64["norms"])
    print("20 steps: %d clipped, largest |param| %.2f" % (clipped, max(float(np.abs(p).max()) for p in ref64["param"])))
    assert 0 < clipped < 20
    got, norms, opt = _run_clipadam(params, steps, max_grad_norm=5, **R.HP)
    assert opt.param_groups[0]["lr"] == pytest.approx(R.HP["lr"] * 0.75 ** 2, rel=1e-12)
    _check("20 steps", got, ref64, G)
    for n, grads in zip(norms, steps):
        assert abs(n - R.norm64(grads)) <= float(np.spacing(np.float32(R.norm64(grads))))
    again, norms2, _ = _run_clipadam(params, steps, max_grad_norm=5, **R.HP)
    assert norms2 == norms
    for kind in R.KINDS:
        for a, b in zip(got[kind], again[kind]):
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), kind


# ---- state dict --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["clipadam", "torch"])
def test_state_dict_exchange(first, lib_built):
    """five steps of one optimizer, its state_dict() into the other, five more: the ten steps of the float64 reference"""
    from multistgraph_amd.optim import ClipAdam
    shapes = [(1025,), (3,), (40, 33)]
    params, _ = R.make_set(shapes, 900)
    rng = np.random.default_rng(901)
    steps = [[((30.0 if s % 3 == 0 else 0.05) * rng.standard_normal(sh)).astype(np.float32) for sh in shapes]
             for s in range(10)]
    ref64, G = R.reference(params, steps, max_norm=5.0, **R.HP)
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(_dev())) for p in params]
    make = dict(clipadam=lambda: ClipAdam(ps, max_grad_norm=5, **R.HP), torch=lambda: torch.optim.Adam(ps, **R.HP))
    order = [first, "torch" if first == "clipadam" else "clipadam"]
    opt = make[order[0]]()
    for s, grads in enumerate(steps):
        if s == 5:
            nxt = make[order[1]]()
            nxt.load_state_dict(opt.state_dict())
            opt = nxt
        for p, g in zip(ps, grads):
            p.grad = torch.from_numpy(g).to(_dev())
        if isinstance(opt, torch.optim.Adam):
            torch.nn.utils.clip_grad_norm_(ps, 5.0)
        opt.step()
    assert [float(opt.state[p]["step"]) for p in ps] == [10.0] * 3
    got = {k: [opt.state[p][k].cpu().numpy() for p in ps] for k in R.KINDS[1:]}
    got["param"] = [p.detach().cpu().numpy() for p in ps]
    _check("state dict, %s first" % first, got, ref64, G)


# ---- through the model -------------------------------------------------------------------------------------------------
def _model(c):
    from multistgraph_amd.model import MultiATGCN
    m = MultiATGCN(dict(c.config("cuda:0"), hip_dropout="device", hip_deterministic=True), c.data_feature).to(_dev())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    return m


def _train(c, batch, fused, steps=5):
    from multistgraph_amd.optim import ClipAdam
    torch.manual_seed(77)           # the device dropout draws from (torch.initial_seed(), the model's own counter)
    m = _model(c)
    m.train()
    opt = ClipAdam(m.parameters(), max_grad_norm=5) if fused else torch.optim.Adam(m.parameters())
    recorded = []
    for _ in range(steps):
        opt.zero_grad()
        m.calculate_loss(batch).backward()
        recorded.append([None if p.grad is None else p.grad.detach().cpu().numpy().copy() for p in m.parameters()])
        if not fused:
            torch.nn.utils.clip_grad_norm_(m.parameters(), 5)
        opt.step()
    return m, recorded


@pytest.fixture(scope="module")
def trained(lib_built):
    c = Case("tiny_multi_uni_c2")
    batch = {"X": torch.from_numpy(c.x).to(_dev()), "y": torch.from_numpy(c.y).to(_dev())}
    start = [p.detach().cpu().numpy().copy() for p in _model(c).parameters()]
    (a, rec), (b, _), (t, _) = _train(c, batch, True), _train(c, batch, True), _train(c, batch, False)
    return c, batch, start, rec, a, b, t


def test_model_training_is_bit_reproducible(trained):
    c, batch, start, rec, a, b, t = trained
    moved = 0
    for (k, pa), pb, s in zip(a.named_parameters(), b.parameters(), start):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), k
        moved += int(not np.array_equal(pa.detach().cpu().numpy(), s))
    assert moved > 10


def test_model_training_against_torch_adam(trained):
    c, batch, start, rec, a, b, t = trained
    ref64, G = R.reference(start, rec, lr=1e-3, max_norm=5.0)
    print("through the model: G param %.3e; clipped steps %d of %d" % (G["param"], sum(n > 5 for n in ref64["norms"]),
                                                                      len(rec)))
    assert G["param"] > 0
    worst = 0.0
    for (k, pa), pt in zip(a.named_parameters(), t.parameters()):
        worst = max(worst, float((pa.detach().double() - pt.detach().double()).abs().max()))
    print("ClipAdam against clip_grad_norm_ + torch.optim.Adam on the GPU: largest gap %.3e = %.3f x 2G"
          % (worst, worst / (2 * G["param"])))
    assert worst <= 2 * G["param"]


def test_next_forward_sees_the_updated_parameters(trained):
    """the kernels write the parameters behind torch's back: without the version bump MultiATGCN would keep running on
    the `prepared` of the parameters before the step"""
    c, batch, start, rec, a, b, t = trained
    a.eval()
    with torch.no_grad():
        got = a.predict(batch).clone()
    fresh = _model(c)
    fresh.load_state_dict(a.state_dict())
    fresh.eval()
    with torch.no_grad():
        want = fresh.predict(batch)
    assert torch.isfinite(got).all() and torch.equal(got.view(torch.int32), want.view(torch.int32))
