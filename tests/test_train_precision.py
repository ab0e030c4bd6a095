"""bf16 training precision: matgcn_set_train_precision (include/matgcn.h) and the plugin's config['hip_precision'].

Mode 1 = bf16 operands for the graph mixes of matgcn_forward_train and the transposed graph mixes of matgcn_backward;
mode 2 = additionally the node-wise contractions of both (bf16 copies of the weights).  fp32 accumulation, fp32 state, activations,
parameters and gradients.  The modes compute different numbers with their own tolerance (GRAD_BF16_TOL, max-normalised
per tensor against the reference's autograd fixtures, set from measurement); the fp32 default stays bit-identical.
"""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN_DIR, Case, max_norm_err

# 2 x the worst tensor measured over FIXTURES in both modes (1.35e-2: tiny_multi_uni_c1, mode 2, weight_tsg;
# DESIGN.md section 5), below the cap of 3e-2
GRAD_BF16_TOL = 2.7e-2
LOSS_REL_TOL = 5e-3
PRED_BF16_TOL = 5e-3
ATOMIC_TOL = 2e-6      # two fp32 backward runs differ in the order of their atomic accumulations only
PREC = {1: "bf16_mix", 2: "bf16"}
FIXTURES = ["tiny_multi_uni_c2", "tiny_multi_uni_c1", "tiny_multi_uni_c2_static", "tiny_heads_331", "tiny_multi_uni_dyn7",
            "dc237_out12", "bm403_out24"]
D_H0 = "__d_h0__"


# ---- CPU -------------------------------------------------------------------------------------------------------------
def test_train_precision_setter(lib_built):
    """the setter exists, starts at 0, returns the previous value, maps invalid values to 0, is independent of the
    inference setting; matgcn_workspace_bytes / matgcn_train_bytes count the bf16 weight copies while mode 2 is set"""
    import ctypes as C
    from multistgraph_amd import _lib
    from multistgraph_amd.ops import spec_from_config
    assert "matgcn_set_train_precision" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert lib.matgcn_set_train_precision(0) == 0
    try:
        assert lib.matgcn_set_train_precision(2) == 0
        assert lib.matgcn_set_train_precision(1) == 2
        assert lib.matgcn_set_train_precision(7) == 1
        assert lib.matgcn_set_train_precision(-1) == 0      # 7 meant 0
        assert lib.matgcn_set_mix_precision(0) == 0         # the inference setting is untouched
        c = Case("tiny_multi_uni_c2")
        dims = spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), 0, 0).dims(c.b)
        ws, tr = C.c_size_t(), C.c_size_t()
        assert lib.matgcn_workspace_bytes(C.byref(dims), C.byref(ws)) == 0
        assert lib.matgcn_train_bytes(C.byref(dims), C.byref(tr)) == 0
        ws0, tr0 = ws.value, tr.value
        lib.matgcn_set_train_precision(2)
        assert lib.matgcn_workspace_bytes(C.byref(dims), C.byref(ws)) == 0
        assert lib.matgcn_train_bytes(C.byref(dims), C.byref(tr)) == 0
        assert ws.value > ws0 and tr.value > tr0
        lib.matgcn_set_train_precision(1)
        assert lib.matgcn_workspace_bytes(C.byref(dims), C.byref(ws)) == 0
        assert lib.matgcn_train_bytes(C.byref(dims), C.byref(tr)) == 0
        assert ws.value == ws0 and tr.value == tr0
    finally:
        lib.matgcn_set_train_precision(0)


@pytest.mark.parametrize("value", ["fp32", "bf16_mix", "bf16"])
def test_hip_precision_key(value):
    """config['hip_precision'] is accepted, kept as an attribute and leaves the checkpoint ABI alone"""
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    torch.manual_seed(0)
    ref = MultiATGCN(c.config(), c.data_feature)
    torch.manual_seed(0)
    m = MultiATGCN(dict(c.config(), hip_precision=value), c.data_feature)
    assert m.hip_precision == value
    assert ref.hip_precision == "fp32"
    sd, rd = m.state_dict(), ref.state_dict()
    assert list(sd) == list(rd)
    assert all(sd[k].shape == rd[k].shape and torch.equal(sd[k], rd[k]) for k in sd)


def test_hip_precision_rejects_unknown_values():
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    for bad in ("fp16", "bfloat16", 2, None):
        with pytest.raises(ValueError):
            MultiATGCN(dict(c.config(), hip_precision=bad), c.data_feature)


# ---- GPU -------------------------------------------------------------------------------------------------------------
def _path(c):
    from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
    dev = torch.device("cuda:0")
    use_static = c.adpadj == "none" or c.adjtype == "multi"
    st = torch.from_numpy(c.gold["static_supports"]).to(dev) if use_static else None
    spec = spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), st.shape[0] if use_static else 0,
                            diagonal_mask(st))
    hp = HotPath(spec, c.b, dev)
    state = {k: torch.from_numpy(v).to(dev) for k, v in c.state.items()}
    hp.bind(state, st)
    return hp, dev, state


def _fixture_mask(gold):
    shape = tuple(int(v) for v in gold["drop_shape"])
    bits = np.unpackbits(gold["drop_bits"])[:int(np.prod(shape))].reshape(shape)
    return (bits.astype(np.float32) / np.float32(0.9)).astype(np.float32)


def _errors(gold, grads):
    """max-normalised error of every gradient against the fixture (large tensors: the fixture's every-17th subsample)"""
    out = {}
    for k, g in grads.items():
        g = g.detach().cpu().numpy()
        w = gold["grad." + k] if "grad." + k in gold else gold["gsub." + k]
        got = g if "grad." + k in gold else g.reshape(-1)[::17]
        out[k] = 0.0 if np.abs(w).max() == 0.0 and np.abs(got).max() <= 1e-6 else max_norm_err(got, w)
    return out


def _step(hp, c, gold, dev, state, mode):
    """one HotPath training step (the fixture's dropout mask and d_out) in precision mode `mode` (None: fp32 default)"""
    hp.precision = mode
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    h0 = c.h0()
    h0 = None if h0 is None else h0.to(dev)
    y = hp.forward_train(x, mask, h0).clone()
    grads = hp.backward(x, torch.from_numpy(gold["d_out"]).to(dev), state, mask, h0)
    grads.pop(D_H0, None)
    return y, {k: v.clone() for k, v in grads.items()}


def _same_up_to_atomics(a, b):
    for k in a:
        scale = float(a[k].abs().max()) + 1e-30
        assert float((a[k] - b[k]).abs().max()) <= ATOMIC_TOL * scale, k


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", FIXTURES)
def test_bf16_training_step_vs_fixture(name, mode, lib_built):
    """forward_train + backward in mode 1 / 2 against the reference's autograd fixture; the variant really ran (the
    gradients differ from the fp32 path's), and the fp32 path afterwards is the fp32 path before it"""
    c = Case(name)
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_%s.npz" % name))
    hp, dev, state = _path(c)
    y32, g32 = _step(hp, c, gold, dev, state, None)
    yb, gb = _step(hp, c, gold, dev, state, mode)
    assert not torch.equal(yb, y32)                                  # the bf16 training forward ran
    assert max_norm_err(yb.cpu().numpy(), gold["pred"]) <= PRED_BF16_TOL
    errs = _errors(gold, gb)
    report = os.environ.get("MATGCN_PRECISION_REPORT")
    if report:
        import json
        with open(report, "a") as fh:
            fh.write(json.dumps({"case": name, "mode": mode, "pred": max_norm_err(yb.cpu().numpy(), gold["pred"]),
                                 "fp32": max(_errors(gold, g32).values()), "grads": errs}) + "\n")
    bad = {k: e for k, e in errs.items() if e > GRAD_BF16_TOL}
    assert not bad, bad
    assert any(not torch.equal(gb[k], g32[k]) for k in g32)
    y32b, g32b = _step(hp, c, gold, dev, state, None)
    assert torch.equal(y32b, y32)
    _same_up_to_atomics(g32, g32b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "bm403_out24"])
def test_plugin_bf16_training_step(name, mode, lib_built, monkeypatch):
    """calculate_loss(batch).backward() with hip_precision set: the loss against the reference's fixture, p.grad too on the
    tiny graph.  (At N = 403 the masked-MAE gradient sign(p - l) flips on the labels the bf16 prediction crosses, so the
    plugin's d_out itself differs from the fixture's: the gradients of the kernels are held to the fixture with its own
    d_out in test_bf16_training_step_vs_fixture instead.)"""
    from multistgraph_amd.model import MultiATGCN
    c = Case(name)
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_%s.npz" % name))
    dev = torch.device("cuda:0")
    model = MultiATGCN(dict(c.config("cuda:0"), hip_precision=PREC[mode]), c.data_feature).to(dev)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    model.train()
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda inp, p=0.5, training=True, inplace=False: inp * mask)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}
    loss = model.calculate_loss(batch)
    assert abs(float(loss.detach()) - float(gold["loss"])) <= LOSS_REL_TOL * abs(float(gold["loss"]))
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()}
    assert all(torch.isfinite(g).all() for g in grads.values())
    if c.n < 64:
        grads = {k: g for k, g in grads.items() if "grad." + k in gold or "gsub." + k in gold}
        bad = {k: e for k, e in _errors(gold, grads).items() if e > GRAD_BF16_TOL}
        assert not bad, bad
    from multistgraph_amd import _lib
    lib = _lib.load()
    assert lib.matgcn_set_train_precision(0) == 0 and lib.matgcn_set_mix_precision(0) == 0   # restored


@pytest.mark.gpu
def test_full_size_bf16_gradients(lib_built):
    """Baltimore 403 at the headline batch B = 64: mode-2 gradients against the fp32 path's"""
    from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
    c = Case("bm403_out24")
    dev = torch.device("cuda:0")
    st = torch.from_numpy(c.gold["static_supports"]).to(dev)
    spec = spec_from_config(dict(c.config(), batch_size=64), c.data_feature, c.n, 20, st.shape[0], diagonal_mask(st))
    hp = HotPath(spec, 64, dev)
    state = {k: torch.from_numpy(v).to(dev) for k, v in c.state.items()}
    hp.bind(state, st)
    rng = np.random.default_rng(5)
    x = np.tile(c.x, (16, 1, 1, 1))[:64].copy()
    x[..., 0] += 0.05 * rng.standard_normal(x.shape[:-1]).astype(np.float32)
    x = torch.from_numpy(x).to(dev)
    d_out = torch.from_numpy(rng.standard_normal((64, c.out, c.n, 1)).astype(np.float32)).to(dev)
    hp.forward_train(x)
    g32 = {k: v.clone() for k, v in hp.backward(x, d_out, state).items()}
    hp.precision = 2
    hp.forward_train(x)
    gb = hp.backward(x, d_out, state)
    errs = {k: max_norm_err(gb[k].cpu().numpy(), g32[k].cpu().numpy()) for k in g32 if float(g32[k].abs().max()) > 0}
    bad = {k: e for k, e in errs.items() if e > GRAD_BF16_TOL}
    assert not bad, bad
    assert any(e > 0 for e in errs.values())


@pytest.mark.gpu
@pytest.mark.parametrize("fwd_mode,bwd_setting", [(2, 0), (None, 2), (1, 2)])
def test_backward_follows_the_forward_mode(fwd_mode, bwd_setting, lib_built):
    """a switch of matgcn_set_train_precision between forward_train and backward never mixes modes: the backward runs in
    the forward's mode (include/matgcn.h, matgcn_set_train_precision)"""
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    hp, dev, state = _path(c)
    _, want = _step(hp, c, gold, dev, state, fwd_mode)       # forward and backward in one mode
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    hp.precision = fwd_mode
    hp.forward_train(x, mask)
    hp.precision = bwd_setting                               # the setting in force for the backward
    with hp._mode(hp.lib.matgcn_set_train_precision):
        got = hp.backward(x, torch.from_numpy(gold["d_out"]).to(dev), state, mask)
    got.pop(D_H0, None)
    _same_up_to_atomics(want, got)


def _backward_on_copy(hp, x, d_out, state, mask, setting):
    """the saved activations of the last forward_train back-propagated with the kernels of mode `setting`: a second train
    buffer is recorded for that mode by a forward_train of its own, then gets the first buffer's contents (and the
    workspace the first forward left) - the layout of both buffers' common prefix is the same in every mode, and the mode-2
    tails are parameter-only copies - before matgcn_backward runs on it"""
    tr, ws, prec = hp._train, hp.workspace, hp.precision
    tr_saved, ws_saved = tr.clone(), ws.clone()
    try:
        hp._train = torch.empty_like(tr)
        hp.precision = setting
        hp.forward_train(x, mask)                     # records `setting` for the new buffer
        hp._train[:tr_saved.numel()].copy_(tr_saved)
        hp.workspace[:ws_saved.numel()].copy_(ws_saved)
        g = hp.backward(x, d_out, state, mask)
        return {k: v.clone() for k, v in g.items() if k != D_H0}
    finally:
        hp._train, hp.workspace, hp.precision = tr, ws, prec
        hp.workspace.copy_(ws_saved)


@pytest.mark.gpu
def test_bf16_backward_kernels_run(lib_built):
    """the backward's own bf16 kernels run: on the saved activations of ONE forward_train, the mode-1 backward differs from
    the fp32 backward (bf16 transposed mixes) and the mode-2 backward from the mode-1 backward (bf16 node contractions) by
    far more than the order of the fp32 atomics - and a repeat of the same backward agrees to that order"""
    c = Case("tiny_multi_uni_c2")
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_tiny_multi_uni_c2.npz"))
    hp, dev, state = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    d_out = torch.from_numpy(gold["d_out"]).to(dev)

    def gap(a, b):
        return max(float((a[k] - b[k]).abs().max()) / (float(a[k].abs().max()) + 1e-30) for k in a)

    for mode, other in ((1, 0), (2, 1)):
        hp.precision = mode
        hp.forward_train(x, mask)
        got = {k: v.clone() for k, v in hp.backward(x, d_out, state, mask).items() if k != D_H0}
        again = _backward_on_copy(hp, x, d_out, state, mask, mode)
        alt = _backward_on_copy(hp, x, d_out, state, mask, other)
        assert gap(got, again) <= ATOMIC_TOL, mode
        assert gap(got, alt) >= 100 * ATOMIC_TOL, (mode, gap(got, alt))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_plugin_inference_precision(mode, lib_built):
    """predict() with hip_precision = bf16_mix / bf16 is HotPath.forward under matgcn_set_mix_precision(1 / 2), bit for
    bit; a default model used in between in the same process stays bit-identical fp32"""
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    dev = torch.device("cuda:0")
    hp, _, _ = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    exact = hp.forward(x).clone()
    prev = hp.lib.matgcn_set_mix_precision(mode)
    try:
        want = hp.forward(x).clone()
    finally:
        hp.lib.matgcn_set_mix_precision(prev)
    models = {}
    for p in (PREC[mode], "fp32"):
        m = MultiATGCN(dict(c.config("cuda:0"), hip_precision=p), c.data_feature).to(dev).eval()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
        models[p] = m
    with torch.no_grad():
        got = models[PREC[mode]].predict({"X": x}).clone()
        plain = models["fp32"].predict({"X": x}).clone()
        again = models[PREC[mode]].predict({"X": x}).clone()
    assert torch.equal(got, want) and torch.equal(again, want)
    assert not torch.equal(got, exact)
    assert torch.equal(plain, exact)
    models[PREC[mode]].hip_precision = "fp32"                # evaluate in fp32 after training in bf16
    with torch.no_grad():
        assert torch.equal(models[PREC[mode]].predict({"X": x}), exact)


CONV_RUNS = 5
CONV_BAND = (0.75, 1.05)   # median mode-2 final loss / fp32 final loss; DESIGN.md section 5 (measured spread)


@pytest.mark.gpu
def test_bf16_training_converges(lib_built, monkeypatch):
    """40 Adam steps (lr 3e-3) from the same start, fp32 once (its final loss repeats to 5 digits) and mode 2 CONV_RUNS
    times (its runs vary: the fp32 atomics' last-bit differences cross bf16 rounding boundaries): every mode-2 run
    decreases the loss, and the median of their final losses lies within CONV_BAND of the fp32 final loss - at most the
    issue's 5 % above it; below it by no more than the measured spread allows (medians of two sessions 0.894 / 0.847,
    lowest single run 0.811 x fp32)"""
    import statistics
    from multistgraph_amd.model import MultiATGCN
    c = Case("tiny_multi_uni_c2")
    dev = torch.device("cuda:0")
    monkeypatch.setattr(torch.nn.functional, "dropout", lambda inp, p=0.5, training=True, inplace=False: inp)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}

    def run(p):
        model = MultiATGCN(dict(c.config("cuda:0"), hip_precision=p), c.data_feature).to(dev)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
        model.train()
        opt = torch.optim.Adam(model.parameters(), lr=3e-3)
        losses = []
        for _ in range(40):
            opt.zero_grad()
            loss = model.calculate_loss(batch)
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        return losses

    fp = run("fp32")
    finals = []
    for _ in range(CONV_RUNS):
        bf = run("bf16")
        assert bf[-1] < bf[0]
        finals.append(bf[-1])
    ratio = statistics.median(finals) / fp[-1]
    assert CONV_BAND[0] <= ratio <= CONV_BAND[1], (finals, fp[-1])
