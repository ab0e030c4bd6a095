"""Device-side dropout on the GPU: the mask a descriptor stands for, the seeded training pair against the explicit-mask
pair, the Monte-Carlo-dropout forward, and the model surface (config['hip_dropout'], predict_mc).

Every seeded result is compared with what the library gives on the mask tensor matgcn_dropout_mask writes for the same
descriptor - and that tensor with the numpy generator of philox_ref.py, bit for bit.  Tolerances: torch.equal wherever the
contract is "the same bits"; 1e-4 max-normalised per gradient tensor under the default atomics (the project's gradient
tolerance); 1e-6 max-normalised for the MC samples, their mean and the p = 0 forward (the forward's parity bound); 1e-5 of
the largest standard deviation for std (Welford in fp32: of order S * 2^-24 with headroom).
"""
import numpy as np
import pytest
import torch

import philox_ref as R
from helpers import Case, max_norm_err

pytestmark = pytest.mark.gpu

SEED, P = 1234, 0.1
GRAD_TOL = 1e-4
FWD_TOL = 1e-6
STD_TOL = 1e-5
OUT = 6


class _Bound:
    """a synthetic model of `nodes` nodes bound to the HIP path at batch size `batch` (closed-form parameters, synthetic
    inputs, the host graph prep's static supports - as the shape-edge fixtures are built); rnn_units < 64 goes through
    the plugin class, which pads it to the kernels' 64 channels"""

    def __init__(self, nodes, batch, **flags):
        from multistgraph_amd import graph_prep, synthetic as syn
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        flags = dict(flags)
        self.out = out = flags.pop("out", OUT)          # output_window
        self.od = od = flags.pop("end_dim", 1)          # flow channels: out_channels = out * od
        self.n, self.b, self.flags = nodes, batch, flags
        self.dev = dev = torch.device("cuda:0")
        seed = 3
        df = dict(syn.make_data_feature(nodes, seed, "DC", ext_dim=1), output_dim=od, feature_dim=od + 1)
        cfg = dict(input_window=24, output_window=out, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
                   adjtype="multi", adpadj="unidirection", cheb_order=2, embed_dim_node=20, embed_dim_adj=20, rnn_units=64,
                   num_layers=2, device=dev, batch_size=batch, start_dim=0, end_dim=od)
        cfg.update(flags)
        shapes = syn.param_shapes(nodes, out_steps=out, feat_in=od + 1, out_dim=od,
                                  k_total=syn.k_total_for("multi", "unidirection", 2), **flags)
        state = syn.closed_form_state(shapes, seed)
        x, _ = syn.make_batch_arrays(batch, nodes, out, seed, feat=od + 1)
        if od > 1:   # channels [flow 0 .. flow od-1 | time of day]
            x = np.ascontiguousarray(np.concatenate([x[..., :1], x[..., 2:], x[..., 1:2]], -1))
        self.x = torch.from_numpy(x).to(dev)
        self.head_steps = 1 if flags.get("fnn_off") else 24
        if flags.get("rnn_units", 64) < 64:
            from multistgraph_amd.model import MultiATGCN
            self.model = MultiATGCN(cfg, df).to(dev)
            self.model.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
            with torch.no_grad():
                self.hp = self.model._path_for_batch(batch, dev)
                self.state = {k: v for k, v in self.model._state().items() if not k.startswith("static_initial")}
        else:
            mats = torch.from_numpy(np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None,
                                                                              "multi"), 0))
            spec = spec_from_config(cfg, df, nodes, min(nodes, 20), mats.shape[0], diagonal_mask(mats))
            self.hp = HotPath(spec, batch, dev)
            self.state = {k: torch.from_numpy(v).to(dev) for k, v in state.items()}
            self.hp.bind(self.state, mats.to(dev))

    def series_source(self):
        """the same kind of batch as label starts into a device-resident series"""
        from multistgraph_amd import windows as W
        rel = W.window_offsets(24)
        steps = 24 * 28 + 24 * 2 + 7
        rng = np.random.default_rng(5)
        series = rng.standard_normal((steps, self.n, 2)).astype(np.float32)
        starts = W.valid_label_starts(steps, rel, 24)
        pick = starts[rng.permutation(len(starts))[:self.b]].astype(np.int32)
        return (torch.from_numpy(series).to(self.dev), torch.from_numpy(pick).to(self.dev), rel)

    def d_out(self):
        g = np.random.default_rng(9).standard_normal((self.b, self.out, self.n, self.od)).astype(np.float32)
        return torch.from_numpy(g).to(self.dev)

    def h0(self):
        s = self.hp.spec
        g = np.random.default_rng(11).standard_normal((s.layers, self.b, s.nodes, s.hidden)).astype(np.float32)
        return torch.from_numpy(0.1 * g).to(self.dev)


@pytest.fixture(scope="module")
def bound(lib_built):
    cache = {}

    def get(nodes, batch, **flags):
        key = (nodes, batch, tuple(sorted(flags.items())))
        if key not in cache:
            cache[key] = _Bound(nodes, batch, **flags)
        return cache[key]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- 1. the mask -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nodes,batch,flags", [(65, 16, {}), (48, 3, {}), (21, 129, {"fnn_off": True})])
def test_exported_mask_equals_the_numpy_generator(nodes, batch, flags, bound):
    p = bound(nodes, batch, **flags)
    for offset in (0, 2 ** 32 + 5):
        for prob in (0.1, 0.5):
            got = p.hp.dropout_mask(SEED, offset, prob).cpu().numpy()
            want = R.mask(batch, p.head_steps, nodes, SEED, offset, prob)
            assert got.shape == want.shape
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (offset, prob)
    ones = p.hp.dropout_mask(SEED, 7, 0.0)
    assert torch.equal(ones, torch.ones_like(ones))


# ---- 2. the training forward -------------------------------------------------------------------------------------------
def _forward_pair(p, x, offset=0, h0=None):
    """(out, train buffer) of the explicit-mask forward_train and of the seeded one, each into a train buffer whose every
    byte was 0xFF before - the whole buffer is compared, which holds the seqDrop region; and of a forward without dropout"""
    hp = p.hp
    mask = hp.dropout_mask(SEED, offset, P)
    hp.forward_train(x, mask, h0)            # sizes the buffers for the current settings
    res = []
    for kw in (dict(drop_mask=mask), dict(dropout=(SEED, offset, P)), dict()):
        hp._train.view(torch.uint8).fill_(0xFF)
        out = hp.forward_train(x, h0=h0, **kw).clone()
        res.append((out, _bits(hp._train).clone()))
    return res


FORWARD_CASES = {
    "n65_b16": (65, 16, {}),            # 32-row items, one node past a tile
    "n257_b33": (257, 33, {}),          # 64-row items
    "n21_b129": (21, 129, {}),          # three row blocks per node
    "pad32_n48_b3": (48, 3, {"rnn_units": 32}),
    "fnn_off": (21, 129, {"fnn_off": True}),
    "gcn_off": (48, 3, {"gcn_off": True}),   # k_apply_dropout
}


@pytest.mark.parametrize("name", sorted(FORWARD_CASES))
def test_seeded_forward_train_equals_the_explicit_mask(name, bound):
    nodes, batch, flags = FORWARD_CASES[name]
    p = bound(nodes, batch, **flags)
    (y_mask, tr_mask), (y_seed, tr_seed), (y_none, tr_none) = _forward_pair(p, p.x, offset=3)
    assert torch.isfinite(y_mask).all()
    assert torch.equal(_bits(y_seed), _bits(y_mask))
    assert torch.equal(tr_seed, tr_mask)
    assert not torch.equal(y_none, y_mask) and not torch.equal(tr_none, tr_mask)    # the dropout is in what was compared


def test_seeded_forward_train_from_the_series(bound):
    p = bound(65, 16)
    (y_mask, tr_mask), (y_seed, tr_seed), (y_none, _) = _forward_pair(p, p.series_source(), offset=2 ** 32 + 5)
    assert torch.equal(_bits(y_seed), _bits(y_mask)) and torch.equal(tr_seed, tr_mask)
    assert not torch.equal(y_none, y_mask)


@pytest.mark.parametrize("setting", ["train_precision_2", "train_bf16x3"])
def test_seeded_forward_train_under_the_precision_modes(setting, bound):
    p = bound(65, 16)
    hp = p.hp
    fp32 = hp.forward_train(p.x, dropout=(SEED, 1, P)).clone()
    try:
        if setting == "train_precision_2":
            hp.precision = 2
        else:
            hp.train_bf16x3 = True
        (y_mask, tr_mask), (y_seed, tr_seed), (y_none, _) = _forward_pair(p, p.x, offset=1)
    finally:
        hp.precision, hp.train_bf16x3 = None, None
    assert torch.equal(_bits(y_seed), _bits(y_mask)) and torch.equal(tr_seed, tr_mask)
    assert not torch.equal(y_none, y_mask)
    assert not torch.equal(y_seed, fp32)                 # the mode's kernels ran


# ---- 3. the backward ---------------------------------------------------------------------------------------------------
def _grad_pair(p, deterministic, offset=0, bwd_offset=None):
    """gradients (d_h0 included) of the explicit-mask pair and of the seeded pair"""
    hp = p.hp
    x, d_out, h0 = p.x, p.d_out(), p.h0()
    mask = hp.dropout_mask(SEED, offset, P)
    hp.deterministic = deterministic
    try:
        hp.forward_train(x, mask, h0)
        want = {k: v.clone() for k, v in hp.backward(x, d_out, p.state, mask, h0).items()}
        hp.forward_train(x, h0=h0, dropout=(SEED, offset, P))
        got = {k: v.clone() for k, v in hp.backward(x, d_out, p.state, h0=h0, dropout=(
            SEED, offset if bwd_offset is None else bwd_offset, P)).items()}
    finally:
        hp.deterministic = None
    assert hp.D_H0 in want and set(got) == set(want)
    return want, got


@pytest.mark.parametrize("nodes,batch", [(65, 16), (257, 33)])
def test_seeded_backward_has_the_bits_of_the_explicit_mask(nodes, batch, bound):
    want, got = _grad_pair(bound(nodes, batch), deterministic=True, offset=5)
    assert all(torch.isfinite(v).all() for v in want.values())
    assert float(want["end_conv.weight"].abs().max()) > 0 and float(want["node_emb"].abs().max()) > 0
    diff = [k for k in want if not torch.equal(_bits(got[k]), _bits(want[k]))]
    assert not diff, diff


def test_seeded_backward_with_the_default_atomics(bound):
    want, got = _grad_pair(bound(65, 16), deterministic=False, offset=5)
    for k in want:
        err = float((got[k] - want[k]).abs().max()) / (float(want[k].abs().max()) + 1e-30)
        print("%s: seeded vs explicit-mask backward %.2e" % (k, err))
        assert err <= GRAD_TOL, (k, err)


def test_a_backward_with_another_offset_differs(bound):
    """sanity, not a contract: the backward draws from the descriptor it is handed"""
    want, got = _grad_pair(bound(65, 16), deterministic=True, offset=5, bwd_offset=6)
    assert any(not torch.equal(got[k], want[k]) for k in want)


# ---- 4. Monte-Carlo dropout --------------------------------------------------------------------------------------------
# the last: out_channels = 24 * 2 = 48, the second 32-channel tile of k_head_mc (NTc 2) with two interleaved output channels
MC_CASES = [(65, 16, {}), (21, 129, {"fnn_off": True}), (65, 3, {"out": 24, "end_dim": 2})]


def _mc_reference(p, samples, offset):
    """matgcn_output_head(matgcn_encoder_fwd(...) * mask(seed, offset + s)) for every sample"""
    hp = p.hp
    seq, _ = hp.encoder(hp.fuse_heads(p.x))
    outs = []
    for s in range(samples):
        m = hp.dropout_mask(SEED, offset + s, P)
        dropped = seq.clone()
        dropped[:, -p.head_steps:] *= m
        outs.append(hp.output_head(dropped).clone())
    return torch.stack(outs, 0)


@pytest.mark.parametrize("nodes,batch,flags", MC_CASES)
def test_forward_mc_samples_mean_and_std(nodes, batch, flags, bound):
    p = bound(nodes, batch, **flags)
    S, offset = 8, 2 ** 32 + 5
    mean, std, samples = p.hp.forward_mc(p.x, seed=SEED, offset=offset, p=P, samples=S, keep_samples=True)
    want = _mc_reference(p, S, offset)
    assert samples.shape == want.shape == (S, batch, p.out, nodes, p.od)
    for s in range(S):
        err = max_norm_err(samples[s].cpu().numpy(), want[s].cpu().numpy())
        assert err <= FWD_TOL, (s, err)
    assert torch.equal(_bits(samples), _bits(want))     # k_head's reduction order is kept: the header promises the bits
    s64 = samples.cpu().numpy().astype(np.float64)
    e_mean = max_norm_err(mean.cpu().numpy(), s64.mean(0))
    sd64 = s64.std(0)                                    # population standard deviation
    e_std = float(np.abs(std.cpu().numpy() - sd64).max() / sd64.max())
    print("mean %.2e (bound %.0e), std %.2e of the largest std (bound %.0e)" % (e_mean, FWD_TOL, e_std, STD_TOL))
    assert e_mean <= FWD_TOL and e_std <= STD_TOL
    assert sd64.max() > 0
    # without keep_samples: the same mean and std
    mean2, std2 = p.hp.forward_mc(p.x, seed=SEED, offset=offset, p=P, samples=S)
    assert torch.equal(mean2, mean) and torch.equal(std2, std)


@pytest.mark.parametrize("nodes,batch,flags", MC_CASES)
def test_forward_mc_edges(nodes, batch, flags, bound):
    from multistgraph_amd import _lib
    p = bound(nodes, batch, **flags)
    hp = p.hp
    mean, std, samples = hp.forward_mc(p.x, seed=SEED, offset=4, p=P, samples=1, keep_samples=True)
    assert torch.equal(std, torch.zeros_like(std)) and torch.equal(_bits(mean), _bits(samples[0]))
    plain = hp.forward(p.x).clone()
    mean0, std0 = hp.forward_mc(p.x, seed=SEED, offset=4, p=0.0, samples=3)
    assert max_norm_err(mean0.cpu().numpy(), plain.cpu().numpy()) <= FWD_TOL
    assert float(std0.abs().max()) <= FWD_TOL * float(plain.abs().max())
    for bad in (0, 1025):
        with pytest.raises(_lib.MatgcnError) as err:
            hp.forward_mc(p.x, seed=SEED, p=P, samples=bad)
        assert "(status -2)" in str(err.value)          # MATGCN_ERR_BAD_ARG


def test_forward_mc_from_the_series_equals_the_windows(bound):
    from multistgraph_amd import windows as W
    p = bound(65, 16)
    series, pick, rel = p.series_source()
    x, _ = W.gather_windows(series.cpu().numpy(), pick.cpu().numpy(), rel, OUT)
    a = p.hp.forward_mc((series, pick, rel), seed=SEED, offset=1, p=P, samples=4)
    b = p.hp.forward_mc(torch.from_numpy(x).to(p.dev), seed=SEED, offset=1, p=P, samples=4)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 5. the model ------------------------------------------------------------------------------------------------------
def _model(c, **extra):
    from multistgraph_amd.model import MultiATGCN
    dev = torch.device("cuda:0")
    m = MultiATGCN(dict(c.config("cuda:0"), **extra), c.data_feature).to(dev)
    return m, dev


def _refuse_torch_dropout(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError("torch.nn.functional.dropout was called in device mode")
    monkeypatch.setattr(torch.nn.functional, "dropout", refuse)


def test_device_mode_trains_without_torch_dropout(lib_built, monkeypatch):
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_dropout="device")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    m.train()
    _refuse_torch_dropout(monkeypatch)
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}
    state = torch.cuda.get_rng_state(dev)
    loss = m.calculate_loss(batch)
    loss.backward()
    assert torch.isfinite(loss) and all(torch.isfinite(q.grad).all() for q in m.parameters() if q.grad is not None)
    assert float(m.end_conv.weight.grad.abs().max()) > 0
    assert torch.equal(torch.cuda.get_rng_state(dev), state)      # nothing was drawn from torch's generator
    assert m._dropout_counter == 1
    with torch.no_grad():
        m.eval()
        eval_loss = m.calculate_loss(batch)
    assert float(eval_loss) != float(loss.detach())                # the training forward did drop


def test_same_seed_same_steps(lib_built, monkeypatch):
    """two models built under the same torch.manual_seed: bit-identical losses and gradients (deterministic on) for two
    consecutive steps, and the second step's mask is not the first's"""
    c = Case("tiny_multi_uni_c2")
    _refuse_torch_dropout(monkeypatch)
    dev = torch.device("cuda:0")
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}

    def run():
        torch.manual_seed(77)
        m, _ = _model(c, hip_dropout="device", hip_deterministic=True)
        m.train()
        steps = []
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            loss = m.calculate_loss(batch)
            loss.backward()
            steps.append((loss.detach().clone(), {k: q.grad.clone() for k, q in m.named_parameters() if q.grad is not None}))
        return steps

    a, b = run(), run()
    for (la, ga), (lb, gb) in zip(a, b):
        assert torch.equal(la, lb) and set(ga) == set(gb)
        assert all(torch.equal(_bits(ga[k]), _bits(gb[k])) for k in ga)
    # no parameter moved between the steps: only the mask can make step 2 differ from step 1
    assert not torch.equal(a[0][0], a[1][0])


@pytest.mark.parametrize("training", [False, True])
def test_predict_mc(training, lib_built):
    from multistgraph_amd import windows as W
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_dropout="device")
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    m.train(training)
    batch = {"X": torch.from_numpy(c.x).to(dev)}
    mean, std = m.predict_mc(batch, samples=8, seed=5)
    mean2, std2, kept = m.predict_mc(batch, samples=8, seed=5, keep_samples=True)
    shape = (c.b, c.out, c.n, 1)
    assert tuple(mean.shape) == tuple(std.shape) == shape and tuple(kept.shape) == (8,) + shape
    assert torch.equal(mean, mean2) and torch.equal(std, std2)
    assert float(std.max()) > 0 and torch.isfinite(mean).all() and not mean.requires_grad
    assert m.training is training and m._dropout_counter == 0     # an explicit seed leaves the counter alone
    m.predict_mc(batch, samples=8)
    assert m._dropout_counter == 8
    # a resident-series batch
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, c.feat)).astype(np.float32)
    pick = W.valid_label_starts(steps, rel, 24)[:c.b].astype(np.int32)
    sb = {"series": torch.from_numpy(series).to(dev), "label_start": torch.from_numpy(pick).to(dev)}
    x, _ = W.gather_windows(series, pick, rel, c.out)
    ms, ss = m.predict_mc(sb, samples=4, seed=5)
    mw, sw = m.predict_mc({"X": torch.from_numpy(x).to(dev)}, samples=4, seed=5)
    assert torch.equal(ms, mw) and torch.equal(ss, sw)
    assert m.training is training


def test_predict_mc_invalidates_a_pending_backward(lib_built):
    c = Case("tiny_multi_uni_c2")
    m, dev = _model(c, hip_dropout="device")
    m.train()
    batch = {"X": torch.from_numpy(c.x).to(dev), "y": torch.from_numpy(c.y).to(dev)}
    loss = m.calculate_loss(batch)
    m.predict_mc(batch, samples=2, seed=1)
    with pytest.raises(RuntimeError, match="another forward ran"):
        loss.backward()
