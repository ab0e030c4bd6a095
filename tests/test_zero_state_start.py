"""Step 0 of an inference forward without h0 starts from the all-zero state: the library skips that step's two graph
mixes and runs the zero-state instantiations of the node kernels.  An explicit h0 - even an
all-zero tensor - takes the general path, so the two forwards of the same inputs are each other's reference.

Compared with numpy.array_equal: value equality, no tolerance (a signed zero does not fail it)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import FULL, GOLDEN_DIR, HID, TINY, Case

pytestmark = pytest.mark.gpu


def _path(c, batch=None, cfg_over=None, state=None):
    from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
    dev = torch.device("cuda:0")
    b = c.b if batch is None else batch
    use_static = c.adpadj == "none" or c.adjtype == "multi"
    st = torch.from_numpy(c.gold["static_supports"]).to(dev) if use_static else None
    cfg = dict(c.config(), batch_size=b, **(cfg_over or {}))
    spec = spec_from_config(cfg, c.data_feature, c.n, min(c.n, 20), st.shape[0] if use_static else 0, diagonal_mask(st))
    hp = HotPath(spec, b, dev)
    tensors = {k: torch.from_numpy(v).to(dev) for k, v in (c.state if state is None else state).items()}
    hp.bind(tensors, st)
    return hp, dev, tensors


def _zeros(hp):
    s = hp.spec
    return torch.zeros(s.layers, hp.batch, s.nodes, s.hidden, dtype=torch.float32, device=hp.device)


def _both(run, hp):
    """run(h0) without h0 (zero-state start) and with an explicit all-zero h0 (general path)"""
    new = run(None).cpu().numpy()
    ref = run(_zeros(hp)).cpu().numpy()
    assert np.isfinite(ref).all()
    assert np.array_equal(new, ref)
    return new


def _inputs(c, batch, seed=77):
    from multistgraph_amd import synthetic as syn
    if batch is None or batch == c.b:
        return c.x
    return syn.make_batch_arrays(batch, c.n, c.out, seed, feat=c.feat, x_steps=24 * sum(c.lens))[0]


def _step_mix_launches(hp, run):
    """k_mix<1> launches of one call, counted by the library's own per-launch profile"""
    from multistgraph_amd import _lib
    cap = 4096
    _lib.check(hp.lib.matgcn_profile_enable(1, cap), "matgcn_profile_enable")
    try:
        run()
        torch.cuda.synchronize()
        ms, kinds, cnt = (C.c_float * cap)(), (C.c_int * cap)(), C.c_int()
        _lib.check(hp.lib.matgcn_profile_collect(ms, kinds, cap, C.byref(cnt)), "matgcn_profile_collect")
    finally:
        hp.lib.matgcn_profile_disable()
    return cnt.value


# every adjacency mode, cheb_order 1 / 2 / 3, static features, the ablations (gcn_off among them), N = 237 and 403
@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("name", TINY + FULL)
def test_forward_without_h0_equals_forward_from_explicit_zeros(name, wavefront, lib_built):
    c = Case(name)
    hp, dev, _ = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    prev = hp.lib.matgcn_set_wavefront(wavefront)
    try:
        _both(lambda h0: hp.forward(x, h0), hp)
    finally:
        hp.lib.matgcn_set_wavefront(prev)


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("batch", [16, 64])
@pytest.mark.parametrize("name", ["dc237_out12", "bm403_out24"])
def test_headline_graphs_at_both_batch_sizes_and_every_precision_mode(name, batch, mode, wavefront, lib_built):
    """N = 237 runs 32-row work items at any batch size, N = 403 at B = 16 only; mode 2 runs the bf16 node kernels"""
    c = Case(name)
    hp, dev, _ = _path(c, batch)
    x = torch.from_numpy(_inputs(c, batch)).to(dev)
    prev_w = hp.lib.matgcn_set_wavefront(wavefront)
    prev_m = hp.lib.matgcn_set_mix_precision(mode)
    try:
        _both(lambda h0: hp.forward(x, h0), hp)
    finally:
        hp.lib.matgcn_set_mix_precision(prev_m)
        hp.lib.matgcn_set_wavefront(prev_w)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "tiny_od_non_c3", "tiny_multi_uni_c1", "tiny_multi_uni_c2_static",
                                  "tiny_multi_uni_dyn7", "abl_gcnoff"])
def test_bf16_modes_on_small_cases(name, mode, lib_built):
    c = Case(name)
    hp, dev, _ = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    prev = hp.lib.matgcn_set_mix_precision(mode)
    try:
        _both(lambda h0: hp.forward(x, h0), hp)
    finally:
        hp.lib.matgcn_set_mix_precision(prev)


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("batch", [3, 40])
def test_one_and_three_layers(layers, batch, wavefront, lib_built):
    """the golden cases all have two layers: the closed-form state of the same model at 1 and 3 layers (as
    test_backward_on_synthetic_shapes_outside_the_golden_set builds it), B = 40 for 64-row work items with padding rows"""
    from multistgraph_amd import synthetic as syn
    c = Case("tiny_multi_uni_c2")
    shapes = syn.param_shapes(c.n, out_steps=c.out, feat_in=c.feat, k_total=c.k_total, layers=layers, len_ts=sum(c.lens))
    state = syn.closed_form_state(shapes, 3)
    hp, dev, _ = _path(c, batch, {"num_layers": layers}, state)
    assert hp.spec.layers == layers
    x = torch.from_numpy(_inputs(c, batch)).to(dev)
    prev = hp.lib.matgcn_set_wavefront(wavefront)
    try:
        _both(lambda h0: hp.forward(x, h0), hp)
    finally:
        hp.lib.matgcn_set_wavefront(prev)


@pytest.mark.parametrize("name", HID)
def test_rnn_units_below_64_through_the_plugin_class(name, lib_built):
    """rnn_units < 64 exists behind the plugin class only (hidden_pad.py): its binding, with and without a zero h0"""
    from multistgraph_amd.model import MultiATGCN
    c = Case(name)
    dev = torch.device("cuda:0")
    m = MultiATGCN(c.config("cuda:0"), c.data_feature).to(dev).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    x = torch.from_numpy(c.x).to(dev)
    with torch.no_grad():
        hp = m._path_for(x)
        _both(lambda h0: hp.forward(x, h0), hp)


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("name", ["tiny_multi_uni_out12", "tiny_multi_uni_c2", "tiny_od_non_c3", "abl_gcnoff"])
def test_forward_series(name, wavefront, lib_built):
    from multistgraph_amd import windows as W
    c = Case(name)
    hp, dev, _ = _path(c)
    rel = W.window_offsets(24)
    steps = 24 * 28 + 24 * 2 + 7
    rng = np.random.default_rng(5)
    series = rng.standard_normal((steps, c.n, c.feat)).astype(np.float32)
    starts = W.valid_label_starts(steps, rel, 24)
    pick = starts[rng.permutation(len(starts))[:c.b]].astype(np.int32)
    sd, pd = torch.from_numpy(series).to(dev), torch.from_numpy(pick).to(dev)
    prev = hp.lib.matgcn_set_wavefront(wavefront)
    try:
        got = _both(lambda h0: hp.forward_series(sd, pd, rel, h0), hp)
        x, _ = W.gather_windows(series, pick, rel, c.out)
        assert np.array_equal(got, hp.forward(torch.from_numpy(x).to(dev)).cpu().numpy())
    finally:
        hp.lib.matgcn_set_wavefront(prev)


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("name", ["tiny_multi_uni_c2", "tiny_od_non_c3", "tiny_multi_bid_c1", "tiny_multi_uni_dyn7",
                                  "abl_gcnoff", "dc237_out12"])
def test_encoder_sequence_and_final_states(name, wavefront, lib_built):
    """matgcn_encoder_fwd takes the zero-state start when its h0 is null: the sequence and the (L, B, N, H) final states"""
    c = Case(name)
    hp, dev, _ = _path(c)
    x0 = torch.from_numpy(c.gold["x0"]).to(dev)
    prev = hp.lib.matgcn_set_wavefront(wavefront)
    try:
        seq_a, fin_a = (t.cpu().numpy() for t in hp.encoder(x0))
        seq_b, fin_b = (t.cpu().numpy() for t in hp.encoder(x0, _zeros(hp)))
    finally:
        hp.lib.matgcn_set_wavefront(prev)
    assert fin_a.shape == (2, c.b, c.n, 64)
    assert np.array_equal(seq_a, seq_b)
    assert np.array_equal(fin_a, fin_b)


@pytest.mark.parametrize("wavefront", [1, 0])
@pytest.mark.parametrize("name,layers", [("tiny_multi_uni_c2", 2), ("tiny_od_non_c3", 2), ("bm403_out24", 2),
                                         ("abl_gcnoff", 2)])
def test_the_step_mixes_of_step_0_are_not_launched(name, layers, wavefront, lib_built):
    """2 L T - 2 L launches of k_mix<1> without h0, 2 L T with one (none at all in the gcn_off ablation)"""
    c = Case(name)
    hp, dev, _ = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    z = _zeros(hp)
    hp.forward(x)
    prev = hp.lib.matgcn_set_wavefront(wavefront)
    try:
        general = _step_mix_launches(hp, lambda: hp.forward(x, z))
        zero = _step_mix_launches(hp, lambda: hp.forward(x))
    finally:
        hp.lib.matgcn_set_wavefront(prev)
    if c.flags.get("gcn_off"):
        assert general == 0 and zero == 0
    else:
        assert general == 2 * layers * 24
        assert zero == general - 2 * layers


GRAD_CASES = sorted(f[5:-4] for f in os.listdir(GOLDEN_DIR) if f.startswith("grad_") and not f.startswith("grad_hid"))


def _fixture_mask(gold):
    shape = tuple(int(v) for v in gold["drop_shape"])
    bits = np.unpackbits(gold["drop_bits"])[:int(np.prod(shape))].reshape(shape)
    return (bits.astype(np.float32) / np.float32(0.9)).astype(np.float32)


@pytest.mark.parametrize("name", GRAD_CASES)
def test_training_step_after_an_inference_forward_matches_the_gradient_fixtures(name, lib_built):
    """training keeps the general step 0 (the backward reads what it saves): a training forward + backward that follows
    an inference forward on the same binding still meets the reference's own prediction and gradients (tolerance of
    test_backward_gpu.py: 1e-4 max-normalised per tensor, 2e-4 on the sums of the subsampled ones)"""
    from helpers import max_norm_err
    c = Case(name)
    gold = np.load(os.path.join(GOLDEN_DIR, "grad_%s.npz" % name))
    hp, dev, state = _path(c)
    x = torch.from_numpy(c.x).to(dev)
    mask = torch.from_numpy(_fixture_mask(gold)).to(dev)
    h0 = c.h0()
    h0 = None if h0 is None else h0.to(dev)
    inference = hp.forward(x, h0)
    y = hp.forward_train(x, mask, h0)
    assert max_norm_err(y.cpu().numpy(), gold["pred"]) <= 1e-4
    assert torch.equal(hp.forward_train(x, None, h0), inference)      # without dropout: the same forward
    hp.forward_train(x, mask, h0)
    grads = hp.backward(x, torch.from_numpy(gold["d_out"]).to(dev), state, mask, h0)
    grads.pop(hp.D_H0, None)          # static-feature cases: the host-side layers behind d_h0 are test_backward_gpu.py's
    bad = {}
    for k, g in grads.items():
        g = g.detach().cpu().numpy()
        if "grad." + k in gold:
            got, w = g, gold["grad." + k]
        else:   # large tensors: every 17th element + [sum, sum |.|]
            got, w = g.reshape(-1)[::17], gold["gsub." + k]
            sums = gold["gsum." + k]
            if abs(float(g.astype(np.float64).sum()) - sums[0]) > 2e-4 * max(sums[1], 1e-30):
                bad[k + " (sum)"] = float(g.astype(np.float64).sum()), float(sums[0])
        if np.abs(w).max() == 0.0:
            if float(np.abs(got).max()) > 1e-6:
                bad[k] = "expected zero"
        elif max_norm_err(got, w) > 1e-4:
            bad[k] = max_norm_err(got, w)
    assert not bad, bad
