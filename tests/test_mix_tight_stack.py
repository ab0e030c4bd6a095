"""The forward's fp32 64 x 64 graph mixes on the tightly stacked A operand.

k_mix (roles 0 and 1) reads a copy of the support stack whose column k*N + n holds S_k[n][.] - no padding between the
supports - and launches over Ks*N stacked rows; stacked row r is support r / N, node r % N (matgcn_capi.hip:launch_mix,
matgcn_kernels.hip:k_mix, k_stack_tight).  What can go wrong is index arithmetic, so the cases are the shapes where it
changes.

All of them run at B = 22.  The 64 x 64 kernels are launched for MORE than 16 column tiles only (matgcn_capi.hip:
mix_half_tiles; up to 16 the mixes take k_mix_c32, which keeps St and Ks*Np rows): the step mixes and the x-part
pre-passes have B column tiles, the layer-0 fold rup(B*24*2, 64) / 64 - 17 at B = 22, the smallest batch at which every
mix of a forward is a 64 x 64 one.  A batch of 4 or less, as first planned for these shapes, reaches none of the changed
code.  That the tight copy is really what a forward reads is itself a test here (test_forward_reads_the_tight_copy).

  every remainder class of the last K-tile,
  odd and even nK                              N = 17 20 21 24 25 29 32 33 45 48  (N mod 16 = 1 4 5 8 9 13 0 1 13 0; nK 2 2 2 2 2 2 2 3 3 3)
  a 64-row tile across two or three supports,
  a support boundary inside a float4 of A      N = 17 21 22 23 (Ks = 3: all 3 N rows in one or two tiles), N = 67
  Ks*N around a multiple of 64                 N = 64 (Ks = 1, 3), N = 43 (129 rows), N = 85 (255 rows)
  Ks = 1, 2, 3                                 od / none (1), multi / none (2: the similarity Laplacian is diagonal and
                                               folded away), multi / unidirection (3); od / none with cheb_order 3 also
                                               sends the Chebyshev products of matgcn_prepare through k_mix<0> on St
  the headline graph                           N = 403, Ks = 3 (1 209 rows in 19 tiles)

The FLUSH instantiation (N > 1 024) has its cases in the suite already - edge_n1039_* (nK = 65, odd) in
test_shape_edges.py and synth4096_out24 (nK = 256, even) in test_hip_parity.py - so none is added here.

Truth is the CPU oracle in float64 (hoisted order), computed once per case.  Tolerances are the suite's own: 1e-4
max-normalised and element-wise for a forward (test_hip_parity.py, test_shape_edges.py), 2e-5 for a single cell
(test_hip_parity.py STAGE_TOL), 1e-4 per gradient tensor (__graft_entry__.smoke, test_backward_gpu.py).
"""
import numpy as np
import pytest
import torch

from helpers import Case, elementwise_excess, max_norm_err

pytestmark = pytest.mark.gpu

E2E_TOL = 1e-4
STAGE_TOL = 2e-5
GRAD_TOL = 1e-4

MODES = {1: ("od", "none", 2), 2: ("multi", "none", 2), 3: ("multi", "unidirection", 2), "cheb3": ("od", "none", 3)}
KS = {1: 1, 2: 2, 3: 3, "cheb3": 2}
SHAPES = [(n, 3) for n in (17, 20, 21, 22, 23, 24, 25, 29, 32, 33, 43, 45, 48, 64, 67, 85, 403)] + \
         [(21, 1), (64, 1), (21, 2), (23, 2), (21, "cheb3"), (29, "cheb3")]
IDS = ["n%d_ks%s" % s for s in SHAPES]
BATCH, OUT = 22, 3      # > 16 column tiles in every mix of a forward: see the module docstring


class _Synth:
    """a synthetic case of any size, built the way helpers.EdgeCase builds its own, bound to the HIP path; the float64
    oracle's parameters and supports beside it"""

    def __init__(self, n, mode):
        from multistgraph_amd import graph_prep, synthetic as syn
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        from oracle import matgcn_oracle as O
        self.n, self.mode = n, mode
        self.adjtype, self.adpadj, self.cheb = MODES[mode]
        seed = 100 + n
        df = syn.make_data_feature(n, seed, "BM" if n == 403 else "DC", ext_dim=1)
        self.mats = np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None, self.adjtype), 0)
        shapes = syn.param_shapes(n, out_steps=OUT, feat_in=2, k_total=syn.k_total_for(self.adjtype, self.adpadj, self.cheb))
        state = syn.closed_form_state(shapes, seed)
        x, _ = syn.make_batch_arrays(BATCH, n, OUT, seed, feat=2)
        cfg = dict(input_window=24, output_window=OUT, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
                   adjtype=self.adjtype, adpadj=self.adpadj, cheb_order=self.cheb, embed_dim_node=20, embed_dim_adj=20,
                   rnn_units=64, num_layers=2, device=torch.device("cpu"), batch_size=BATCH, start_dim=0, end_dim=1)
        self.ocfg = dict(adjtype=self.adjtype, adpadj=self.adpadj, cheb_order=self.cheb, num_layers=2, rnn_units=64,
                         len_closeness=48, len_period=24, len_trend=24, output_window=OUT, input_window=24,
                         add_time_in_day=True, add_day_in_week=False, load_dynamic=False, start_dim=0, end_dim=1)
        self.dev = torch.device("cuda:0")
        st = torch.from_numpy(self.mats)
        spec = spec_from_config(cfg, df, n, min(n, 20), st.shape[0], diagonal_mask(st))
        self.hp = HotPath(spec, BATCH, self.dev)
        self.hp.bind({k: torch.from_numpy(v).to(self.dev) for k, v in state.items()}, st.to(self.dev))
        self.x = torch.from_numpy(x).to(self.dev)
        self.p64 = O.to_tensors(state, torch.float64)
        self.st64 = O.supports_as_tensors(self.mats, torch.float64)
        self.want = O.forward(torch.from_numpy(x).double(), self.p64, self.st64, self.ocfg, faithful=False).numpy()


@pytest.fixture(scope="module")
def synth(lib_built):
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _Synth(*shape)
        return cache[shape]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_stack_has_the_dense_supports_the_case_is_about(shape, synth):
    """the mode really gives Ks = 1, 2, 3 (a folded or missing support would quietly test another shape), and the stack
    read back from `prepared` is the one the oracle mixes with"""
    from oracle import matgcn_oracle as O
    p = synth(shape)
    got = p.hp.supports().cpu().numpy()
    assert got.shape == (KS[shape[1]], p.n, p.n)
    stack = O.support_stack(p.p64, p.st64, p.adjtype, p.adpadj, p.cheb, None).numpy()[1:]
    dense = [s for s in stack if np.abs(s - np.diag(np.diagonal(s))).max() > 0]
    assert len(dense) == got.shape[0]
    assert max_norm_err(got, np.stack(dense, 0)) <= STAGE_TOL


def _stacks(p):
    """(St [Np][Mp], StT [Np][Mt], Ks, Np) as views of `prepared`: St by matgcn_supports_layout, the tight copy as the
    LAST block of `prepared`, Np rows of Mt = Ks*N rounded up to 64 floats"""
    import ctypes as C
    hp = p.hp
    hp._need_prepared()
    hp.prepare_join()
    torch.cuda.synchronize()
    lay = (C.c_int64 * 4)()
    assert hp.lib.matgcn_supports_layout(C.byref(hp.dims), lay) == 0
    o_st, mp, np_, ks = (int(v) for v in lay)
    mt = (ks * p.n + 63) // 64 * 64
    o_tight = hp.prepared.numel() - (np_ * mt + 63) // 64 * 64
    assert o_tight >= o_st + np_ * mp
    return (hp.prepared[o_st:o_st + np_ * mp].view(np_, mp), hp.prepared[o_tight:o_tight + np_ * mt].view(np_, mt),
            ks, np_)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_tight_copy_is_the_stack_without_its_padding(shape, synth):
    """StT[m][k*N + n] == St[m][k*Np + n] bit for bit, zero from column Ks*N to the end of the last 64-row tile"""
    p = synth(shape)
    st, tight, ks, np_ = _stacks(p)
    n = p.n
    assert ks == KS[shape[1]] and tight.shape[1] % 64 == 0 and 0 <= tight.shape[1] - ks * n < 64
    for k in range(ks):
        assert torch.equal(tight[:, k * n:(k + 1) * n], st[:, k * np_:k * np_ + n]), k
        assert float(st[:n, k * np_:k * np_ + n].abs().max()) > 0.0, k
    assert not tight[:, ks * n:].any()


@pytest.mark.parametrize("shape", [(21, 3), (43, 3), (64, 1), (67, 3)], ids=["n21_ks3", "n43_ks3", "n64_ks1", "n67_ks3"])
def test_forward_reads_the_tight_copy(shape, synth):
    """with the tight copy overwritten by NaN every prediction is NaN, with St overwritten instead none changes: the
    mixes of an fp32 forward at this batch read StT and nothing else (k_mix_c32, at B <= 16, would read St)"""
    p = synth(shape)
    st, tight, _, _ = _stacks(p)
    want = p.hp.forward(p.x).clone()
    assert torch.isfinite(want).all()
    keep = tight.clone()
    try:
        tight.fill_(float("nan"))
        assert torch.isnan(p.hp.forward(p.x)).all()
        tight.copy_(keep)
        st.fill_(float("nan"))
        assert torch.equal(p.hp.forward(p.x), want)
    finally:
        p.hp.prepare()                        # rebuilds both from the parameters
    assert torch.equal(p.hp.forward(p.x), want)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_matches_the_float64_oracle(shape, synth):
    p = synth(shape)
    got = p.hp.forward(p.x).cpu().numpy()
    assert got.shape == p.want.shape and np.isfinite(got).all()
    err, excess = max_norm_err(got, p.want), elementwise_excess(got, p.want)
    print("n%d ks%s: forward vs fp64 %.3e (element-wise excess %.3f)" % (shape[0], shape[1], err, excess))
    assert err <= E2E_TOL, err
    assert excess <= 1.0, excess


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_one_cell_matches_the_float64_oracle(shape, synth):
    """matgcn_atgru_cell: the two recurrent mixes (of h and of z*h, B = 22 column tiles: k_mix<1> on the tight copy) and
    nothing between them and the oracle but one cell, on a state without zeros - every stacked row and every reduction
    index carries weight.  (The cell's own layer-0 fold has one column tile and takes k_mix_c32.)"""
    from oracle import matgcn_oracle as O
    p = synth(shape)
    rng = np.random.default_rng(shape[0])
    x = rng.standard_normal((BATCH, p.n, 2)).astype(np.float32)
    h = np.tanh(rng.standard_normal((BATCH, p.n, 64))).astype(np.float32)
    got = p.hp.atgru_cell(0, torch.from_numpy(x).to(p.dev), torch.from_numpy(h).to(p.dev)).cpu().numpy()
    want = O.atgru_cell(torch.from_numpy(x).double(), torch.from_numpy(h).double(), p.p64, "encoder.agru_cells.0.",
                        p.st64, p.adjtype, p.adpadj, p.cheb).numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    err = max_norm_err(got, want)
    print("n%d ks%s: cell vs fp64 %.3e" % (shape[0], shape[1], err))
    assert err <= STAGE_TOL, err


@pytest.mark.parametrize("shape", [(21, 3), (403, 3)], ids=["n21_ks3", "n403_ks3"])
def test_wavefront_and_serial_schedules_agree_bitwise(shape, synth):
    p = synth(shape)
    prev = p.hp.lib.matgcn_set_wavefront(1)
    try:
        a = p.hp.forward(p.x).cpu().numpy()
        p.hp.lib.matgcn_set_wavefront(0)
        b = p.hp.forward(p.x).cpu().numpy()
    finally:
        p.hp.lib.matgcn_set_wavefront(prev)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3_train"])
def test_training_step_at_21_nodes_matches_the_oracles_autograd(precision, lib_built):
    """the backward reads St (plain stack, planes) while the forward's fp32 mixes read the tight copy: one training step
    through the plugin, fp32 and three-piece, every gradient within 1e-4 of float64 autograd through the oracle"""
    from multistgraph_amd.model import MultiATGCN
    from oracle import matgcn_oracle as O
    c = Case("tiny_multi_uni_c2")
    assert c.n == 21
    dev = torch.device("cuda:0")
    model = MultiATGCN(dict(c.config("cuda:0"), hip_precision=precision), c.data_feature).to(dev).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    y = torch.from_numpy(c.y)
    loss = model.calculate_loss({"X": torch.from_numpy(c.x).to(dev), "y": y.to(dev)})
    loss.backward()
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in c.state.items()}
    sc = c.data_feature["scaler"]
    ref = O.calculate_loss(torch.from_numpy(c.x).double(), y.double(), p64,
                           O.supports_as_tensors(c.gold["static_supports"], torch.float64), c.oracle_cfg(),
                           mean=float(getattr(sc, "mean", 0.0)), std=float(getattr(sc, "std", 1.0)), faithful=False)
    ref.backward()
    errs = {}
    for k, prm in model.named_parameters():
        w = p64[k].grad
        if w is None or float(w.abs().max()) == 0.0:
            continue
        errs[k] = max_norm_err(prm.grad.cpu().numpy(), w.numpy())
    worst = max(errs, key=errs.get)
    print("%s: loss %.6f (oracle %.6f), worst gradient %.3e (%s)" % (precision, float(loss.detach()), float(ref.detach()),
                                                                     errs[worst], worst))
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-4 * abs(float(ref.detach()))
    bad = {k: e for k, e in errs.items() if e > GRAD_TOL}
    assert len(errs) > 10 and not bad, bad
