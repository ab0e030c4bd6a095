"""The setup chain in front of layer 0's first step: what matgcn_prepare and a forward write before the first gate kernel.

matgcn_prepare builds both support stacks (St, and its tight copy StT) in at most two launches that also write all of
their padding (k_adaptive_stack, k_static_stack), and the dense weights in one launch on a library stream (k_prep_dense);
a forward writes the padding rows of x0p in k_fuse_heads, folds the layer-0 x part through LDS (k_build_xa0) and
initialises the state of every layer in one launch in front of the fork (k_state_init).  No buffer is memset any more, so
the cases below start from buffers filled with NaN: whatever is read without having been written shows in the result.

Shapes (OUT = 3): N = 17 (15 padding rows), 32 (Np == N: none), 33, 67;  B = 3 (the mixes take k_mix_c32 and read St, the
layer-0 matrix has padding columns) and 22 (the mixes read StT);  modes multi / unidirection (adaptive + static),
multi / none (static only), od / none (Ks = 1), cheb_order 3 (the retained recursion), cheb_order 1 (the retained
accumulate path);  one case with C0 = 4 input channels (time of day + two dynamic channels).

Truth is the CPU oracle in float64 (hoisted order), once per case.  Tolerances are the suite's own (test_mix_tight_stack.py):
1e-4 max-normalised and element-wise for a forward, 2e-5 for the stack, 1e-4 per gradient tensor.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import elementwise_excess, max_norm_err

pytestmark = pytest.mark.gpu

E2E_TOL = 1e-4
STAGE_TOL = 2e-5
GRAD_TOL = 1e-4
OUT = 3

MODES = {"multi_uni": ("multi", "unidirection", 2), "multi_none": ("multi", "none", 2), "od": ("od", "none", 2),
         "cheb3": ("od", "none", 3), "cheb1": ("multi", "unidirection", 1)}
CASES = [(n, b, m, 2) for m in MODES for n in (17, 32, 33, 67) for b in (3, 22)] + [(33, 22, "multi_uni", 4)]
IDS = ["n%d_b%d_%s_c%d" % c for c in CASES]
NAN = float("nan")


class _Synth:
    """a synthetic case of any size, built the way helpers.EdgeCase builds its own, bound to the HIP path; the float64
    oracle's parameters and supports beside it.  feat: input channels C0 (2: flow + time of day; more: dynamic ones)"""

    def __init__(self, n, batch, mode, feat=2, seed_shift=0, oracle=True):
        from multistgraph_amd import graph_prep, synthetic as syn
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        from oracle import matgcn_oracle as O
        self.n, self.b, self.mode, self.feat = n, batch, mode, feat
        self.adjtype, self.adpadj, self.cheb = MODES[mode]
        seed = 300 + n + seed_shift
        df = syn.make_data_feature(n, 300 + n, "DC", ext_dim=feat - 1)
        self.mats = np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None, self.adjtype), 0)
        shapes = syn.param_shapes(n, out_steps=OUT, feat_in=feat,
                                  k_total=syn.k_total_for(self.adjtype, self.adpadj, self.cheb))
        self.state = syn.closed_form_state(shapes, seed)
        x, _ = syn.make_batch_arrays(batch, n, OUT, 300 + n, feat=feat)
        common = dict(output_window=OUT, input_window=24, add_time_in_day=True, add_day_in_week=False,
                      load_dynamic=feat > 2, adjtype=self.adjtype, adpadj=self.adpadj, cheb_order=self.cheb,
                      rnn_units=64, num_layers=2, start_dim=0, end_dim=1)
        cfg = dict(common, embed_dim_node=20, embed_dim_adj=20, device=torch.device("cpu"), batch_size=batch)
        self.ocfg = dict(common, len_closeness=48, len_period=24, len_trend=24)
        self.dev = torch.device("cuda:0")
        st = torch.from_numpy(self.mats)
        spec = spec_from_config(cfg, df, n, min(n, 20), st.shape[0], diagonal_mask(st))
        assert spec.feat_in == feat
        self.hp = HotPath(spec, batch, self.dev)
        self.dev_state = {k: torch.from_numpy(v).to(self.dev) for k, v in self.state.items()}
        self.dev_static = st.to(self.dev)
        self.hp.bind(self.dev_state, self.dev_static)
        self.x_np = x
        self.x = torch.from_numpy(x).to(self.dev)
        rng = np.random.default_rng(n)
        self.h0_np = np.tanh(rng.standard_normal((n, 64))).astype(np.float32)          # the oracle's (N, H) initial state
        self.h0 = torch.from_numpy(self.h0_np).to(self.dev).expand(2, batch, -1, -1).contiguous()
        self.p64 = O.to_tensors(self.state, torch.float64)
        self.st64 = O.supports_as_tensors(self.mats, torch.float64)
        self._want = {}

    def want(self, h0=False):
        """the float64 oracle's prediction, computed once and kept"""
        from oracle import matgcn_oracle as O
        if h0 not in self._want:
            self._want[h0] = O.forward(torch.from_numpy(self.x_np).double(), self.p64, self.st64, self.ocfg, faithful=False,
                                       h0=torch.from_numpy(self.h0_np).double() if h0 else None).numpy()
        return self._want[h0]

    def fill(self, value, train=False):
        """every caller-owned buffer of the binding <- value, behind whatever still writes them"""
        self.hp.prepare_join()
        torch.cuda.synchronize()
        self.hp.prepared.fill_(value)
        self.hp.workspace.fill_(value)
        if train:
            self.hp._train_buffer().fill_(value)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def synth(lib_built):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _Synth(*case)
        return cache[case]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


def _close_to_oracle(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all(), what
    err, excess = max_norm_err(got, want), elementwise_excess(got, want)
    print("%s: vs fp64 %.3e (element-wise excess %.3f)" % (what, err, excess))
    assert err <= E2E_TOL, (what, err)
    assert excess <= 1.0, (what, excess)


# ---- 1. dirty buffers ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_from_nan_filled_buffers(case, synth):
    """`prepared` and the workspace full of NaN, then prepare and forward - without and with an initial state: the bits
    of the same calls from zero-filled buffers, and the float64 oracle's values"""
    p = synth(case)
    res = {}
    for value in (0.0, NAN):
        p.fill(value)
        p.hp.prepare()
        res[value != 0.0] = (p.hp.forward(p.x).clone(), p.hp.forward(p.x, p.h0).clone())
    for i, what in enumerate(("zero state", "h0")):
        assert torch.equal(res[True][i], res[False][i]), what
        _close_to_oracle(res[True][i], p.want(h0=bool(i)), "%s %s" % (IDS[CASES.index(case)], what))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_train_from_nan_filled_buffers(case, synth):
    """the training forward - same setup code, plus the backward's copy of h0 - on a NaN-filled train buffer"""
    p = synth(case)
    res = {}
    for value in (0.0, NAN):
        p.fill(value, train=True)
        p.hp.prepare()
        res[value != 0.0] = (p.hp.forward_train(p.x).clone(), p.hp.forward_train(p.x, h0=p.h0).clone())
    for i, what in enumerate(("zero state", "h0")):
        assert torch.isfinite(res[True][i]).all(), what
        assert torch.equal(res[True][i], res[False][i]), what


def test_gradients_at_21_nodes_from_nan_filled_buffers(lib_built):
    """one training step at N = 21 (multi / unidirection, B = 3) from NaN-filled buffers, with an initial state: every
    gradient within 1e-4 of float64 autograd through the oracle (loss = sum(prediction * d_out))"""
    from oracle import matgcn_oracle as O
    p = _Synth(21, 3, "multi_uni")
    d_out = np.random.default_rng(9).standard_normal((3, OUT, 21, 1)).astype(np.float32)
    p.fill(NAN, train=True)
    p.hp.prepare()
    out = p.hp.forward_train(p.x, h0=p.h0)
    grads = p.hp.backward(p.x, torch.from_numpy(d_out).to(p.dev), p.dev_state, h0=p.h0)
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.state.items()}
    ref = O.forward(torch.from_numpy(p.x_np).double(), p64, p.st64, p.ocfg, faithful=False,
                    h0=torch.from_numpy(p.h0_np).double())
    _close_to_oracle(out, ref.detach().numpy(), "n21 forward_train")
    (ref * torch.from_numpy(d_out).double()).sum().backward()
    errs = {}
    for k, w in p64.items():
        if w.grad is None or float(w.grad.abs().max()) == 0.0 or k not in grads:
            continue
        errs[k] = max_norm_err(grads[k].cpu().numpy(), w.grad.numpy())
    worst = max(errs, key=errs.get)
    print("worst gradient %.3e (%s) of %d" % (errs[worst], worst, len(errs)))
    bad = {k: e for k, e in errs.items() if not e <= GRAD_TOL}
    assert len(errs) > 10 and not bad, bad


# ---- 2. padding of the stacks ----------------------------------------------------------------------------------------
def _stacks(p):
    """(St [Np][Mp], StT [Np][Mt], Ks, Np) as views of `prepared`: St by matgcn_supports_layout, the tight copy as the
    LAST block of `prepared`, Np rows of Mt = Ks*N rounded up to 64 floats"""
    hp = p.hp
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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_stacks_and_their_padding_after_a_prepare_on_nan(case, synth):
    from oracle import matgcn_oracle as O
    p = synth(case)
    n = p.n
    p.fill(NAN)
    p.hp.prepare()
    st, tight, ks, np_ = _stacks(p)
    stack = O.support_stack(p.p64, p.st64, p.adjtype, p.adpadj, p.cheb, None).numpy()[1:]
    dense = [s for s in stack if np.abs(s - np.diag(np.diagonal(s))).max() > 0]
    if p.cheb == 1:
        dense = [np.sum(dense, 0)]            # cheb_order = 1: the dense supports share one slot
    assert ks == len(dense) and ks >= 1
    inside = torch.zeros_like(st, dtype=torch.bool)
    for k in range(ks):
        inside[:n, k * np_:k * np_ + n] = True
        got = st[:n, k * np_:k * np_ + n].t().cpu().numpy()      # St[m][k*Np + n] = S_k[n][m]
        assert max_norm_err(got, dense[k]) <= STAGE_TOL, k
        assert torch.equal(tight[:, k * n:(k + 1) * n], st[:, k * np_:k * np_ + n]), k      # rows m >= N included
    assert torch.isfinite(st).all() and torch.isfinite(tight).all()
    assert not st[~inside].any()                                   # pad columns of every slot, rows m >= N, the Mp tail
    assert not tight[:, ks * n:].any()
    assert not tight[n:].any() and not st[n:].any()


# ---- 3. ordering -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(33, 22, "multi_uni", 2), (33, 3, "multi_uni", 2), (17, 22, "multi_none", 2)],
                         ids=["n33_b22_multi_uni", "n33_b3_multi_uni", "n17_b22_multi_none"])
def test_alternating_parameter_sets_without_synchronisation(case, synth):
    """bind / prepare / forward of two parameter sets in turn, ten times, nothing between the calls: a launch that a
    reader of Rg / Ru / Head, of the stacks or of the initial state is not ordered behind reads the other set's values"""
    p = synth(case)
    q = _Synth(case[0], case[1], case[2], case[3], seed_shift=1000)      # the second parameter set, and its reference
    sets = [(p.dev_state, p.hp.forward(p.x).clone()), (q.dev_state, q.hp.forward(p.x).clone())]
    assert not torch.equal(sets[0][1], sets[1][1])
    torch.cuda.synchronize()
    got = []
    for i in range(10):
        p.hp.bind(sets[i & 1][0], p.dev_static)
        p.hp.prepare()
        got.append(p.hp.forward(p.x).clone())
    torch.cuda.synchronize()
    p.hp.bind(p.dev_state, p.dev_static)
    p.hp.prepare()
    for i, g in enumerate(got):
        assert torch.equal(g, sets[i & 1][1]), i


# ---- 4. schedules ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_three_schedules_agree_bitwise(case, synth):
    """one stream (matgcn_set_wavefront(0)), the default, and an eagerly joined prepare (matgcn_set_lazy_prepare(0)):
    prepare + forward from NaN-filled buffers under each, the same bits"""
    p = synth(case)
    lib = p.hp.lib
    res = []
    for wavefront, lazy in ((0, None), (None, None), (None, 0)):
        p.fill(NAN)
        pw = lib.matgcn_set_wavefront(wavefront) if wavefront is not None else None
        pl = lib.matgcn_set_lazy_prepare(lazy) if lazy is not None else None
        try:
            p.hp.prepare()
            res.append((p.hp.forward(p.x).clone(), p.hp.forward(p.x, p.h0).clone()))
            torch.cuda.synchronize()
        finally:
            if pw is not None:
                lib.matgcn_set_wavefront(pw)
            if pl is not None:
                lib.matgcn_set_lazy_prepare(pl)
    assert torch.isfinite(res[1][0]).all() and torch.isfinite(res[1][1]).all()
    for r in (res[0], res[2]):
        assert torch.equal(r[0], res[1][0]) and torch.equal(r[1], res[1][1])


# ---- 5. series entry -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(33, 22, "multi_uni", 2), (17, 3, "multi_uni", 2)], ids=["n33_b22", "n17_b3"])
def test_forward_series_from_a_nan_filled_workspace(case, synth):
    """matgcn_forward_series shares k_fuse_heads: the windows gathered from a resident series give the bits of the
    forward over the same windows, from a dirty workspace too"""
    p = synth(case)
    xs = p.x.shape[1]
    series = torch.from_numpy(np.random.default_rng(5).standard_normal((xs + 40, p.n, p.feat)).astype(np.float32)).to(p.dev)
    label = torch.arange(p.b, dtype=torch.int32, device=p.dev) + xs
    rel = list(range(-xs, 0))
    windows = torch.stack([series[int(l) - xs:int(l)] for l in label.cpu()], 0).contiguous()
    p.fill(0.0)
    p.hp.prepare()
    want = p.hp.forward(windows).clone()
    p.fill(NAN)
    p.hp.prepare()
    got = p.hp.forward_series(series, label, rel)
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
