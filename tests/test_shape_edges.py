"""Every shape-dependent kernel choice of the host schedule, run on the far side of its rule.

The library picks kernels by N and B.  Each case below is the smallest shape that sits on one side of such a rule; its
truth is the CPU oracle in float64 (tests/golden/make_edge_golden.py -> edge_*.npz; the oracle is pinned to the reference
by test_oracle_golden.py).  Whoever moves a threshold moves the shape with it:

  case            - rule                                                                   - where the rule lives
  edge_n48_b3     - Np 48 != NpC 64, Ks*Np = 144 (ragged 64-row mix tile), odd rows        - matgcn_bwd.hip:launch_mix_plain / mix_backward_tile
  edge_n64_b17    - N = Np = NpC (no padding row); first B past k_mix_c32 and NRT 1        - matgcn_capi.hip:mix_half_tiles (nColTiles <= 16), hoist_x (nrt)
  edge_n65_b16    - one node past a tile: Np 80, NpC 128; last B of k_mix_c32 and NRT 1    - matgcn_capi.hip:plan_from_dims, mix_half_tiles, hoist_x
  edge_n256_b33   - last N of the 32-row items at B > 32; first B of NRT 4; 2 blocks of 32 - matgcn_capi.hip:cell_phase (rows32), hoist_x (nrt)
  edge_n257_b33   - first shape on 64-row items by both criteria; Np 272, NpC 320          - matgcn_capi.hip:cell_phase (rows32)
  edge_n257_b65   - 64-row items, two row blocks per node (RB = 2): rb / rtb of PX and R   - matgcn_node16.hip:node_item, k_gate16 / k_update16 (RB, rb, rtb)
  edge_n256_b65   - three 32-row blocks per node, the last with one real row               - matgcn_node16.hip:node_item / node_items
  edge_n263_b8    - N % 8 = 7 (grids round N up to 8); nColTiles % 8 == 0 swizzle in c32   - matgcn_node16.hip:node_items, matgcn_kernels.hip:k_mix_c32
  edge_n1024_b2   - nK = 64: the longest reduction chain without FLUSH, even rows          - matgcn_capi.hip:mix_flush (a.nK > 64)
  edge_n1039_b3   - Np 1040, nK = 65: FLUSH, odd nK, last group of one tile; odd rows      - matgcn_capi.hip:mix_flush, matgcn_kernels.hip:k_mix<., true>
  edge_n1039_b2   - the same N with even rows (forward only)                               - matgcn_bwd.hip:mix_backward_tile ((rows & 1) == 0)
  edge_n21_b129   - RB = 3; carrier of precision mode 2 (always 64-row items) at B > 64    - matgcn_capi.hip:cell_phase (!c.prec.node)

The library also picks kernels by the configuration, and a configuration-dependent kernel has to be run past its first
tile as well.  The cases below carry a configuration of their own (edge_index.json holds it whole; everything not
named here is the default above: multi / unidirection, cheb_order 2, two layers, two input channels, 24 -> 6, embed_dim_node
20, no initial state).  The synthetic data has no static features, so the similarity support of 'multi' is -I: it is
diagonal and folded into the weights, and 'multi' has three dense first-order supports with an adaptive one (adaptive,
od, dist) and two without.  Ks = dense slots of the stack (matgcn_capi.hip:make_plan), confirmed per case by
test_host_logic.py::test_plans_of_the_configuration_edge_cases:

  case                  - configuration            - rule                                                          - where the rule lives
  edge_c3_n65_b5        - cheb 3                   - Ks 6 > MAX_FUSED_PARTS (4): k_chain_res_fused + the CHAIN_NODE  - matgcn_bwd.hip:bwd_chain (fused), matgcn_capi.hip:prepare_impl
                                                     pair on (5*80+63)/64 = 7 workgroups, the last with 16 of its 64
                                                     rows; non-direct prepare, recursion with NpC/64 = 2 column
                                                     tiles, tgrid 3 x 3
  edge_c3bi_n257_b3     - cheb 3, bidirection, h0  - k_adaptive_adj takes a second trip of its 256-thread loops,    - matgcn_capi.hip:prepare_impl, matgcn_bwd.hip:bwd_chain (k_dh0_out)
                                                     rank = embed_dim_node; k_dh0_out adds 6 parts; Np 272, NpC 320
  edge_c3none_n80_b17   - cheb 3, adpadj none      - Ks 4 = MAX_FUSED_PARTS, the last stack on the fused chain;     - matgcn_capi.hip:prepare_impl (hasAdp, cheb), matgcn_bwd.hip:bwd_chain
                                                     no adaptive support (plainA serves the recursion only);
                                                     N = Np, NpC 128
  edge_c4_n65_b3        - cheb 4                   - iPrev2 >= 0: three-buffer rotation, k_cheb_combine with a real - matgcn_capi.hip:prepare_impl (iOut = 3 - iPrev1 - iPrev2)
                                                     T_{k-2}; Ks 9, a reference stack of 13
  edge_c1_n65_b17_l3    - cheb 1, 3 layers         - sumDense: three dense supports accumulated into one slot over  - matgcn_capi.hip:make_plan (sumDense), prepare_impl (accumulate)
                                                     3 x 3 tiles of k_static_transpose; Ks 1; odd layer count
  edge_oduni_n65_b3     - od / unidirection        - the adaptive support alone on the direct path: k_adaptive_stack - matgcn_capi.hip:prepare_impl (direct, tail = 1)
                                                     writes the tail padding; no static support; Ks 1
  edge_dist_n65_b33_l1  - dist / none, 1 layer     - k_static_stack alone; L = 1 (one parity buffer, no layer above);- matgcn_capi.hip:prepare_impl (direct, nStatic), matgcn_bwd.hip (P.L > 1)
                                                     two 32-row blocks
  edge_ident_c3_n65_b5  - cheb 3, identity / none  - Ks 0: every slot folded into the weights, no mix anywhere,      - matgcn_capi.hip:make_plan (diagFirst), matgcn_bwd.hip (P.Ks > 0)
                                                     over more than one node tile
  edge_ext13_n65_b7     - 14 input channels        - (Ks+1)*C0*T*B = 4*14*24*7 = 9408 > 8192: bChunk 7 -> 3,        - matgcn_capi.hip:fold_x0 (T = 24 from forward_impl)
                                                     grid.y 3 with a last chunk of one sample (B = 5 and 6 still
                                                     fit: 6720, 8064); Kx 64; the C0 = 14 narrow variants
  edge_ext8_n48_b17     - 9 input channels         - 4*9*24*16 = 13824 > 8192: bChunk 16 -> 8, grid.y 3 with a last - matgcn_capi.hip:fold_x0
                                                     chunk of one sample; Kx 48
  edge_ext0_n65_b16     - the flow channel alone   - C0 1, Kx 16                                                    - matgcn_capi.hip:make_plan (Kx)
  edge_od2_out24_n65_b3 - end_dim 2, 24 steps out  - out_channels 48: NTc 2, the second 32-channel tile of k_head   - matgcn_capi.hip:make_plan (NTc), matgcn_kernels.hip:k_head
                                                     with two interleaved output channels
  edge_l4_n48_b3        - 4 layers, h0             - MATGCN_MAX_LAYERS; d_h0 of four layers                         - include/matgcn.h, matgcn_capi.hip:make_plan
  edge_emb8_n65_b3      - embed_dim_node 8         - k_prep_mfma<3> and the pool gradients over 65 nodes            - matgcn_capi.hip:prepare_impl, matgcn_bwd.hip:bwd_pools_layer
  edge_emb40_n65_b3     - embed_dim_node 40        - P.d > 32: the kernels for wide embeddings (k_prep_stream, the  - matgcn_capi.hip:prepare_impl, matgcn_bwd.hip:bwd_pools_layer
                                                     generic pool-gradient GEMMs) over 65 nodes

Every configuration case was admitted by the generator's own rule: the oracle's fp32 run is within 5e-6 of its fp64 run
on the prediction and on every gradient tensor (1/20 of the tolerance below) - where the Chebyshev recursion is
ill-conditioned in fp32 itself (cheb_order 4 on od / unidirection, cheb_order 5 on dist / none) a case would test the
number format and is left out.  The bf16 modes 1 and 2 stay out of the configuration cases: their 5e-3 / 2.7e-2 bounds
were measured on cheb_order 2 stacks only, and nothing tells what a squared support costs them.  An `h0` case starts
every layer and sample from the seeded (N, H) state of its fixture; the fixture holds the gradient of that state, which
the HIP path's d_h0 (L, B, N, H) sums to over layers and batch.

Tolerances are the project's own and do not depend on what the kernels give: 1e-4 max-normalised and element-wise
(helpers.elementwise_excess) for the forward - 140 x the oracle's own fp32-vs-fp64 gap, which every fixture carries as
gap32_pred / gap32_grad and every test prints next to the measured distance -, 1e-4 per gradient tensor, 2e-4 on the sums
of the subsampled ones, 5e-3 / 2.7e-2 for the bf16 modes (test_hip_parity.py, test_train_precision.py; measured at
N <= 403, which is why the precision cases stay there).
"""
import numpy as np
import pytest
import torch

from helpers import EDGE, EDGE_GRAD, EdgeCase, elementwise_excess, max_norm_err

pytestmark = pytest.mark.gpu

E2E_TOL = 1e-4
GRAD_TOL = 1e-4
GRAD_SUM_TOL = 2e-4
BF16_TOL = 5e-3            # test_hip_parity.py
GRAD_BF16_TOL = 2.7e-2     # test_train_precision.py
PRECISION_CASES = ["edge_n257_b65", "edge_n256_b65", "edge_n21_b129"]


class _Bound:
    """an edge case bound to the HIP path, its fp32 forward computed once"""

    def __init__(self, name):
        from multistgraph_amd.ops import HotPath
        c = self.c = EdgeCase(name)
        self.dev = torch.device("cuda:0")
        spec, st = c.spec_and_static()
        self.hp = HotPath(spec, c.b, self.dev)
        self.state = {k: torch.from_numpy(v).to(self.dev) for k, v in c.state.items()}
        self.hp.bind(self.state, None if st is None else st.to(self.dev))
        self.x = torch.from_numpy(c.x).to(self.dev)
        h0 = c.h0()             # (N, H) -> the (L, B, N, H) the C ABI takes: every layer and sample starts from it
        self.h0 = None if h0 is None else \
            torch.from_numpy(h0).to(self.dev).expand(spec.layers, c.b, -1, -1).contiguous()
        self.pred = self.hp.forward(self.x, self.h0).clone()

    def zeros(self):
        s = self.hp.spec
        return torch.zeros(s.layers, self.hp.batch, s.nodes, s.hidden, dtype=torch.float32, device=self.dev)


@pytest.fixture(scope="module")
def bound(lib_built):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _Bound(name)
        return cache[name]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", EDGE)
def test_inputs_parameters_and_host_graph_prep_match_the_fixture(name, bound):
    c = bound(name).c
    assert c.checksum_errors() == []
    if c.grad_gold is not None:
        assert c.checksum_errors(c.grad_gold) == []


@pytest.mark.parametrize("name", EDGE)
def test_forward_matches_the_float64_oracle(name, bound):
    p = bound(name)
    got, want = p.pred.cpu().numpy(), p.c.gold["pred64"]
    assert got.shape == want.shape and np.isfinite(got).all()
    err, excess = max_norm_err(got, want), elementwise_excess(got, want)
    print("%s: forward vs fp64 %.3e (element-wise excess %.3f); oracle fp32 vs fp64 %.3e" % (
        name, err, excess, float(p.c.gold["gap32_pred"])))
    assert err <= E2E_TOL, err
    assert excess <= 1.0, excess


@pytest.mark.parametrize("name", EDGE)
def test_wavefront_and_serial_schedules_agree_bitwise(name, bound):
    p = bound(name)
    prev = p.hp.lib.matgcn_set_wavefront(1)
    try:
        a = p.hp.forward(p.x, p.h0).cpu().numpy()
        p.hp.lib.matgcn_set_wavefront(0)
        b = p.hp.forward(p.x, p.h0).cpu().numpy()
    finally:
        p.hp.lib.matgcn_set_wavefront(prev)
    assert np.array_equal(a, b)
    assert np.array_equal(a, p.pred.cpu().numpy())


@pytest.mark.parametrize("name", EDGE)
def test_forward_without_h0_equals_forward_from_explicit_zeros(name, bound):
    """the contract of test_zero_state_start.py: the zero-state instantiations against the general path (an `h0` case
    too: its fixture comparison runs from the case's state, this one from none and from zeros)"""
    p = bound(name)
    ref = p.hp.forward(p.x, p.zeros()).cpu().numpy()
    assert np.isfinite(ref).all()
    assert np.array_equal(p.hp.forward(p.x).cpu().numpy(), ref)


def _grad_errors(gold, grads):
    """max-normalised error of every gradient against the fixture (tensors above 20000 elements: every `sub`-th element,
    and their sum against the stored [sum, sum |.|]); returns (errors of the non-zero tensors, violations of the sum and
    expected-zero checks)"""
    sub = int(gold["sub"])
    errs, bad = {}, {}
    for k, g in grads.items():
        g = g.detach().cpu().numpy()
        if "grad." + k in gold:
            got, w = g, gold["grad." + k]
        else:
            got, w = g.reshape(-1)[::sub], gold["gsub." + k]
            sums = gold["gsum." + k]
            if abs(float(g.astype(np.float64).sum()) - sums[0]) > GRAD_SUM_TOL * max(sums[1], 1e-30):
                bad[k + " (sum)"] = float(g.astype(np.float64).sum()), float(sums[0])
        assert got.shape == w.shape, k
        if np.abs(w).max() == 0.0:
            if float(np.abs(got).max()) > 1e-6:
                bad[k] = "expected zero"
        else:
            errs[k] = max_norm_err(got, w)
    return errs, bad


def _fold_d_h0(grads):
    """the HIP path's d_h0 (L, B, N, H) summed over layers and batch (in float64): the gradient of the (N, H) state
    that an `h0` case expands to every layer and sample, which is what its fixture holds"""
    from multistgraph_amd.ops import HotPath
    if HotPath.D_H0 in grads:
        grads[HotPath.D_H0] = grads[HotPath.D_H0].double().sum((0, 1))
    return grads


def _fixture_keys(gold):
    return {k[5:] for k in gold.files if k.startswith("grad.") or k.startswith("gsub.")}


@pytest.mark.parametrize("name", EDGE_GRAD)
def test_training_step_matches_the_float64_autograd(name, bound):
    p = bound(name)
    gold = p.c.grad_gold
    assert torch.equal(p.hp.forward_train(p.x, None, p.h0), p.pred)   # the saving instantiations compute the same forward
    grads = p.hp.backward(p.x, torch.from_numpy(p.c.d_out()).to(p.dev), p.state, None, p.h0)
    torch.cuda.synchronize()
    _fold_d_h0(grads)
    assert set(grads) == _fixture_keys(gold)
    errs, bad = _grad_errors(gold, grads)
    worst = max(errs, key=errs.get)
    print("%s: worst gradient vs fp64 %.3e (%s); oracle fp32 vs fp64 %.3e" % (
        name, errs[worst], worst, float(gold["gap32_grad"])))
    bad.update({k: e for k, e in errs.items() if e > GRAD_TOL})
    assert not bad, bad
    p.hp._train = None                                           # the train buffer of this shape is not needed again


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", PRECISION_CASES)
def test_inference_precision_modes(name, mode, bound):
    """matgcn_set_mix_precision(1 / 2): mode 2 always runs 64-row items - here with 2 and 3 row blocks per node"""
    p = bound(name)
    prev = p.hp.lib.matgcn_set_mix_precision(mode)
    try:
        got = p.hp.forward(p.x).clone()
        from_zeros = p.hp.forward(p.x, p.zeros())
    finally:
        p.hp.lib.matgcn_set_mix_precision(prev)
    assert not torch.equal(got, p.pred)                          # the variant really ran
    err = max_norm_err(got.cpu().numpy(), p.c.gold["pred64"])
    print("%s mode %d: forward vs fp64 %.3e" % (name, mode, err))
    assert err <= BF16_TOL, err
    assert np.array_equal(got.cpu().numpy(), from_zeros.cpu().numpy())
    assert torch.equal(p.hp.forward(p.x), p.pred)                # and the default is untouched afterwards


@pytest.mark.parametrize("mode", [1, 2])
def test_training_precision_modes_with_two_row_blocks(mode, bound):
    p = bound("edge_n257_b65")
    gold = p.c.grad_gold
    d_out = torch.from_numpy(p.c.d_out()).to(p.dev)
    prev = p.hp.lib.matgcn_set_train_precision(mode)
    try:
        y = p.hp.forward_train(p.x).clone()
        grads = p.hp.backward(p.x, d_out, p.state)
        torch.cuda.synchronize()
    finally:
        p.hp.lib.matgcn_set_train_precision(prev)
        p.hp._train = None
    assert not torch.equal(y, p.pred)                            # the bf16 training forward ran
    perr = max_norm_err(y.cpu().numpy(), p.c.gold["pred64"])
    errs, _ = _grad_errors(gold, grads)          # (the 2e-4 sum check belongs to the fp32 path)
    worst = max(errs, key=errs.get)
    print("edge_n257_b65 training mode %d: forward vs fp64 %.3e, worst gradient %.3e (%s)" % (mode, perr, errs[worst], worst))
    assert perr <= BF16_TOL, perr
    bad = {k: e for k, e in errs.items() if e > GRAD_BF16_TOL}
    assert not bad, bad
    assert torch.equal(p.hp.forward_train(p.x), p.pred)          # fp32 again once the setting is restored
    p.hp._train = None
