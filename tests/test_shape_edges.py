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
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        c = self.c = EdgeCase(name)
        self.dev = torch.device("cuda:0")
        st = torch.from_numpy(c.mats)
        spec = spec_from_config(c.config(), c.data_feature, c.n, min(c.n, 20), st.shape[0], diagonal_mask(st))
        self.hp = HotPath(spec, c.b, self.dev)
        self.state = {k: torch.from_numpy(v).to(self.dev) for k, v in c.state.items()}
        self.hp.bind(self.state, st.to(self.dev))
        self.x = torch.from_numpy(c.x).to(self.dev)
        self.pred = self.hp.forward(self.x).clone()

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
        a = p.hp.forward(p.x).cpu().numpy()
        p.hp.lib.matgcn_set_wavefront(0)
        b = p.hp.forward(p.x).cpu().numpy()
    finally:
        p.hp.lib.matgcn_set_wavefront(prev)
    assert np.array_equal(a, b)
    assert np.array_equal(a, p.pred.cpu().numpy())


@pytest.mark.parametrize("name", EDGE)
def test_forward_without_h0_equals_forward_from_explicit_zeros(name, bound):
    """the contract of test_zero_state_start.py: the zero-state instantiations against the general path"""
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


def _fixture_keys(gold):
    return {k[5:] for k in gold.files if k.startswith("grad.") or k.startswith("gsub.")}


@pytest.mark.parametrize("name", EDGE_GRAD)
def test_training_step_matches_the_float64_autograd(name, bound):
    p = bound(name)
    gold = p.c.grad_gold
    assert torch.equal(p.hp.forward_train(p.x), p.pred)          # the saving instantiations compute the same forward
    grads = p.hp.backward(p.x, torch.from_numpy(p.c.d_out()).to(p.dev), p.state)
    torch.cuda.synchronize()
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
