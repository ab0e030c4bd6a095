"""Every entry point keeps the order of a caller's own stream.

include/matgcn.h promises that the library forks onto its own streams and joins back "so the caller still sees one
in-order stream".  The cases below hold every entry point to that sentence with the gated sandwich of stream_gate.py:
inputs that were written on the caller's stream microseconds before the call must be read (read-after-write at entry),
outputs must be complete and inputs, workspace and train buffer free again once the stream is past the call (writes and
reads complete at exit), and the one documented exception - a lazy matgcn_prepare - may run on as far as promises (a) and
(b) at matgcn_set_lazy_prepare allow and no further.

Callers: the null stream and four side streams created one after the other (stream_gate.caller_streams).  The forward
family runs under all five; the heavier sandwiches (training step, precision modes) under the null stream and the first
and third side stream - nothing here can show which hardware queue a stream got, so the choice follows the round robin
the header describes and is not a measurement.

Reference: the same binding and values on the null stream, a device synchronisation between all steps,
matgcn_set_wavefront(0).  Forwards and the deterministic backward must give its bits; the default backward (fp32 atomics)
is held to the bound the suite already uses between schedules, 2e-6 x max|g| per tensor (test_sharding.py).  The
reference's own fp32 forward is held to the float64 oracle once per case at the suite's 1e-4 (test_forward_setup.py), so
that two equal wrong answers do not pass.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import stream_gate as SG
from helpers import max_norm_err
from stream_gate import bits_equal, caller_name, sandwich

E2E_TOL = 1e-4          # a forward against the float64 oracle (the suite's own, test_forward_setup.py)
ATOMIC_TOL = 2e-6       # x max|g|: two runs of the default backward (test_sharding.py, between the stream modes)
OUT = 3
MC_SAMPLES = 3

# id -> (N, B, layers, flags): the smallest shapes that have every edge.  T = 24 everywhere: the backward's x-column
# chunks are 6 steps.
CASES = {
    "l2_n33_b3": (33, 3, 2, {}),                       # k_mix_c32, padding rows, chain[1], xpart[1]
    "l3_n67_b22": (67, 22, 3, {}),                     # chain[2]; the backward's l + 2 < L scratch-reuse wait; bchain takes
                                                       # the middle layer
    "l4_n32_b5": (32, 5, 4, {"adpadj": "none"}),       # all of MATGCN_MAX_LAYERS, Np == N, static stack only
    "l1_n21_b3": (21, 3, 1, {"adjtype": "od", "adpadj": "none"}),   # no layer wavefront: fork / join degenerate
    "gcnoff_l3": (21, 2, 3, {"gcn_off": True}),        # bwd_dense_layer; the late bwd_fuse_heads
    "fnnoff_l2": (21, 2, 2, {"fnn_off": True}),        # headT = 1
}
FORWARD_KINDS = ["prepare_eager", "prepare_lazy", "prepare_forward_eager", "prepare_forward_lazy", "forward", "forward_h0",
                 "forward_series", "forward_train_mask", "forward_train_seeded", "forward_mc"]
HEAVY_KINDS = ["train_backward_det", "train_backward_atomic"]
HEAVY_CALLERS = (0, 1, 3)       # the null stream, the first and the third side stream
PRECISION_CASES = ["l2_n33_b3", "l3_n67_b22"]


class Binding:
    """one synthetic case bound to the HIP path (built as test_backward_gpu.py builds its synthetic shapes): every float
    input exists twice - the tensor the library reads, and a staging copy the sandwich restores it from"""

    def __init__(self, name):
        from multistgraph_amd import graph_prep, synthetic as syn
        from multistgraph_amd.ops import HotPath, diagonal_mask, spec_from_config
        self.name = name
        n, b, layers, flags = CASES[name]
        self.n, self.b, self.layers = n, b, layers
        adjtype, adpadj = flags.get("adjtype", "multi"), flags.get("adpadj", "unidirection")
        abl = {k: v for k, v in flags.items() if k not in ("adjtype", "adpadj")}
        common = dict(input_window=24, output_window=OUT, add_time_in_day=True, add_day_in_week=False, load_dynamic=False,
                      adjtype=adjtype, adpadj=adpadj, cheb_order=2, rnn_units=64, num_layers=layers, start_dim=0,
                      end_dim=1, **abl)
        cfg = dict(common, embed_dim_node=20, embed_dim_adj=20, device=torch.device("cpu"), batch_size=b)
        self.ocfg = dict(common, len_closeness=48, len_period=24, len_trend=24)
        df = dict(syn.make_data_feature(n, 3, "DC", ext_dim=1), output_dim=1, feature_dim=2)
        self.mats = np.stack(graph_prep.build_static_supports(df["adj_mx"], df["coordinate"], None, adjtype), 0)
        shapes = syn.param_shapes(n, out_steps=OUT, feat_in=2, out_dim=1, k_total=syn.k_total_for(adjtype, adpadj, 2),
                                  layers=layers, embed_dim_node=20, len_ts=4, **abl)
        self.state_np = syn.closed_form_state(shapes, 3)
        self.x_np, _ = syn.make_batch_arrays(b, n, OUT, 3, feat=2)
        st = torch.from_numpy(self.mats)
        spec = spec_from_config(cfg, df, n, min(n, 20), st.shape[0], diagonal_mask(st))
        dev = self.dev = torch.device("cuda:0")
        hp = self.hp = HotPath(spec, b, dev)
        self.state = {k: torch.from_numpy(v).to(dev) for k, v in self.state_np.items()}
        self.static = st.to(dev)
        hp.bind(self.state, self.static)
        rng = np.random.default_rng(100 + n)
        self.h0_np = np.tanh(rng.standard_normal((n, 64))).astype(np.float32)
        xs = self.x_np.shape[1]
        series = rng.standard_normal((xs + 40, n, 2)).astype(np.float32)
        self.label = (torch.arange(b, dtype=torch.int32) + xs).to(dev)     # index data: written once, never poisoned
        self.rel = list(range(-xs, 0))
        self.x = torch.from_numpy(self.x_np).to(dev)
        self.h0 = torch.from_numpy(self.h0_np).to(dev).expand(layers, b, -1, -1).contiguous()
        self.series = torch.from_numpy(series).to(dev)
        self.d_out = torch.from_numpy(rng.standard_normal((b, OUT, n, 1)).astype(np.float32)).to(dev)
        self.mask = hp.dropout_mask(11, 0, 0.1)
        torch.cuda.synchronize()
        self.stage = {id(t): t.clone() for t in (self.x, self.h0, self.series, self.d_out, self.mask, self.static)}
        self.stage.update({id(t): t.clone() for t in self.state.values()})
        self.refs = {}
        self.restore()

    def pair(self, *tensors):
        return [(t, self.stage[id(t)]) for t in tensors]

    def params(self):
        return self.pair(self.static, *self.state.values())

    def buffers(self, prepared=False, train=False):
        hp = self.hp
        return [hp.workspace, hp.prepared if prepared else None, hp._train if train else None]

    def restore(self):
        """every input and `prepared` as a synchronised caller leaves them"""
        torch.cuda.synchronize()
        for t in (self.x, self.h0, self.series, self.d_out, self.mask, self.static, *self.state.values()):
            t.copy_(self.stage[id(t)])
        self.hp.prepare()
        self.hp.prepare_join()
        torch.cuda.synchronize()

    def oracle(self):
        from oracle import matgcn_oracle as O
        return O.forward(torch.from_numpy(self.x_np).double(), O.to_tensors(self.state_np, torch.float64),
                         O.supports_as_tensors(self.mats, torch.float64), self.ocfg, faithful=False).numpy()

    # ---- the sandwiches: kind -> what stream_gate.sandwich takes -----------------------------------------------------------
    def spec(self, kind):
        hp, x = self.hp, self.x
        ws = lambda *_: self.buffers()                                              # noqa: E731
        ws_train = lambda *_: self.buffers(train=True)                              # noqa: E731
        out = lambda r: {"out": r}                                                  # noqa: E731
        if kind in ("prepare_eager", "prepare_lazy"):
            lazy = kind.endswith("lazy")

            def call():
                hp.prepare()
                if lazy:            # promise (b): `prepared` is the caller's to read behind matgcn_prepare_join only
                    hp.prepare_join()
            both = lambda *_: self.buffers(prepared=True)                           # noqa: E731
            return dict(lazy=int(lazy), inputs=self.params(), before=both, call=call,
                        outputs=lambda r: {"prepared": hp.prepared}, after=both, dirty=True)
        if kind in ("prepare_forward_eager", "prepare_forward_lazy"):
            lazy = kind.endswith("lazy")

            def call():
                hp.prepare()
                return hp.forward(x)
            # promise (a): the parameters may go once a later call on the stream is enqueued - the forward is one;
            # promise (b): `prepared` of a lazy prepare stays until matgcn_prepare_join, which this sandwich never calls
            return dict(lazy=int(lazy), inputs=self.params() + self.pair(x), before=lambda *_: self.buffers(prepared=True),
                        call=call, outputs=out, after=lambda *_: self.buffers(prepared=not lazy), dirty=True)
        if kind == "forward":
            return dict(inputs=self.pair(x), before=ws, call=lambda: hp.forward(x), outputs=out, after=ws)
        if kind == "forward_h0":
            return dict(inputs=self.pair(x, self.h0), before=ws, call=lambda: hp.forward(x, self.h0), outputs=out, after=ws)
        if kind == "forward_series":
            return dict(inputs=self.pair(self.series), before=ws,
                        call=lambda: hp.forward_series(self.series, self.label, self.rel), outputs=out, after=ws)
        if kind == "forward_train_mask":
            return dict(inputs=self.pair(x, self.mask), before=ws_train,
                        call=lambda: hp.forward_train(x, drop_mask=self.mask), outputs=out, after=ws_train)
        if kind == "forward_train_seeded":
            return dict(inputs=self.pair(x), before=ws_train, call=lambda: hp.forward_train(x, dropout=(11, 0, 0.1)),
                        outputs=out, after=ws_train)
        if kind == "forward_mc":
            return dict(inputs=self.pair(x), before=ws,
                        call=lambda: hp.forward_mc(x, seed=5, offset=2, p=0.1, samples=MC_SAMPLES, keep_samples=True),
                        outputs=lambda r: dict(zip(("mean", "std", "samples"), r)), after=ws)
        if kind in ("train_backward_det", "train_backward_atomic"):
            det = kind.endswith("det")
            # the deterministic step draws its dropout on the device (matgcn_*_seeded), the default one takes the mask
            drop = dict(dropout=(11, 0, 0.1)) if det else dict(drop_mask=self.mask)
            late = lambda *_: self.buffers(train=True) + [self.d_out]               # noqa: E731

            def call():
                pred = hp.forward_train(x, **drop)
                self.d_out.copy_(self.stage[id(self.d_out)])      # written between the two calls, on the stream
                return pred, hp.backward(x, self.d_out, self.state, **drop)
            return dict(det=det, inputs=self.pair(x) if det else self.pair(x, self.mask), before=late, call=call,
                        outputs=lambda r: dict({"g/" + k: v for k, v in r[1].items()}, out=r[0]), after=late)
        raise KeyError(kind)

    def run(self, kind, stream, synchronous=False):
        sp = self.spec(kind)
        hp = self.hp
        prev_lazy = hp.lib.matgcn_set_lazy_prepare(sp["lazy"]) if "lazy" in sp else None
        hp.deterministic = sp.get("det")
        try:
            return sandwich(stream, sp["inputs"], sp["call"], sp["outputs"], sp["after"], poison_before=sp["before"],
                            synchronous=synchronous)
        finally:
            hp.deterministic = None
            if prev_lazy is not None:
                hp.lib.matgcn_set_lazy_prepare(prev_lazy)
            if sp.get("dirty"):
                self.restore()

    def reference(self, kind, precision=None):
        """null stream, a synchronisation between all steps, matgcn_set_wavefront(0); once per (kind, precision)"""
        key = (kind, precision)
        if key not in self.refs:
            prev = self.hp.lib.matgcn_set_wavefront(0)
            try:
                self.refs[key] = self.run(kind, None, synchronous=True)
            finally:
                self.hp.lib.matgcn_set_wavefront(prev)
        return self.refs[key]


class Ctx:
    def __init__(self):
        self.callers = SG.caller_streams()
        self.bindings = {}
        self.worst_atomic = (0.0, "")
        self.oracle_done = set()

    def binding(self, name):
        if name not in self.bindings:
            self.bindings[name] = Binding(name)
        return self.bindings[name]


@pytest.fixture(scope="module")
def ctx(lib_built):
    c = Ctx()
    yield c
    SG.Gate.report()
    print("[stream order] worst default-backward gradient against the synchronised run: %.3f of the %.0e x max|g| bound (%s)"
          % (c.worst_atomic[0], ATOMIC_TOL, c.worst_atomic[1] or "no case ran"))
    c.bindings.clear()
    torch.cuda.empty_cache()


def _mismatches(ctx, got, want, det, what):
    """names of the results that miss the reference: bits, or for the default backward's gradients the atomic bound"""
    bad = []
    assert sorted(got) == sorted(want), what
    for k in sorted(want):
        if det or not k.startswith("g/"):
            if not bits_equal(got[k], want[k]):
                nan = int(torch.isnan(got[k]).sum()) if got[k].is_floating_point() else 0
                bad.append("%s (%d NaN of %d)" % (k, nan, got[k].numel()))
            continue
        scale = float(want[k].abs().max())
        gap = float((got[k].double() - want[k].double()).abs().max())
        ratio = gap / (ATOMIC_TOL * scale) if scale > 0.0 else (0.0 if gap == 0.0 else float("inf"))
        if ratio > ctx.worst_atomic[0] and ratio != float("inf") and ratio == ratio:
            ctx.worst_atomic = (ratio, "%s %s" % (what, k))
        if not ratio <= 1.0:
            bad.append("%s (%.3g x the atomic bound)" % (k, ratio))
    return bad


def _sweep(ctx, case, kind, wavefront, callers, precision=None, x3=None):
    bd = ctx.binding(case)
    hp = bd.hp
    hp.precision, hp.train_bf16x3 = precision, x3
    try:
        want = bd.reference(kind, (precision, x3))
        if kind.startswith("prepare"):
            assert want and all(v.numel() for v in want.values())
        else:
            for k, v in want.items():
                assert torch.isfinite(v).all(), "the synchronised reference of %s holds a non-finite %s" % (kind, k)
        if kind == "forward" and precision is None and case not in ctx.oracle_done:
            err = max_norm_err(want["out"].cpu().numpy(), bd.oracle())
            print("%s: synchronised forward against the float64 oracle %.3e" % (case, err))
            assert err <= E2E_TOL, err
            ctx.oracle_done.add(case)
        failed = {}
        prev = hp.lib.matgcn_set_wavefront(wavefront)
        try:
            for i in callers:
                s = ctx.callers[i]
                bd.run(kind, s, synchronous=True)      # warm-up on this stream: buffer growth and allocator blocks
                got = bd.run(kind, s)
                bad = _mismatches(ctx, got, want, bd.spec(kind).get("det", True), "%s %s wavefront %d" % (case, kind, wavefront))
                if bad:
                    failed[caller_name(i)] = bad
        finally:
            hp.lib.matgcn_set_wavefront(prev)
        assert not failed, failed
    finally:
        hp.precision, hp.train_bf16x3 = None, None


gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("wavefront", [1, 0], ids=["wavefront", "one_stream"])
@pytest.mark.parametrize("kind", FORWARD_KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_forward_family_behind_a_gate(case, kind, wavefront, ctx):
    """prepare, the inference forwards, the training forwards and the Monte-Carlo forward, each in a sandwich of its own
    under all five callers: the bits of the synchronised null-stream run"""
    _sweep(ctx, case, kind, wavefront, range(5))


@gpu
@pytest.mark.parametrize("wavefront", [1, 0], ids=["wavefront", "one_stream"])
@pytest.mark.parametrize("kind", HEAVY_KINDS)
@pytest.mark.parametrize("case", list(CASES))
def test_training_step_behind_a_gate(case, kind, wavefront, ctx):
    """forward_train + backward in one sandwich, d_out written between the two: the prediction's bits, and the gradients'
    bits (deterministic) or the gradients within the atomic bound (default) of the synchronised run; workspace and train
    buffer are overwritten right behind the backward"""
    _sweep(ctx, case, kind, wavefront, HEAVY_CALLERS)


@gpu
@pytest.mark.parametrize("wavefront", [1, 0], ids=["wavefront", "one_stream"])
@pytest.mark.parametrize("mode", [1, 2, 3, "train_bf16x3"])
@pytest.mark.parametrize("case", PRECISION_CASES)
def test_precision_modes_behind_a_gate(case, mode, wavefront, ctx):
    """the bf16 copies and planes the precision modes make per call in the workspace (in front of the fork: every chain
    reads them) under the same sandwich: the inference forward and the deterministic training step of modes 1, 2, 3,
    the training step of the three-piece switch"""
    if mode == "train_bf16x3":
        _sweep(ctx, case, "train_backward_det", wavefront, HEAVY_CALLERS, x3=True)
        return
    _sweep(ctx, case, "forward", wavefront, HEAVY_CALLERS, precision=mode)
    _sweep(ctx, case, "train_backward_det", wavefront, HEAVY_CALLERS, precision=mode)


# ---- two further orderings, both behind one gate -------------------------------------------------------------------------
def _pair_of_bindings(ctx):
    a, b = ctx.binding("l2_n33_b3"), ctx.binding("l3_n67_b22")
    for bd in (a, b):
        bd.restore()
    return a, b


ROUNDS, ROUNDS_BEHIND_THE_GATE = 10, 3


@gpu
@pytest.mark.parametrize("caller", [0, 2], ids=["null_stream", "side_stream_2"])
def test_two_bindings_interleaved_on_one_stream(caller, ctx):
    """A.forward, B.forward_train, A.forward_series, B.backward, A.forward_train, B.forward, A.backward - ten rounds with
    nothing but the calls on the stream and no synchronisation anywhere.  The library's streams, its events and its table
    of training modes are per device, not per binding: every result must be that binding's own synchronised result,
    round after round.

    One gate, in front of round 0 - but it cannot hold ten rounds: the HIP runtime keeps a bounded number of commands
    behind a stream that does not advance (stream_gate.COMMANDS_BEHIND_A_SHUT_STREAM), and a round is about 2000
    launches.  Step 6 is therefore taken behind round 3: the first three rounds were enqueued while the stream was shut
    and reach the device as one DAG; the seven behind them follow with nothing between the calls either, at the pace of
    the host.  (Shutting the stream again in front of rounds 3, 6 and 9 was tried: the call that exceeds the bound then
    waits until the NEXT gate has opened too - [True, False, True, True] at every gate length up to the cap.)"""
    a, b = _pair_of_bindings(ctx)
    inputs = a.pair(a.x, a.series, a.d_out, a.h0) + b.pair(b.x, b.d_out)
    bufs = lambda *_: a.buffers(train=True) + b.buffers(train=True)                 # noqa: E731
    late = lambda *_: bufs() + [d for d, _ in inputs]                               # noqa: E731
    gate = SG.Gate("interleaved rounds, %d behind the gate" % ROUNDS_BEHIND_THE_GATE)

    def rounds(n, between=lambda: None, regate=None):
        def call():
            res = {}
            for r in range(n):
                if regate is not None and r == 0:
                    regate()
                    for d, v in inputs:         # the inputs, behind the gate
                        d.copy_(v)
                if regate is not None and r == ROUNDS_BEHIND_THE_GATE:
                    regate.close()              # step 6
                res["%d/A.forward" % r] = a.hp.forward(a.x)
                between()
                res["%d/B.forward_train" % r] = b.hp.forward_train(b.x)
                between()
                res["%d/A.forward_series" % r] = a.hp.forward_series(a.series, a.label, a.rel)
                between()
                res.update({"%d/B.backward/%s" % (r, k): v for k, v in b.hp.backward(b.x, b.d_out, b.state).items()})
                between()
                res["%d/A.forward_train" % r] = a.hp.forward_train(a.x, h0=a.h0)
                between()
                res["%d/B.forward" % r] = b.hp.forward(b.x)
                between()
                res.update({"%d/A.backward/%s" % (r, k): v
                            for k, v in a.hp.backward(a.x, a.d_out, a.state, h0=a.h0).items()})
                between()
            if regate is not None:
                regate.close()
            return res
        return call

    a.hp.deterministic = b.hp.deterministic = True
    lib = a.hp.lib
    try:
        prev = lib.matgcn_set_wavefront(0)
        try:
            want = sandwich(None, inputs, rounds(1, torch.cuda.synchronize), dict, bufs, poison_before=bufs,
                            synchronous=True)
        finally:
            lib.matgcn_set_wavefront(prev)
        assert len(want) > 40 and all(torch.isfinite(v).all() for v in want.values())
        s = ctx.callers[caller]
        sandwich(s, inputs, rounds(ROUNDS), dict, bufs, poison_before=bufs, synchronous=True)      # warm-up
        sandwich(s, inputs, rounds(ROUNDS), dict, bufs, poison_before=bufs, gated=False, gate=gate)
        gate.cover(gate.last_host_ms * ROUNDS_BEHIND_THE_GATE / ROUNDS)   # the host's enqueue time of the gated rounds
        while True:     # the gates are queued by the call itself: the sandwich around it adds none
            regate = SG.Regate(gate, s)
            got = sandwich(s, [], rounds(ROUNDS, regate=regate), dict, late, poison_before=late, gated=False, gate=gate)
            gate.sandwiches += 1
            if all(regate.in_time):
                break
            gate.grow("the gate opened before %d rounds were enqueued" % ROUNDS_BEHIND_THE_GATE)
    finally:
        a.hp.deterministic = b.hp.deterministic = None
    assert regate.in_time == [True]
    assert len(got) == ROUNDS * len(want)
    bad = [k for k, v in got.items() if not bits_equal(v, want["0/" + k.split("/", 1)[1]])]
    assert not bad, bad[:8]


@gpu
@pytest.mark.parametrize("first,second", [(1, 2), (3, 0)], ids=["side_1_to_side_2", "side_3_to_null"])
@pytest.mark.parametrize("what", ["lazy_prepare_then_forward", "forward_train_then_backward"])
def test_one_binding_moved_between_two_caller_streams(what, first, second, ctx):
    """the first call on one caller stream, `second.wait_stream(first)`, the second call on another: nothing may remember
    the first caller - the weight streams of a lazy prepare, the saved activations and the side stream of forward_train
    must be ordered behind the stream that CALLS next"""
    bd = ctx.binding("l3_n67_b22")
    bd.restore()
    hp = bd.hp
    s1 = ctx.callers[first]
    s2 = ctx.callers[second] if ctx.callers[second] is not None else torch.cuda.default_stream()
    s1 = s1 if s1 is not None else torch.cuda.default_stream()

    flat = [False]      # the reference: both calls on the null stream, a synchronisation between them

    def hop(fn):
        if flat[0]:
            torch.cuda.synchronize()
            return fn()
        s2.wait_stream(s1)
        with torch.cuda.stream(s2):
            r = fn()
        s1.wait_stream(s2)      # the sandwich clones and poisons on the first stream
        return r

    if what == "lazy_prepare_then_forward":
        def call():
            hp.prepare()
            return {"out": hop(lambda: hp.forward(bd.x))}
        kw = dict(write_inputs=bd.params() + bd.pair(bd.x), poison_before=lambda *_: bd.buffers(prepared=True),
                  poison_after=lambda *_: bd.buffers())
        lazy = 1
    else:
        def call():
            pred = hp.forward_train(bd.x, dropout=(11, 0, 0.1))
            grads = hop(lambda: hp.backward(bd.x, bd.d_out, bd.state, dropout=(11, 0, 0.1)))
            return dict({"g/" + k: v for k, v in grads.items()}, out=pred)
        kw = dict(write_inputs=bd.pair(bd.x, bd.d_out), poison_before=lambda *_: bd.buffers(train=True),
                  poison_after=lambda *_: bd.buffers(train=True))
        lazy = None
    hp.deterministic = True
    prev_lazy = hp.lib.matgcn_set_lazy_prepare(lazy) if lazy is not None else None
    try:
        prev, flat[0] = hp.lib.matgcn_set_wavefront(0), True
        try:
            want = sandwich(None, call=call, outputs=dict, synchronous=True, **kw)
        finally:
            hp.lib.matgcn_set_wavefront(prev)
            flat[0] = False
        assert all(torch.isfinite(v).all() for v in want.values())
        sandwich(s1, call=call, outputs=dict, synchronous=True, **kw)
        got = sandwich(s1, call=call, outputs=dict, **kw)
    finally:
        hp.deterministic = None
        if prev_lazy is not None:
            hp.lib.matgcn_set_lazy_prepare(prev_lazy)
        bd.restore()
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, bad


# ---- the single-stream families: one sandwich per exported entry point that takes a stream -----------------------------------
# The loss, metric, MC-score, conformal, region, region-loss and optimizer families document "the caller's stream only".
# Their values are held to the numpy references by their own files; this sweep adds only the stream: a side stream, inputs
# written behind the gate, the bits of the synchronised null-stream call.  Shapes: B = 3, out_steps = 3, N = 33, od = 1,
# S = 5 samples, two regions that overlap, three optimizer tensors of 5 / 4097 / 0 elements.
SB, SO, SN, SOD, SS = 3, 3, 33, 1, 5
PROBS = (0.05, 0.5, 0.95)
MEAN, STD = 1.5, 2.0


class Env:
    """the inputs of the sweep: device tensors with a staging copy each (float data), and the index data - region map,
    optimizer tables - uploaded and synchronised here, in front of every gate"""

    def __init__(self, ctx):
        from multistgraph_amd import ops
        from multistgraph_amd.regions import RegionMap
        self.bd = ctx.binding("l2_n33_b3")
        self.bd.restore()
        assert (self.bd.n, self.bd.b) == (SN, SB)
        dev = self.dev = torch.device("cuda:0")
        rng = np.random.default_rng(7)
        self.stage = {}
        pred = rng.standard_normal((SB, SO, SN, SOD))
        y = pred + 0.7 * rng.standard_normal((SB, SO, SN, SOD))
        y[0, 0, :4] = (0.0 - MEAN) / STD          # labels that de-scale to 0: masked by null_val = 0
        self.pred, self.y = self.t(pred), self.t(y)
        self.samples = self.t(pred[None] + 0.5 * rng.standard_normal((SS, SB, SO, SN, SOD)))
        self.regions = RegionMap(SN, groups=[list(range(0, 20)), list(range(15, SN))])
        self.regions.groups_on(dev), self.regions.node_groups_on(dev)
        sizes = (5, 4097, 0)
        self.opt = {k: [self.t(rng.standard_normal(n) * (0.1 if k == "exp_avg_sq" else 1.0)) for n in sizes]
                    for k in ("params", "grads", "exp_avgs", "exp_avg_sqs")}
        for v in self.opt["exp_avg_sqs"]:
            v.abs_()
            self.stage[id(v)].abs_()
        h = self.bd.hp.spec.hidden
        self.xin = self.t(rng.standard_normal((SB, SN, 2)))
        self.xh = self.t(rng.standard_normal((SB, SN, h)))
        self.h = self.t(np.tanh(rng.standard_normal((SB, SN, h))))
        self.x0 = self.t(rng.standard_normal((SB, 24, SN, 2)))
        self.seq = self.t(np.tanh(rng.standard_normal((SB, 24, SN, h))))
        # matgcn_debug_gemm: M, N, K = 17, 19, 23 inside padded blocks, strides as test_backward_gpu.py lays them out
        self.ga, self.gb, self.gc = (self.t(rng.standard_normal(s)) for s in (17 * 25 + 8, 23 * 23 + 8, 17 * 21 + 1))
        # inputs that are another entry point's output: made here, synchronously
        torch.cuda.synchronize()
        self.sums = self.t(ops.metric_sums(self.pred, self.y), np.float64)
        self.sums_nodes = self.t(ops.metric_sums_nodes(self.pred, self.y), np.float64)
        self.scores = self.t(ops.mc_conformity(self.samples, self.y, PROBS))
        self.margin = self.t(ops.conformal_quantile(self.scores, SB, "horizon", 0.9)[0])
        self.norm = self.t(ops.grad_norm(self.opt["grads"]).reshape(1))
        torch.cuda.synchronize()

    def t(self, a, dtype=np.float32):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        d = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(self.dev)
        self.stage[id(d)] = d.clone()
        return d

    def pair(self, *tensors):
        return [(t, self.stage[id(t)]) for t in tensors]


def _grad_of(loss_fn, pred):
    """the gradient entry point behind a loss's autograd function: d loss / d pred on a leaf that shares pred's memory"""
    leaf = pred.detach().requires_grad_()
    loss_fn(leaf).backward()
    return {"d_pred": leaf.grad}


def _single(inputs, call, outputs=None, workspace=False):
    return dict(inputs=inputs, call=call, outputs=outputs or (lambda r: {"result": r}), workspace=workspace)


def _loss_cases():
    from multistgraph_amd.ops import TRAIN_LOSSES
    return sorted(TRAIN_LOSSES)


def _build_single(e, name, variant):
    """(inputs, call, outputs) of the sandwich of entry point ``name``"""
    from multistgraph_amd import ops
    hp = e.bd.hp
    lab = e.pair(e.pred, e.y)
    mc = e.pair(e.samples, e.y)
    table = {
        "matgcn_masked_mae": lambda: _single(lab, lambda: ops.masked_mae_device(e.pred, e.y, 0, MEAN, STD, 0.0)),
        "matgcn_masked_mae_grad": lambda: _single(lab, lambda: _grad_of(
            lambda p: ops.masked_mae_loss(p, e.y, 0, MEAN, STD, 0.0), e.pred), dict),
        "matgcn_loss": lambda: _single(lab, lambda: ops.train_loss_device(e.pred, e.y, 0, MEAN, STD, variant)),
        "matgcn_loss_grad": lambda: _single(lab, lambda: _grad_of(
            lambda p: ops.train_loss(p, e.y, 0, MEAN, STD, variant), e.pred), dict),
        "matgcn_metric_sums": lambda: _single(lab, lambda: ops.metric_sums(e.pred, e.y)),
        "matgcn_metric_table": lambda: _single(e.pair(e.sums), lambda: ops.metric_table(e.sums)),
        "matgcn_metric_table_rows": lambda: _single(e.pair(e.sums_nodes), lambda: ops.metric_table_rows(e.sums_nodes, SO)),
        "matgcn_metric_sums_nodes": lambda: _single(lab, lambda: ops.metric_sums_nodes(e.pred, e.y)),
        "matgcn_mc_quantiles": lambda: _single(e.pair(e.samples), lambda: ops.mc_quantiles(e.samples, PROBS, MEAN, STD)),
        "matgcn_mc_quantiles_scaled": lambda: _single(e.pair(e.samples),
                                                      lambda: ops.mc_quantiles_scaled(e.samples, PROBS, clamp_min=-0.5)),
        "matgcn_mc_scores": lambda: _single(mc, lambda: ops.mc_scores(e.samples, e.y, PROBS, 0, MEAN, STD)),
        "matgcn_mc_scores_nodes": lambda: _single(mc, lambda: ops.mc_scores_nodes(e.samples, e.y, PROBS)),
        "matgcn_mc_conformity": lambda: _single(mc, lambda: ops.mc_conformity(e.samples, e.y, PROBS)),
        "matgcn_conformal_quantile": lambda: _single(
            e.pair(e.scores), lambda: ops.conformal_quantile(e.scores, SB, variant, 0.9),
            lambda r: {"margin": r[0], "count": r[1]}),
        "matgcn_conformal_coverage": lambda: _single(
            e.pair(e.scores, e.margin), lambda: ops.conformal_coverage(e.scores, SB, "horizon", e.margin)),
        "matgcn_group_sums": lambda: _single(e.pair(e.pred), lambda: ops.group_sums(e.pred, e.regions)),
        "matgcn_group_label_sums": lambda: _single(e.pair(e.y), lambda: ops.group_label_sums(e.y, e.regions, SO, SOD)),
        "matgcn_region_loss": lambda: _single(lab, lambda: ops.region_loss_device(e.pred, e.y, e.regions, 0, MEAN, STD,
                                                                                  "mae")),
        "matgcn_region_loss_grad": lambda: _single(lab, lambda: _grad_of(
            lambda p: ops.region_train_loss(p, e.y, e.regions, 0, MEAN, STD, "mse"), e.pred), dict),
        "matgcn_grad_norm": lambda: _single(e.pair(*e.opt["grads"]), lambda: ops.grad_norm(e.opt["grads"])),
        "matgcn_adam_step": lambda: _single(
            e.pair(e.norm, *[t for k in e.opt for t in e.opt[k]]),
            lambda: ops.adam_step(e.opt["params"], e.opt["grads"], e.opt["exp_avgs"], e.opt["exp_avg_sqs"], lr=1e-2,
                                  betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, step=3, max_norm=0.5,
                                  total_norm=e.norm.reshape(())),
            lambda r: {"%s%d" % (k, i): t for k in ("params", "exp_avgs", "exp_avg_sqs") for i, t in enumerate(e.opt[k])}),
        "matgcn_dropout_mask": lambda: _single([], lambda: hp.dropout_mask(11, 3, 0.1)),
        "matgcn_fuse_heads": lambda: _single(e.bd.pair(e.bd.x), lambda: hp.fuse_heads(e.bd.x), workspace=True),
        "matgcn_agcn_gate_fwd": lambda: _single(e.pair(e.xin, e.h), lambda: hp.agcn_gate(0, e.xin, e.h), workspace=True),
        "matgcn_atgru_cell_fwd": lambda: _single(e.pair(e.xh, e.h), lambda: hp.atgru_cell(1, e.xh, e.h), workspace=True),
        "matgcn_res_cell_fwd": lambda: _single(e.pair(e.xin, e.h), lambda: hp.res_cell(0, e.xin, e.h), workspace=True),
        "matgcn_encoder_fwd": lambda: _single(e.pair(e.x0), lambda: hp.encoder(e.x0),
                                              lambda r: {"seq": r[0], "finals": r[1]}, workspace=True),
        "matgcn_output_head": lambda: _single(e.pair(e.seq), lambda: hp.output_head(e.seq), workspace=True),
        "matgcn_debug_gemm": lambda: _single(
            e.pair(e.ga, e.gb, e.gc),
            lambda: ops.debug_gemm(e.ga, e.gb, e.gc, (17, 19, 23, 1, 25, 1, 0, 23, 1, 0, 21, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1),
                                   alpha=1.25, beta=0.5),
            lambda r: {"c": e.gc}),
    }
    return table[name]()


# entry point -> the variants swept (None: one sandwich)
SWEPT = {
    "matgcn_masked_mae": None, "matgcn_masked_mae_grad": None,
    "matgcn_loss": "losses", "matgcn_loss_grad": "losses",
    "matgcn_metric_sums": None, "matgcn_metric_table": None, "matgcn_metric_table_rows": None,
    "matgcn_metric_sums_nodes": None,
    "matgcn_mc_quantiles": None, "matgcn_mc_quantiles_scaled": None, "matgcn_mc_scores": None,
    "matgcn_mc_scores_nodes": None,
    "matgcn_mc_conformity": None, "matgcn_conformal_quantile": ("horizon", "element"), "matgcn_conformal_coverage": None,
    "matgcn_group_sums": None, "matgcn_group_label_sums": None, "matgcn_region_loss": None,
    "matgcn_region_loss_grad": None,
    "matgcn_grad_norm": None, "matgcn_adam_step": None,
    "matgcn_dropout_mask": None, "matgcn_fuse_heads": None, "matgcn_agcn_gate_fwd": None, "matgcn_atgru_cell_fwd": None,
    "matgcn_res_cell_fwd": None, "matgcn_encoder_fwd": None, "matgcn_output_head": None, "matgcn_debug_gemm": None,
}
# entry points that take a stream and are NOT in the sweep, each with the place that covers it
_BINDING = "forks onto the library's streams: the binding sandwiches above (test_forward_family_behind_a_gate, " \
           "test_training_step_behind_a_gate) cover it under five callers"
EXCUSED = {
    "matgcn_prepare": _BINDING, "matgcn_prepare_join": _BINDING, "matgcn_forward": _BINDING,
    "matgcn_forward_series": _BINDING, "matgcn_forward_mc": _BINDING, "matgcn_forward_train": _BINDING,
    "matgcn_forward_train_seeded": _BINDING, "matgcn_backward": _BINDING, "matgcn_backward_seeded": _BINDING,
}
LOSS_NAMES = ("logcosh", "huber", "mae", "mape", "masked_mae", "masked_mape", "masked_mse", "masked_rmse", "mse", "quantile",
              "rmse")
SINGLE = [(n, v) for n, vs in SWEPT.items() for v in (LOSS_NAMES if vs == "losses" else vs or (None,))]


def test_every_entry_point_with_a_stream_is_swept_or_excused():
    """the table of swept names is the set of functions in the binding's signature table whose last argument is the
    stream, minus the excused ones: an entry point added later joins the sweep or is excused in writing"""
    from multistgraph_amd import _lib
    from multistgraph_amd.ops import TRAIN_LOSSES
    with_stream = {n for n, (_, args) in _lib._SIGNATURES.items() if args and args[-1] is C.c_void_p}
    assert len(with_stream) > 30
    assert not set(SWEPT) & set(EXCUSED)
    assert set(SWEPT) | set(EXCUSED) == with_stream, sorted(with_stream ^ (set(SWEPT) | set(EXCUSED)))
    assert all(isinstance(r, str) and len(r) > 20 for r in EXCUSED.values())
    assert sorted(LOSS_NAMES) == sorted(TRAIN_LOSSES) and len(LOSS_NAMES) == 11
    # the entry points that wait for the device by design take no stream - nothing to order - and stay out of sandwiches
    assert set(SG.KNOWN_HOST_SYNCS) <= set(_lib._SIGNATURES) and not set(SG.KNOWN_HOST_SYNCS) & with_stream


@pytest.fixture(scope="module")
def env(ctx):
    return Env(ctx)


@gpu
@pytest.mark.parametrize("name,variant", SINGLE, ids=["%s[%s]" % (n, v) if v else n for n, v in SINGLE])
def test_single_stream_entry_point_behind_a_gate(name, variant, env, ctx):
    """one entry point of the "caller's stream only" families on a side stream, its inputs written behind the gate: the
    bits of its own synchronised null-stream call (a launch on another stream reads the NaN the inputs held before)"""
    sp = _build_single(env, name, variant)
    bufs = (lambda *_: env.bd.buffers()) if sp["workspace"] else ()
    args = (sp["inputs"], sp["call"], sp["outputs"], bufs)
    want = sandwich(None, *args, poison_before=bufs, synchronous=True)
    assert want
    side = ctx.callers[2]
    sandwich(side, *args, poison_before=bufs, synchronous=True)
    got = sandwich(side, *args, poison_before=bufs)
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, bad


# ---- through the model ---------------------------------------------------------------------------------------------------
TRAIN_STEPS = 5
STEPS_PER_GATE = 5      # five training steps of the tiny model stay below stream_gate.COMMANDS_BEHIND_A_SHUT_STREAM


class Trainee:
    """the tiny golden case as test_optim_gpu._train trains it (device dropout, deterministic backward, ClipAdam with the
    global-norm clip), with everything a run changes - parameters, moments, step counts, the dropout counter - put back
    from staging copies, so that one model serves the warm-up, the reference and the gated run"""

    def __init__(self, regions):
        from helpers import Case
        from multistgraph_amd.model import MultiATGCN
        from multistgraph_amd.optim import ClipAdam
        from multistgraph_amd.regions import RegionMap
        c = self.case = Case("tiny_multi_uni_c2")
        dev = torch.device("cuda:0")
        torch.manual_seed(77)       # the device dropout draws from (torch.initial_seed(), the model's own counter)
        m = self.model = MultiATGCN(dict(c.config("cuda:0"), hip_dropout="device", hip_deterministic=True),
                                    c.data_feature).to(dev)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
        m.train()
        self.opt = ClipAdam(m.parameters(), max_grad_norm=5)
        self.regions = RegionMap(c.n, groups=[list(range(0, c.n // 2 + 2)), list(range(c.n // 2 - 2, c.n))]) if regions else None
        if self.regions is not None:
            self.regions.groups_on(dev), self.regions.node_groups_on(dev)
        self.x, self.y = torch.from_numpy(c.x).to(dev), torch.from_numpy(c.y).to(dev)
        self.batch = {"X": self.x, "y": self.y}
        self.params = [p for p in m.parameters()]
        torch.cuda.synchronize()
        self.x_stage, self.y_stage = self.x.clone(), self.y.clone()
        self.param_stage = [p.data.clone() for p in self.params]
        self.counter = m._dropout_counter
        self.steps(1)               # the optimizer's state tensors, the binding and its buffers exist from here on
        torch.cuda.synchronize()

    def inputs(self):
        """(destination, staging): batch and parameters from their copies, the moments from zeros"""
        pairs = [(self.x, self.x_stage), (self.y, self.y_stage)]
        pairs += [(p.data, v) for p, v in zip(self.params, self.param_stage)]
        return pairs + [(mom, torch.zeros_like(mom)) for mom in self.moments()]

    def reset(self):
        """host-side state of a fresh run; the device side comes back through ``inputs``"""
        m = self.model
        m._dropout_counter = self.counter
        m._prepared_key = None          # the parameters are about to be rewritten behind the model's back
        for p in self.params:
            st = self.opt.state.get(p)
            if st:
                st["step"].fill_(0.0)
            p.grad = None

    def moments(self):
        return [self.opt.state[p][k] for p in self.params if self.opt.state.get(p) for k in ("exp_avg", "exp_avg_sq")]

    def buffers(self, *_):
        out = []
        for hp in self.model._paths.values():
            out += [hp.workspace, hp._train]
        return out

    def loss(self):
        if self.regions is None:
            return self.model.calculate_loss(self.batch)
        return self.model.train_loss(self.batch, "masked_mae", regions=self.regions)

    def steps(self, n, between=lambda: None, regate=None, late=None):
        for i in range(n):
            if regate is not None and i % STEPS_PER_GATE == 0:
                regate()
                if i == 0:
                    late()
            self.opt.zero_grad()
            self.loss().backward()
            between()
            self.opt.step()
            between()
        if regate is not None:
            regate.close()

    def result(self, *_):
        return {k: p.data for k, p in self.model.named_parameters()}


@gpu
@pytest.mark.parametrize("regions", [False, True], ids=["calculate_loss", "train_loss_regions"])
def test_five_training_steps_behind_one_gate(regions, ctx):
    """five steps of MultiATGCN + ClipAdam with nothing read back between them, all enqueued behind one gate on a side
    stream: the parameters' bits of the null-stream run that synchronises after every step.  The in-place Adam write
    must not reach a straggling reader of the parameters (the weight-gradient stream, a lazy prepare), and the next
    prepare must see the new parameters"""
    t = Trainee(regions)
    inputs = t.inputs()
    assert len(inputs) == 2 + 3 * len(t.params)
    late = lambda *_: t.buffers() + [d for d, _ in inputs]                          # noqa: E731

    def run(stream, steps=None, **kw):
        t.reset()
        return sandwich(stream, inputs, lambda: t.steps(TRAIN_STEPS, **(steps or {})), t.result, t.buffers,
                        poison_before=t.buffers, **kw)

    want = run(None, synchronous=True, steps=dict(between=torch.cuda.synchronize))
    moved = sum(int(not bits_equal(want[k], v)) for (k, _), v in zip(t.model.named_parameters(), t.param_stage))
    assert moved > 10 and all(torch.isfinite(v).all() for v in want.values())
    side = ctx.callers[2]
    run(side, synchronous=True)                                  # warm-up on the side stream
    gate = SG.Gate("five training steps")
    run(side, gated=False, gate=gate)                            # the host's enqueue time
    gate.cover(gate.last_host_ms * min(STEPS_PER_GATE, TRAIN_STEPS) / TRAIN_STEPS)
    while True:
        regate = SG.Regate(gate, side)
        t.reset()
        copy_in = lambda: [d.copy_(v) for d, v in inputs]                           # noqa: E731
        got = sandwich(side, [], lambda: t.steps(TRAIN_STEPS, regate=regate, late=copy_in), t.result, late,
                       poison_before=late, gated=False, gate=gate)
        gate.sandwiches += 1
        if all(regate.in_time):
            break
        gate.grow("gates still shut behind their steps: %s" % regate.in_time)
    assert len(regate.in_time) == (TRAIN_STEPS + STEPS_PER_GATE - 1) // STEPS_PER_GATE
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, bad


def _eval_model(c):
    from multistgraph_amd.model import MultiATGCN
    m = MultiATGCN(c.config("cuda:0"), c.data_feature).to(torch.device("cuda:0")).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c.state.items()})
    return m


class Evaluation:
    """the tiny golden case in eval mode and three batches of it, staged"""

    def __init__(self):
        from helpers import Case
        c = self.case = Case("tiny_multi_uni_c2")
        self.model = _eval_model(c)
        dev = torch.device("cuda:0")
        self.batches = [{"X": torch.from_numpy(c.x * (1.0 + 0.25 * i)).float().to(dev),
                         "y": torch.from_numpy(c.y + 0.5 * i).float().to(dev)} for i in range(3)]
        torch.cuda.synchronize()
        self.inputs = [(t, t.clone()) for b in self.batches for t in (b["X"], b["y"])]
        with torch.no_grad():
            self.model.predict(self.batches[0])       # the binding, its buffers and the prepare
        torch.cuda.synchronize()

    def buffers(self, *_):
        return [hp.workspace for hp in self.model._paths.values()]


@pytest.fixture(scope="module")
def evaluation(lib_built):
    return Evaluation()


@gpu
def test_interval_and_calibrator_behind_a_gate(evaluation, ctx):
    """predict_interval with a fitted ConformalCalibrator (the Monte-Carlo forward, the quantiles, apply) on a side
    stream behind the gate: mean, std and the calibrated band of the synchronised null-stream call"""
    from multistgraph_amd.evaluator import ConformalCalibrator
    e, levels = evaluation, (0.25, 0.5, 0.75)
    m = e.model
    cal = ConformalCalibrator({}, probs=levels, grouping="element")
    m.calibrate_mc(e.batches[1], cal, samples=8, seed=11)
    cal.fit()
    torch.cuda.synchronize()
    inputs = e.inputs[:2]

    def call():
        return m.predict_interval(e.batches[0], samples=8, probs=levels, seed=11, calibrator=cal)
    args = (inputs, call, lambda r: dict(zip(("mean", "std", "band"), r)), e.buffers)
    want = sandwich(None, *args, poison_before=e.buffers, synchronous=True)
    assert all(torch.isfinite(v).all() for v in want.values())
    side = ctx.callers[2]
    sandwich(side, *args, poison_before=e.buffers, synchronous=True)
    got = sandwich(side, *args, poison_before=e.buffers)
    bad = [k for k in want if not bits_equal(got[k], want[k])]
    assert not bad, bad


@gpu
@pytest.mark.parametrize("kind", ["device", "node", "region"])
def test_one_evaluator_pass_behind_one_gate(kind, evaluation, ctx):
    """one pass of DeviceEvaluator / NodeEvaluator / RegionEvaluator over three batches, every batch enqueued behind one
    gate on a side stream - a per-batch upload of the scaler's numbers would make the host wait for the device here -,
    the ``.cpu()`` that ends the pass behind the gate check: the sums and the table of the synchronised pass"""
    from multistgraph_amd.evaluator import DeviceEvaluator, NodeEvaluator, RegionEvaluator
    from multistgraph_amd.regions import RegionMap
    e = evaluation
    m, n = e.model, e.case.n
    regions = RegionMap(n, groups=[list(range(0, n // 2 + 2)), list(range(n // 2 - 2, n))])
    regions.groups_on(torch.device("cuda:0"))
    cfg = {"metrics": ["MAE", "RMSE", "masked_MAPE", "R2"]}
    make = {"device": lambda: DeviceEvaluator(cfg, streaming=True), "node": lambda: NodeEvaluator(cfg),
            "region": lambda: RegionEvaluator(cfg, regions)}[kind]
    table = {"device": lambda ev: ev.table(), "node": lambda ev: ev.node_table(), "region": lambda ev: ev.node_table()}[kind]
    made = []

    def call():
        ev = make()
        made.append(ev)
        with torch.no_grad():
            for b in e.batches:
                m.collect_metrics(ev, b)
        return ev

    def sums(ev):
        return {"sums": ev._sums if kind == "device" else ev._metric_sums}
    args = (e.inputs, call, sums, e.buffers)
    want = sandwich(None, *args, poison_before=e.buffers, synchronous=True)
    want_table = table(made[-1])
    assert torch.isfinite(want["sums"]).all() and float(want["sums"].abs().sum()) > 0.0
    side = ctx.callers[2]
    sandwich(side, *args, poison_before=e.buffers, synchronous=True)
    got = sandwich(side, *args, poison_before=e.buffers)
    assert bits_equal(got["sums"], want["sums"])
    assert bits_equal(table(made[-1]), want_table)


# ---- own-pool mode: matgcn_set_stream_pool(1) must precede stream creation, so every mode gets a process of its own -------------
POOL_CASE = "l3_n67_b22"
POOL_KINDS = ["forward", "forward_h0", "forward_series", "forward_train_seeded", "train_backward_det"]
POOL_CALLERS = (0, 2)
CHILD_SECONDS = 120.0


def _pool_child(rank, pool, out_dir):
    """one process = one stream mode: the sandwiches of POOL_CASE under two callers, results into an .npz, one line per
    gate check into a text file"""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from multistgraph_amd import _lib
    torch.cuda.set_device(0)
    lib = _lib.load()
    assert lib.matgcn_set_stream_pool(pool) == 0           # before any stream of the library exists
    c = Ctx()
    bd = c.binding(POOL_CASE)
    out, lines = {}, []
    for kind in POOL_KINDS:
        for k, v in bd.reference(kind).items():
            out["ref/%s/%s" % (kind, k)] = v.cpu().numpy()
        for i in POOL_CALLERS:
            bd.run(kind, c.callers[i], synchronous=True)
            before = SG.GATE.sandwiches
            got = bd.run(kind, c.callers[i])               # raises when no gate up to the cap stays shut
            lines.append("pool %d caller %d %s: shut when enqueued, gate %.0f ms, %d attempt(s)"
                         % (pool, i, kind, SG.GATE.ms, SG.GATE.sandwiches - before))
            for k, v in got.items():
                out["caller%d/%s/%s" % (i, kind, k)] = v.cpu().numpy()
    assert lib.matgcn_set_stream_pool(pool) == 0           # still the mode in use
    np.savez(os.path.join(out_dir, "pool%d.npz" % pool), **out)
    with open(os.path.join(out_dir, "pool%d.txt" % pool), "w") as fh:
        fh.write("\n".join(lines) + "\n")


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@gpu
def test_own_stream_pool_keeps_the_callers_order(tmp_path):
    """the hot entry points on the library's `main` stream (forked from and joined back into the caller's): the same
    sandwiches in a child of each mode, one child at a time, each under its own time limit.  Within a mode every caller
    gives the synchronised run's bits (deterministic gradients included); across the modes the forwards agree bit for
    bit and the gradients within 2e-6 x scale, as test_sharding.py has it"""
    import torch.multiprocessing as mp
    for pool in (0, 1):
        child = mp.spawn(_pool_child, args=(pool, str(tmp_path)), nprocs=1, join=False)
        done = child.join(timeout=CHILD_SECONDS)
        if not done:
            for p in child.processes:
                p.kill()
            raise AssertionError("the child of stream mode %d did not finish within %.0f s" % (pool, CHILD_SECONDS))
    res = [np.load(tmp_path / ("pool%d.npz" % pool)) for pool in (0, 1)]
    checks = [(tmp_path / ("pool%d.txt" % pool)).read_text().splitlines() for pool in (0, 1)]
    for pool in (0, 1):
        print("\n".join(checks[pool]))
        assert len(checks[pool]) == len(POOL_KINDS) * len(POOL_CALLERS)
        assert all("shut when enqueued" in line for line in checks[pool])
    assert sorted(res[0].files) == sorted(res[1].files) and len(res[0].files) > 40
    for pool in (0, 1):         # within a mode: bit for bit against its own synchronised run
        for k in res[pool].files:
            if not k.startswith("ref/"):
                assert _same_bits(res[pool][k], res[pool]["ref/" + k.split("/", 1)[1]]), (pool, k)
    for k in res[0].files:      # across the modes
        a, b = res[0][k], res[1][k]
        if "/g/" in k:
            scale = float(np.abs(a).max()) + 1e-30
            assert float(np.abs(a.astype(np.float64) - b).max()) <= ATOMIC_TOL * scale, k
        else:
            assert _same_bits(a, b), k
