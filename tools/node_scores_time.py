"""The per-node reductions at a bench workload's output shape (default Baltimore 403, B = 64, out = 24): matgcn_metric_sums_nodes,
matgcn_mc_scores_nodes and matgcn_mc_quantiles_scaled on the re-transformed scale (scaler, per-tract affine, clamp at 0,
truth filter), next to their per-horizon siblings in the same process and to a torch route - torch.sort over the sample axis,
the same terms in torch, index_add_ per (horizon, node); HIP events, median over the repetitions after the first three.
Prints one JSON line per measurement.  The inputs are synthetic: the kernels' time depends on the shape alone.
usage: node_scores_time.py [workload] [reps] [S ...]     (default: bm403 20 32 128)"""
import json, math, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import build, ops
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sizes = [int(v) for v in sys.argv[3:]] or [32, 128]
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
PROBS = (0.05, 0.5, 0.95)
MEAN, STD, S_SMALL = 14.41, 29.3, 6.0
B, OUT, N = w["batch"], w["out"], w["nodes"]
shape = (B, OUT, N, 1)


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for _ in range(reps + 3):
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        ms.append(ev[0].elapsed_time(ev[1]))
    return statistics.median(ms[3:])


def report(what, s, ms, **more):
    print(json.dumps(dict(workload=name, batch=B, out=OUT, nodes=N, samples=s, what=what, ms=round(ms, 4), reps=reps,
                          source=build.source_id(), **more)), flush=True)


gen = torch.Generator(device=dev).manual_seed(0)
y = torch.randn(shape, generator=gen, device=dev)
pred = y + 0.3 * torch.randn(shape, generator=gen, device=dev)
gm = 20.0 * torch.rand(N, generator=gen, device=dev)
gs = 0.5 + torch.rand(N, generator=gen, device=dev)
rows = (torch.arange(OUT, device=dev)[:, None] * N + torch.arange(N, device=dev)[None, :]).expand(B, OUT, N).reshape(-1)
mean_t, std_t = torch.tensor([MEAN], device=dev), torch.tensor([STD], device=dev)      # no upload inside the timed calls
scale = dict(mean=mean_t, std=std_t, group_mean=gm, group_std=gs, clamp_min=0.0, truth_min=S_SMALL, min_s=-1.0)


def retransform(x):
    return (x * STD + MEAN) * gs[:, None] + gm[:, None]


def torch_metric_nodes():
    l, p = retransform(y), retransform(pred).clamp_min(0.0)
    keep = (l > S_SMALL).double()
    d = (p - l).double()
    terms = torch.stack([keep, d.abs() * keep, d * d * keep, (d / l).abs() * keep, l * keep, l * l * keep, p * keep, p * p * keep], -1)
    return torch.zeros(OUT * N, terms.shape[-1], dtype=torch.float64, device=dev).index_add_(0, rows, terms.reshape(B * OUT * N, -1))


def torch_scores_nodes(samples):
    s = samples.shape[0]
    xs = torch.sort(retransform(samples).clamp_min(0.0), dim=0).values
    l = retransform(y)
    q = []
    for level in PROBS:
        h = float(torch.tensor(level, dtype=torch.float32)) * (s - 1)
        j = int(math.floor(h))
        lo, hi = xs[j], xs[min(j + 1, s - 1)]
        q.append(lo + (h - j) * (hi - lo))
    coef = (2.0 * torch.arange(s, device=dev, dtype=torch.float64) - s + 1.0).reshape(s, 1, 1, 1, 1)
    xd, ld = xs.double(), l.double()
    crps = (xd - ld[None]).abs().sum(0) / s - (coef * xd).sum(0) / (s * s)
    keep = (l > S_SMALL).double()
    width = (q[-1] - q[0]).double()
    c = 2.0 / (1.0 - (PROBS[-1] - PROBS[0]))
    wink = width + c * (q[0] - l).clamp_min(0).double() + c * (l - q[-1]).clamp_min(0).double()
    terms = [keep, crps * keep, ((q[0] <= l) & (l <= q[-1])).double() * keep, width * keep, wink * keep]
    terms += [torch.maximum(lv * (ld - qq.double()), (lv - 1.0) * (ld - qq.double())) * keep for lv, qq in zip(PROBS, q)]
    terms = torch.stack(terms, -1)
    return torch.zeros(OUT * N, terms.shape[-1], dtype=torch.float64, device=dev).index_add_(0, rows, terms.reshape(B * OUT * N, -1))


differ = float((ops.metric_sums_nodes(pred, y, **scale)[..., 0].reshape(-1) - torch_metric_nodes()[:, 0]).abs().sum())
report("matgcn_metric_sums_nodes", 0, timed(lambda: ops.metric_sums_nodes(pred, y, **scale)), counts_differing_from_torch=differ)
report("matgcn_metric_sums (per horizon)", 0, timed(lambda: ops.metric_sums(pred, y, **scale)))
report("torch terms + index_add_ (metric sums per node)", 0, timed(torch_metric_nodes))
for s in sizes:
    samples = torch.randn((s,) + shape, generator=gen, device=dev)
    mb = samples.numel() * 4 / 1e6
    got, ref = ops.mc_scores_nodes(samples, y, PROBS, null_val=float("nan"), **scale), torch_scores_nodes(samples)
    worst = float((got.reshape(ref.shape)[:, 1] - ref[:, 1]).abs().max())
    report("matgcn_mc_scores_nodes", s, timed(lambda: ops.mc_scores_nodes(samples, y, PROBS, null_val=float("nan"), **scale)),
           sample_mb=round(mb, 1), crps_sum_against_torch=worst)
    report("matgcn_mc_scores (per horizon)", s, timed(lambda: ops.mc_scores(samples, y, PROBS, mean=MEAN, std=STD)), sample_mb=round(mb, 1))
    report("torch.sort + terms + index_add_ (scores per node)", s, timed(lambda: torch_scores_nodes(samples)), sample_mb=round(mb, 1))
    qs = {k: v for k, v in scale.items() if k not in ("truth_min", "min_s")}
    report("matgcn_mc_quantiles_scaled", s, timed(lambda: ops.mc_quantiles_scaled(samples, PROBS, **qs)), sample_mb=round(mb, 1))
    report("matgcn_mc_quantiles (scalar affine)", s, timed(lambda: ops.mc_quantiles(samples, PROBS, MEAN, STD)), sample_mb=round(mb, 1))
    report("one read (samples.sum(0))", s, timed(lambda: samples.sum(0)), sample_mb=round(mb, 1))
    del samples, got, ref
