"""Region totals at a bench workload's output shape (default Baltimore 403, B = 64, out = 24), S = 32 and 128 samples, on the
re-transformed scale (scaler, per-tract affine, clamp at 0).  Two maps: ten roughly equal regions, and the same plus one
whole-city group.  Routes per map and S:
  matgcn_group_sums                     one read of the samples, members added in the map's order in fp64
  torch de-scale + clamp + index_add_   a temporary of the samples' size, float atomics: another order every run
  torch de-scale + clamp + matmul       the same temporary, a dense (N, G) membership matrix, fp32 sums in the GEMM's order
  one read (samples.sum(0))             the floor: what reading the samples once costs
Then the whole model.predict_interval(..., regions=) next to the node-level call of the same model and S.
Protocol: one process; the routes of a group alternate three times, each visit the median of `reps` calls after three
warm-up calls, HIP events; reported per route: the median of its three visits and their spread (max - min).  A route
counts as faster than the baseline when the gap exceeds twice the spread of the torch route's three visits (the larger of
the torch route's and its own), otherwise "level".  One JSON line per route; the inputs are synthetic: the kernel's time
depends on the shape and the map alone.
Measured (MI355X, bm403 20 32 128, profiles/region_times.jsonl; ms, spread of the three visits in brackets):
  S = 32 (79 MB), ten regions:    matgcn_group_sums 0.078 (0.002), matmul 0.146 (0.001), index_add_ 1.616 (0.008), one read 0.019
  S = 32, ten + the whole city:   0.124 (0.003), 0.145 (0.002), 3.113 (0.010), 0.019
  S = 128 (317 MB), ten regions:  0.248 (0.002), 0.614 (0.005), 5.790 (0.018), 0.057
  S = 128, ten + the whole city:  0.396 (0.003), 0.614 (0.003), 11.905 (0.023), 0.056
  The kernel is faster than the matmul route in all four (gaps 0.021 .. 0.365 ms against bars of at most 0.009 ms) and 4.1 to
  4.4 times the plain read with ten regions, 6.5 to 7.0 times with the whole-city chain beside them: it is not at memory speed.
  index_add_ did not repeat its own bits from one call to the next; the kernel did.
  predict_interval(regions=) against the node-level call: 8.98 / 9.08 against 8.98 ms at S = 32 (level), 17.15 / 17.22 against
  17.44 ms at S = 128 (faster by more than the bar with ten regions, level with the city group).
  DESIGN.md section 5d.2.
usage: region_time.py [workload] [reps] [S ...]     (default: bm403 20 32 128)"""
import json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import build, ops
from multistgraph_amd import synthetic as syn
from multistgraph_amd.regions import RegionMap
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sizes = [int(v) for v in sys.argv[3:]] or [32, 128]
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
PROBS = (0.05, 0.5, 0.95)
MEAN, STD = 14.41, 29.3
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


def compare(routes, baseline, **more):
    """routes: [(label, fn)], alternated three times; one JSON line each, with its verdict against ``baseline``"""
    visits = {label: [] for label, _ in routes}
    for _ in range(3):
        for label, fn in routes:
            visits[label].append(timed(fn))
    med = {k: statistics.median(v) for k, v in visits.items()}
    spread = {k: max(v) - min(v) for k, v in visits.items()}
    for label, _ in routes:
        bar = 2.0 * max(spread[label], spread[baseline])
        gap = med[baseline] - med[label]
        verdict = "baseline" if label == baseline else ("faster" if gap > bar else "slower" if -gap > bar else "level")
        print(json.dumps(dict(workload=name, batch=B, out=OUT, nodes=N, what=label, ms=round(med[label], 4),
                              spread_ms=round(spread[label], 4), against=baseline, verdict=verdict, reps=reps,
                              source=build.source_id(), **more)), flush=True)
    return med


gen = torch.Generator(device=dev).manual_seed(0)
gm = 20.0 * torch.rand(N, generator=gen, device=dev)
gs = 0.5 + torch.rand(N, generator=gen, device=dev)
mean_t, std_t = torch.tensor([MEAN], device=dev), torch.tensor([STD], device=dev)      # no upload inside the timed calls
scale = dict(mean=mean_t, std=std_t, group_mean=gm, group_std=gs, clamp_min=0.0)
ten = [list(range(g * N // 10, (g + 1) * N // 10)) for g in range(10)]
MAPS = {"ten regions": RegionMap(N, groups=ten), "ten regions + the whole city": RegionMap(N, groups=ten + [list(range(N))])}


def retransform(x):
    return ((x * STD + MEAN) * gs[:, None] + gm[:, None]).clamp_min(0.0)


for s in sizes:
    samples = torch.randn((s,) + shape, generator=gen, device=dev)
    mb = round(samples.numel() * 4 / 1e6, 1)
    for label, rm in MAPS.items():
        g = rm.num_groups
        index = torch.tensor(rm.node, device=dev)
        owner = torch.repeat_interleave(torch.arange(g, device=dev), torch.tensor([len(rm.members(k)) for k in range(g)],
                                                                                  device=dev))
        dense = torch.zeros(N, g, device=dev)
        dense.index_put_((index, owner), torch.ones(index.numel(), device=dev), accumulate=True)
        out = torch.empty((s, B, OUT, g, 1), device=dev)

        def by_index_add():
            v = retransform(samples).reshape(-1, N)
            return torch.zeros(v.shape[0], g, device=dev).index_add_(1, owner, v[:, index])

        def by_matmul():
            return retransform(samples).reshape(-1, N) @ dense

        got = ops.group_sums(samples, rm, **scale).reshape(-1, g)
        ref = by_matmul()
        worst = float(((got - ref).abs() / ref.abs().clamp_min(1.0)).max())
        repeat = bool(torch.equal(got, ops.group_sums(samples, rm, **scale).reshape(-1, g)))
        atomics_repeat = bool(torch.equal(by_index_add(), by_index_add()))
        med = compare([("matgcn_group_sums", lambda: ops.group_sums(samples, rm, out=out, **scale)),
                       ("torch de-scale + clamp + index_add_", by_index_add),
                       ("torch de-scale + clamp + matmul", by_matmul),
                       ("one read (samples.sum(0))", lambda: samples.sum(0))],
                      "torch de-scale + clamp + matmul", samples=s, sample_mb=mb, map=label, groups=g, members=rm.num_members,
                      worst_relative_gap_to_matmul=worst, kernel_repeats_bit_equal=repeat,
                      index_add_repeats_bit_equal=atomics_repeat)
        print(json.dumps(dict(workload=name, samples=s, map=label, what="matgcn_group_sums over the plain-read floor",
                              ratio=round(med["matgcn_group_sums"] / med["one read (samples.sum(0))"], 3),
                              source=build.source_id())), flush=True)
        del dense, out, got, ref
    del samples

# ---- the whole call: predict_interval with and without regions ------------------------------------------------------------
model, df, cfg = bench.build_model(w, dev, 0)
model.eval()
model._scaler = syn.PlainScaler(MEAN, STD)
x_np, _ = syn.make_batch_arrays(B, N, OUT, 0, feat=2)
batch = {"X": torch.from_numpy(x_np).to(dev)}
kw = dict(group_mean=gm, group_std=gs, clamp_min=0.0)
with torch.no_grad():
    for s in sizes:
        routes = [("predict_interval (node level)", lambda: model.predict_interval(batch, samples=s, probs=PROBS, seed=1, **kw))]
        for label, rm in MAPS.items():
            routes.append(("predict_interval(regions=%s)" % label,
                           lambda rm=rm: model.predict_interval(batch, samples=s, probs=PROBS, seed=1, regions=rm, **kw)))
        compare(routes, "predict_interval (node level)", samples=s)
