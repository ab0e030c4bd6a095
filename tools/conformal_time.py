"""Conformal calibration at a bench workload's output shape (default Baltimore 403, B = 64, out = 24).
Per batch, S = 32 and 128: matgcn_mc_conformity next to matgcn_mc_scores_nodes (the same sort, so parity is the expectation)
and to a torch route - torch.sort over the sample axis and the same arithmetic.  Per calibration, a store of 540 rows:
matgcn_conformal_quantile in both groupings next to torch.kthvalue (per horizon, NaN scores sorted behind +inf) and
torch.sort (per element), and matgcn_conformal_coverage next to the torch comparison.
Protocol: one process; the routes of a group alternate three times, each visit the median of `reps` calls after three
warm-up calls, HIP events; reported per route: the median of its three visits and their spread (max - min).  A route
counts as faster than the torch route when the gap exceeds twice the larger spread, otherwise "level".
One JSON line per route; the inputs are synthetic: the kernels' time depends on the shape alone (the radix select's on no
value at all - every loop bound is a count).
Measured (MI355X, bm403 20 32 128, profiles/conformal_times.jsonl; ms, spread of the three visits in brackets):
  S = 32:  matgcn_mc_conformity 0.137 (0.009), matgcn_mc_scores_nodes 0.176 (0.004), torch.sort + score 0.485 (0.009)
  S = 128: 0.909 (0.003), 0.979 (0.002), 4.744 (0.005)
  540 rows: matgcn_conformal_quantile per horizon 0.343 (0.0004) against torch.kthvalue per horizon 19.96 (0.004: 24 ranks
  read back from the device), per element 0.224 (0.002) against torch.sort per group 0.417 (0.001)
  one batch: matgcn_conformal_coverage 0.031 / 0.017 against torch compare + sum 0.054 / 0.046
Every kernel is faster than its torch route by more than twice the larger spread; scores and margins equal torch's.
usage: conformal_time.py [workload] [reps] [S ...]     (default: bm403 20 32 128)"""
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
ROWS = 540
B, OUT, N = w["batch"], w["out"], w["nodes"]
shape = (B, OUT, N, 1)
NAN, INF = float("nan"), float("inf")


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


gen = torch.Generator(device=dev).manual_seed(0)
y = torch.randn(shape, generator=gen, device=dev)
gm = 20.0 * torch.rand(N, generator=gen, device=dev)
gs = 0.5 + torch.rand(N, generator=gen, device=dev)
mean_t, std_t = torch.tensor([MEAN], device=dev), torch.tensor([STD], device=dev)      # no upload inside the timed calls
scale = dict(mean=mean_t, std=std_t, group_mean=gm, group_std=gs, clamp_min=0.0, truth_min=S_SMALL, min_s=-1.0)
nan_t = torch.tensor(NAN, device=dev)


def retransform(x):
    return (x * STD + MEAN) * gs[:, None] + gm[:, None]


def torch_conformity(samples):
    s = samples.shape[0]
    xs = torch.sort(retransform(samples).clamp_min(0.0), dim=0).values
    l = retransform(y)
    q = []
    for level in (PROBS[0], PROBS[-1]):
        h = float(torch.tensor(level, dtype=torch.float32)) * (s - 1)
        j = int(math.floor(h))
        lo, hi = xs[j], xs[min(j + 1, s - 1)]
        q.append(lo + (h - j) * (hi - lo))
    return torch.where(l > S_SMALL, torch.maximum(q[0] - l, l - q[1]), nan_t)


for s in sizes:
    samples = torch.randn((s,) + shape, generator=gen, device=dev)
    mb = round(samples.numel() * 4 / 1e6, 1)
    out = torch.empty(shape, device=dev)
    got, ref = ops.mc_conformity(samples, y, PROBS, null_val=NAN, **scale), torch_conformity(samples)
    same = float(((got == ref) | (torch.isnan(got) & torch.isnan(ref))).float().mean())
    compare([("matgcn_mc_conformity", lambda: ops.mc_conformity(samples, y, PROBS, null_val=NAN, out=out, **scale)),
             ("matgcn_mc_scores_nodes", lambda: ops.mc_scores_nodes(samples, y, PROBS, null_val=NAN, **scale)),
             ("torch.sort + score", lambda: torch_conformity(samples))],
            "torch.sort + score", samples=s, sample_mb=mb, share_equal_to_torch=round(same, 6))
    del samples, got, ref

# ---- per calibration: a store of ROWS rows of scores, 10 % of them masked --------------------------------------------------
store = torch.randn((2 * ROWS, OUT, N, 1), generator=gen, device=dev)
store[torch.rand(store.shape, generator=gen, device=dev) < 0.1] = NAN
coverage = float(torch.tensor(PROBS[-1], dtype=torch.float32)) - float(torch.tensor(PROBS[0], dtype=torch.float32))


def torch_quantile(grouping):
    """the same rank rule in torch; NaN scores are moved behind every number, the rank is per group"""
    x = store[:ROWS].reshape(ROWS, OUT, N)
    x = x.permute(1, 0, 2).reshape(OUT, ROWS * N) if grouping == "horizon" else x.permute(1, 2, 0).reshape(OUT * N, ROWS)
    n = (~torch.isnan(x)).sum(1)
    k = torch.ceil((n + 1).double() * coverage).clamp_min(1).long()
    filled = torch.where(torch.isnan(x), torch.full_like(x, INF), x)
    if grouping == "horizon":      # one kthvalue per horizon: the ranks differ, and each is read back for the call
        picked = torch.stack([torch.kthvalue(filled[o], int(min(k[o], filled.shape[1]))).values for o in range(OUT)])
    else:
        picked = torch.sort(filled, dim=1).values.gather(1, (k.clamp_max(ROWS) - 1)[:, None])[:, 0]
    return torch.where(k <= n, picked, torch.full_like(picked, INF)), n


for grouping in ("horizon", "element"):
    margin, count = ops.conformal_quantile(store, ROWS, grouping, coverage)
    ref_m, ref_n = torch_quantile(grouping)
    same = bool(torch.equal(margin.reshape(-1), ref_m) and torch.equal(count.reshape(-1).long(), ref_n))
    torch_route = "torch.kthvalue per horizon" if grouping == "horizon" else "torch.sort per element"
    compare([("matgcn_conformal_quantile (%s)" % grouping, lambda: ops.conformal_quantile(store, ROWS, grouping, coverage)),
             (torch_route, lambda: torch_quantile(grouping))],
            torch_route, rows=ROWS, store_mb=round(ROWS * OUT * N * 4 / 1e6, 1), equal_to_torch=same)
    batch = store[:B]
    m3 = margin.reshape(OUT, -1, 1) if grouping == "element" else margin.reshape(OUT, 1, 1)
    over = (0,) if grouping == "element" else (0, 2, 3)
    torch_cover = lambda: torch.stack([(~torch.isnan(batch)).sum(over), (batch <= m3).sum(over)], -1)
    assert torch.equal(ops.conformal_coverage(batch, B, grouping, margin), torch_cover())
    compare([("matgcn_conformal_coverage (%s)" % grouping, lambda: ops.conformal_coverage(batch, B, grouping, margin)),
             ("torch compare + sum", torch_cover)], "torch compare + sum", rows=B)
