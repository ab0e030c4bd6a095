"""Quantiles and scores of a Monte-Carlo-dropout ensemble at a bench workload's output shape (default Baltimore 403, B = 64):
matgcn_mc_quantiles with three levels and matgcn_mc_scores, next to what a user had before - torch.sort over the sample axis
plus the same interpolation in torch - and to the floor, one read of the tensor (samples.sum(0)); HIP events, median over the
repetitions after the first three, all in one process.  The samples are synthetic: the kernels' time depends on their shape,
not on the model that drew them.
usage: mc_scores_time.py [workload] [reps] [S ...]     (default: bm403 20 32 128)"""
import math, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd.ops import mc_quantiles, mc_scores
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sizes = [int(v) for v in sys.argv[3:]] or [32, 128]
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
PROBS = (0.05, 0.5, 0.95)
MEAN, STD = -1.25, 3.5
shape = (w["batch"], w["out"], w["nodes"], 1)


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


def torch_quantiles(samples):
    xs = torch.sort(samples * STD + MEAN, dim=0).values
    out = []
    for q in PROBS:
        h = float(torch.tensor(q, dtype=torch.float32)) * (xs.shape[0] - 1)
        j = int(math.floor(h))
        lo, hi = xs[j], xs[min(j + 1, xs.shape[0] - 1)]
        out.append(lo + (h - j) * (hi - lo))
    return torch.stack(out, 0)


gen = torch.Generator(device=dev).manual_seed(0)
y = torch.randn(shape, generator=gen, device=dev)
for s in sizes:
    samples = torch.randn((s,) + shape, generator=gen, device=dev)
    worst = float((mc_quantiles(samples, PROBS, MEAN, STD) - torch_quantiles(samples)).abs().max())
    t_q = timed(lambda: mc_quantiles(samples, PROBS, MEAN, STD))
    t_s = timed(lambda: mc_scores(samples, y, PROBS, mean=MEAN, std=STD))
    t_t = timed(lambda: torch_quantiles(samples))
    t_f = timed(lambda: samples.sum(0))
    print("%s B = %d, S = %d (%.1f MB): matgcn_mc_quantiles %.3f ms, matgcn_mc_scores %.3f ms, torch.sort + interpolation "
          "%.3f ms, one read (samples.sum(0)) %.3f ms; kernel against torch quantiles: largest difference %.2e"
          % (name, w["batch"], s, samples.numel() * 4 / 1e6, t_q, t_s, t_t, t_f, worst), flush=True)
    del samples
