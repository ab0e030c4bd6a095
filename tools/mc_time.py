"""Monte-Carlo-dropout forward of a bench workload (default Baltimore 403, B = 64): matgcn_forward_mc at S samples next to
one matgcn_forward of the same process, timed with HIP events (median over the repetitions after the first three).
usage: mc_time.py [workload] [reps] [S ...]     (default: bm403 20 32 128)
(under `rocprofv3 --kernel-trace --stats` the k_head_mc line divided by its calls and S gives the per-sample time)"""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import synthetic as syn
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sizes = [int(v) for v in sys.argv[3:]] or [32, 128]
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
model, df, cfg = bench.build_model(w, dev, 0)
model.eval()
x_np, _ = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
batch = {"X": torch.from_numpy(x_np).to(dev)}


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


with torch.no_grad():
    fwd = timed(lambda: model.predict(batch))
    print("%s B = %d: matgcn_forward %.3f ms" % (name, w["batch"], fwd), flush=True)
    for s in sizes:
        mc = timed(lambda: model.predict_mc(batch, samples=s, seed=1))
        print("matgcn_forward_mc S = %d: %.3f ms = forward + %.3f ms (%.1f us per sample); %d host-loop forwards would take %.1f ms"
              % (s, mc, mc - fwd, 1e3 * (mc - fwd) / s, s, s * fwd), flush=True)
