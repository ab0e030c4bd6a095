"""The optimizer step of the training recipe alone, over a bench workload's parameter set (default Baltimore 403) and the
gradient bucket one real backward at B = 16 filled: device time (HIP events) and host enqueue time (perf_counter, no
synchronisation inside) of three routes, in one process, the routes alternating:
  (a) clip_grad_norm_(5) + torch.optim.Adam, torch's default implementation
  (b) the same with fused=True
  (c) multistgraph_amd.optim.ClipAdam(max_grad_norm=5)
Every (round, route) is one JSON line: the medians over the steps after the first three.  The last lines give, per route,
the median over the rounds and their spread (largest - smallest): a difference counts only beyond twice the spread of (a).
usage: optim_time.py [--out FILE] [workload] [steps] [rounds]     (default: bm403 30 3; FILE gets the JSON lines appended)"""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import build as mbuild, synthetic as syn
from multistgraph_amd.optim import ClipAdam
out_path = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out_path = sys.argv[i + 1]
    del sys.argv[i:i + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
w = dict(bench.WORKLOADS[name])
w["batch"] = 16
dev = torch.device("cuda:0")
model, df, cfg = bench.build_model(w, dev, 0)
model.train()
x_np, y_np = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
model.calculate_loss({"X": torch.from_numpy(x_np).to(dev), "y": torch.from_numpy(y_np).to(dev)}).backward()
params = [p for p in model.parameters() if p.grad is not None]
filled = [p.grad.clone() for p in params]          # clip_grad_norm_ scales .grad in place: every step starts from these
elements = sum(p.numel() for p in params)
torch.cuda.synchronize()


def torch_route(**kw):
    opt = torch.optim.Adam(params, lr=3e-3, **kw)

    def step():
        torch.nn.utils.clip_grad_norm_(params, 5)
        opt.step()
    return step


def fused_route():
    return ClipAdam(params, lr=3e-3, max_grad_norm=5).step


ROUTES = (("a: clip_grad_norm_ + Adam", lambda: torch_route()), ("b: clip_grad_norm_ + Adam(fused=True)",
          lambda: torch_route(fused=True)), ("c: ClipAdam", fused_route))
lines = []
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for r in range(rounds):
    for label, make in ROUTES:
        step = make()
        dev_ms, host_ms = [], []
        for _ in range(steps + 3):
            torch._foreach_copy_([p.grad for p in params], filled)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            step()
            ev[1].record()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            dev_ms.append(ev[0].elapsed_time(ev[1]))
        line = dict(tool="optim_time", workload=name, tensors=len(params), elements=elements, round=r, route=label,
                    steps=steps, device_ms=round(statistics.median(dev_ms[3:]), 4),
                    host_ms=round(statistics.median(host_ms[3:]), 4), source_id=mbuild.source_id(),
                    torch=torch.__version__)
        lines.append(line)
        print(json.dumps(line), flush=True)
for label, _ in ROUTES:
    mine = [l for l in lines if l["route"] == label]
    for key in ("device_ms", "host_ms"):
        vals = [l[key] for l in mine]
        print("%-40s %-9s median of %d rounds %.4f ms, spread %.4f ms" % (label, key, rounds, statistics.median(vals),
                                                                        max(vals) - min(vals)), flush=True)
if out_path:
    with open(out_path, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
