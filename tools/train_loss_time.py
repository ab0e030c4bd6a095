"""A training objective alone - forward and backward of the loss, no model step - on one HIP prediction of a bench workload
(default Baltimore 403, B = 64, out = 24): device time (HIP events) and host enqueue time (perf_counter, no synchronisation
inside) of two routes, in one process, the routes alternating:
  (a) torch: the executor closure's arithmetic (two inverse_transforms, then the elementwise kernels of libcity's loss
      function and their autograd twins; tests/train_loss_ref.torch_loss, which the host tests pin to the reference's bits)
  (b) device: ops.train_loss - matgcn_loss, then matgcn_loss_grad from backward()
Every (round, objective, route) is one JSON line: the medians over the steps after the first three.  The last lines give,
per objective and route, the median over the rounds and their spread (largest - smallest): a difference counts only beyond
twice the spread of (a); otherwise the routes are level.
usage: train_loss_time.py [--out FILE] [workload] [steps] [rounds]     (default: bm403 30 3; FILE gets the JSON lines appended)"""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import train_loss_ref
from multistgraph_amd import build as mbuild, ops, synthetic as syn
out_path = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out_path = sys.argv[i + 1]
    del sys.argv[i:i + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OBJECTIVES = ("masked_mse", "huber", "logcosh")
MEAN, STD = 14.41, 29.3        # Baltimore's flow statistics
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
model, df, cfg = bench.build_model(w, dev, 0)
model.eval()
x_np, y_np = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
y = torch.from_numpy(y_np).to(dev)
with torch.no_grad():
    pred = model.predict({"X": torch.from_numpy(x_np).to(dev)}).clone()
torch.cuda.synchronize()


def torch_route(objective):
    def step():
        p = pred.detach().requires_grad_(True)
        loss = train_loss_ref.torch_loss(objective, p * STD + MEAN, y[..., 0:1] * STD + MEAN)
        loss.backward()
        return loss, p.grad
    return step


def device_route(objective):
    def step():
        p = pred.detach().requires_grad_(True)
        loss = ops.train_loss(p, y, 0, MEAN, STD, objective)
        loss.backward()
        return loss, p.grad
    return step


ROUTES = (("a: torch closure", torch_route), ("b: matgcn_loss + matgcn_loss_grad", device_route))
lines = []
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for objective in OBJECTIVES:       # the two routes compute the same thing, at the size that is timed
    (la, ga), (lb, gb) = torch_route(objective)(), device_route(objective)()
    print("%s: torch %.6f device %.6f, gradients differ by %.3g of their largest" % (
        objective, float(la.detach()), float(lb.detach()), float((ga - gb).abs().max() / ga.abs().max())), flush=True)
for r in range(rounds):
    for objective in OBJECTIVES:
        for label, make in ROUTES:
            step = make(objective)
            dev_ms, host_ms = [], []
            for _ in range(steps + 3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ev[0].record()
                step()
                ev[1].record()
                host_ms.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                dev_ms.append(ev[0].elapsed_time(ev[1]))
            line = dict(tool="train_loss_time", workload=name, batch=w["batch"], elements=pred.numel(), round=r,
                        objective=objective, route=label, steps=steps, device_ms=round(statistics.median(dev_ms[3:]), 4),
                        host_ms=round(statistics.median(host_ms[3:]), 4), source_id=mbuild.source_id(),
                        torch=torch.__version__)
            lines.append(line)
            print(json.dumps(line), flush=True)
for objective in OBJECTIVES:
    for label, _ in ROUTES:
        mine = [l for l in lines if l["route"] == label and l["objective"] == objective]
        for key in ("device_ms", "host_ms"):
            vals = [l[key] for l in mine]
            print("%-11s %-36s %-9s median of %d rounds %.4f ms, spread %.4f ms" % (
                objective, label, key, rounds, statistics.median(vals), max(vals) - min(vals)), flush=True)
if out_path:
    with open(out_path, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
