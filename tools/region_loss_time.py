"""The tract + region training objective alone - forward and backward of the loss, no model step - on one HIP prediction of
a bench workload (default Baltimore 403, B = 64, out = 24), ten regions and ten regions plus one whole-city group: device
time (HIP events) and host enqueue time (perf_counter, no synchronisation inside), in one process, the routes alternating:
  (a) device: ops.tract_region_loss - matgcn_loss + matgcn_region_loss, then matgcn_loss_grad + matgcn_region_loss_grad
  (b) torch: de-scale, dense-membership matmul, tests/train_loss_ref.torch_loss on both levels, autograd
  (c) device, tracts only: ops.train_loss - what (a) adds to is (a) - (c)
  (e) matgcn_region_loss_grad alone on the scratch of a value call (base = NULL)
  (d) the memory floor of (e): one plain read of the totals (a copy of them) plus one write of d_pred (a fill)
Every (round, map, objective, route) is one JSON line: the medians over the steps after the first three.  The last lines
give, per map, objective and route, the median over the rounds and their spread (largest - smallest): (a) against (b)
counts only beyond twice the spread of (b).
usage: region_loss_time.py [--out FILE] [workload] [steps] [rounds]    (default: bm403 30 3; FILE gets the JSON lines appended)"""
import json, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench
import train_loss_ref
from multistgraph_amd import build as mbuild, ops, synthetic as syn
from multistgraph_amd.regions import RegionMap
out_path = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out_path = sys.argv[i + 1]
    del sys.argv[i:i + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
OBJECTIVES = ("masked_mae", "huber", "masked_mse")
MEAN, STD = 14.41, 29.3        # Baltimore's flow statistics
TW, RW = 1.0, 0.5
w = dict(bench.WORKLOADS[name])
dev = torch.device("cuda:0")
model, df, cfg = bench.build_model(w, dev, 0)
model.eval()
x_np, y_np = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
y = torch.from_numpy(y_np).to(dev)
with torch.no_grad():
    pred = model.predict({"X": torch.from_numpy(x_np).to(dev)}).clone()
torch.cuda.synchronize()
n = w["nodes"]
labels = np.random.default_rng(n).integers(0, 10, n)
ten = [np.flatnonzero(labels == g).tolist() for g in range(10)]
MAPS = {"ten": RegionMap(n, groups=ten), "ten+city": RegionMap(n, groups=ten + [list(range(n))])}


def dense(rm):
    m = torch.zeros(rm.num_groups, n)
    for g in range(rm.num_groups):
        for k in rm.members(g):
            m[g, k] += 1.0
    return m.to(dev)


DENSE = {k: dense(rm) for k, rm in MAPS.items()}


def device_route(objective, key):
    def step():
        p = pred.detach().requires_grad_(True)
        loss = ops.tract_region_loss(p, y, MAPS[key], 0, MEAN, STD, objective, tract_weight=TW, region_weight=RW)
        loss.backward()
        return loss, p.grad
    return step


def torch_route(objective, key):
    def step():
        p = pred.detach().requires_grad_(True)
        ps, ls = p * STD + MEAN, y[..., 0:1] * STD + MEAN
        m = DENSE[key]
        loss = TW * train_loss_ref.torch_loss(objective, ps, ls) + RW * train_loss_ref.torch_loss(
            objective, torch.einsum("gn,bonc->bogc", m, ps), torch.einsum("gn,bonc->bogc", m, ls))
        loss.backward()
        return loss, p.grad
    return step


def tract_route(objective, key):
    def step():
        p = pred.detach().requires_grad_(True)
        loss = ops.train_loss(p, y, 0, MEAN, STD, objective)
        loss.backward()
        return loss, p.grad
    return step


def grad_kernel_route(objective, key):
    desc = ops.train_loss_desc(objective, MEAN, STD)
    view = ops._label_view(pred, y, None)
    scratch, _ = ops._region_loss_call(view, MAPS[key], 0, desc)
    up = torch.ones(1, device=dev)
    d_pred = torch.empty_like(view.pred)

    def step():
        ops._region_loss_grad_call(view, MAPS[key], 0, desc, scratch, up, None, d_pred)
        return None, d_pred
    return step


def floor_route(objective, key):
    totals = torch.zeros(2 * pred.shape[0] * pred.shape[1] * MAPS[key].num_groups, device=dev)
    copy, d_pred = torch.empty_like(totals), torch.empty_like(pred)

    def step():
        copy.copy_(totals)
        d_pred.fill_(1.0)
        return None, d_pred
    return step


ROUTES = (("a: tract_region_loss", device_route), ("b: torch, both levels", torch_route), ("c: train_loss, tracts only", tract_route),
          ("e: matgcn_region_loss_grad alone", grad_kernel_route), ("d: read totals + write d_pred", floor_route))
lines = []
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
for key in MAPS:                   # the two routes compute the same thing, at the size that is timed
    for objective in OBJECTIVES:
        (la, ga), (lb, gb) = device_route(objective, key)(), torch_route(objective, key)()
        print("%s %s: device %.6f torch %.6f, gradients differ by %.3g of their largest" % (
            key, objective, float(la.detach()), float(lb.detach()), float((ga - gb).abs().max() / gb.abs().max())), flush=True)
for r in range(rounds):
    for key in MAPS:
        for objective in OBJECTIVES:
            for label, make in ROUTES:
                step = make(objective, key)
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
                line = dict(tool="region_loss_time", workload=name, batch=w["batch"], elements=pred.numel(), round=r,
                            regions=key, groups=MAPS[key].num_groups, members=MAPS[key].num_members, objective=objective,
                            route=label, steps=steps, device_ms=round(statistics.median(dev_ms[3:]), 4),
                            host_ms=round(statistics.median(host_ms[3:]), 4), source_id=mbuild.source_id(),
                            torch=torch.__version__)
                lines.append(line)
                print(json.dumps(line), flush=True)
for key in MAPS:
    for objective in OBJECTIVES:
        for label, _ in ROUTES:
            mine = [l for l in lines if l["route"] == label and l["objective"] == objective and l["regions"] == key]
            for k in ("device_ms", "host_ms"):
                vals = [l[k] for l in mine]
                print("%-9s %-11s %-34s %-9s median of %d rounds %.4f ms, spread %.4f ms" % (
                    key, objective, label, k, rounds, statistics.median(vals), max(vals) - min(vals)), flush=True)
if out_path:
    with open(out_path, "a") as fh:
        for line in lines:
            fh.write(json.dumps(line) + "\n")
