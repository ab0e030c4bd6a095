"""Ensemble training (config['hip_train_loss'] = "crps") on a bench workload (default Baltimore 403, out = 24) at B = 64 and
at the reference's shipped B = 16, S = 8 and 32 samples: device time (HIP events) and host enqueue time (perf_counter, no
synchronisation inside), one process, the routes alternating, the protocol of tools/train_step.py:
  (a) the CRPS step: calculate_loss (matgcn_forward_train_mc + matgcn_crps_loss) + backward (matgcn_crps_loss_grad +
      matgcn_backward_mc) + torch.optim.Adam
  (b) the same build's seeded masked-MAE step (hip_dropout = "device", one mask)
  (c) the route a user has without the feature: S seeded steps whose gradients accumulate, one optimizer step
  (d) pieces, alone: matgcn_forward_train_mc against matgcn_forward_train (the difference is the head over the samples
      against one head), matgcn_backward_mc against matgcn_backward_seeded (the difference is the three head kernels over
      the samples against the head's two GEMMs), matgcn_crps_loss + matgcn_crps_loss_grad on the samples, and one read of
      the samples (samples.sum(0)) - the CRPS pair's floor is one read plus one write of them
Every (round, batch, S, route) is one JSON line: the medians over the steps after the first three.  The last lines give the
median over the rounds and their spread per (batch, S, route).  The kernels' own durations come from a kernel trace of
`crps_train_time.py --kernels` (the serial schedule, a handful of CRPS steps at B = 64, S = 32: every kernel alone on one
stream): k_head_mc, k_crps_partial, k_crps_grad, k_head_mc_dseq, k_head_mc_wgrad.
usage: crps_train_time.py [--out FILE] [--kernels] [workload] [steps] [rounds]   (default: bm403 30 3)"""
import json, os, statistics, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import build as mbuild, ops, synthetic as syn
out_path = None
if "--out" in sys.argv:
    i = sys.argv.index("--out")
    out_path = sys.argv[i + 1]
    del sys.argv[i:i + 2]
kernels = "--kernels" in sys.argv
if kernels:
    sys.argv.remove("--kernels")
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
SAMPLES = (8, 32)
MEAN, STD = 14.41, 29.3        # Baltimore's flow statistics
dev = torch.device("cuda:0")
w = dict(bench.WORKLOADS[name])
model, df, cfg = bench.build_model(w, dev, 0)
model.train()
model.hip_dropout = "device"
model._scaler = syn.PlainScaler(MEAN, STD)
opt = torch.optim.Adam(model.parameters(), lr=1e-3)
BUILD = mbuild.source_id()


def batch_of(b):
    x_np, y_np = syn.make_batch_arrays(b, w["nodes"], w["out"], 0, feat=2)
    return {"X": torch.from_numpy(x_np).to(dev), "y": torch.from_numpy(y_np).to(dev)}


def timed(fn, n):
    """medians over the calls after the first three: (device ms, host enqueue ms)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dev_ms, host_ms = [], []
    for _ in range(n + 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        torch.cuda.synchronize()
        dev_ms.append(a.elapsed_time(b))
    return statistics.median(dev_ms[3:]), statistics.median(host_ms[3:])


def step_route(batch, loss_name, samples, repeats=1):
    def step():
        model.hip_train_loss, model.hip_train_samples = loss_name, samples
        opt.zero_grad()
        for _ in range(repeats):
            model.calculate_loss(batch).backward()
        opt.step()
    return step


def piece_routes(batch, s):
    hp = model._path_for_batch(batch["X"].shape[0], dev)
    state = {k: v for k, v in model._state().items() if not k.startswith("static_initial")}
    x, y = batch["X"], batch["y"]
    drop = (1234, 0, 0.1)
    kept = hp.forward_train_mc(x, drop, s).clone()
    d_one = torch.randn_like(kept[0])

    def crps_pair():
        t = kept.clone().requires_grad_(True)
        ops.crps_loss(t, y, 0, MEAN, STD, 0.0).backward()

    def bwd_mc():
        hp.forward_train_mc(x, drop, s)
        hp.backward_mc(x, kept, state, drop)

    def bwd_one():
        hp.forward_train(x, dropout=drop)
        hp.backward(x, d_one, state, dropout=drop)

    return {"forward_train_mc": lambda: hp.forward_train_mc(x, drop, s), "forward_train": lambda: hp.forward_train(x, dropout=drop),
            "forward_train_mc+backward_mc": bwd_mc, "forward_train+backward_seeded": bwd_one,
            "clone+crps_loss+grad": crps_pair, "clone": lambda: kept.clone(), "samples.sum(0)": lambda: kept.sum(0)}


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out_path:
        with open(out_path, "a") as fh:
            fh.write(line + "\n")


if kernels:      # for a kernel trace: the serial schedule, a handful of CRPS steps at S = 32
    from multistgraph_amd import _lib
    _lib.load().matgcn_set_wavefront(0)
    b = batch_of(w["batch"])
    fn = step_route(b, "crps", 32)
    for _ in range(steps if len(sys.argv) > 2 else 6):
        fn()
    torch.cuda.synchronize()
    print("ran CRPS steps at %s, B = %d, S = 32 in the serial schedule (build %s)" % (name, w["batch"], BUILD))
    sys.exit(0)

records = []
for b_size in (w["batch"], 16):
    b = batch_of(b_size)
    for rnd in range(rounds):
        for s in SAMPLES:
            routes = {"a_crps_step": (step_route(b, "crps", s), steps),
                      "b_seeded_mae_step": (step_route(b, "none", s), steps),
                      "c_S_seeded_steps": (step_route(b, "none", s, repeats=s), max(4, steps // 6))}
            for key, fn in piece_routes(b, s).items():
                routes["d_" + key] = (fn, steps)
            for key, (fn, n) in routes.items():
                d_ms, h_ms = timed(fn, n)
                rec = dict(tool="crps_train_time", build=BUILD, workload=name, batch=b_size, samples=s, round=rnd, route=key,
                           steps=n, device_ms=round(d_ms, 4), host_ms=round(h_ms, 4))
                records.append(rec)
                emit(rec)
model.hip_train_loss = "none"
for b_size in (w["batch"], 16):
    for s in SAMPLES:
        for key in dict.fromkeys(r["route"] for r in records):
            v = [r["device_ms"] for r in records if (r["batch"], r["samples"], r["route"]) == (b_size, s, key)]
            print("B = %d, S = %d, %-32s median %.3f ms over %d rounds, spread %.3f ms" % (
                b_size, s, key, statistics.median(v), len(v), max(v) - min(v)))
