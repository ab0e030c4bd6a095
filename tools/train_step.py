"""Training steps of the bench workload (default Baltimore 403, B=64): forward_train + backward through the plugin
surface (calculate_loss().backward()), timed with HIP events.
usage: train_step.py [--deterministic] [--bf16x3] [--device-dropout] [--clip] [--fused-optimizer] [--loss NAME] [--region-weight W] [workload] [steps] [serial|wave] [batch] [fp32|bf16_mix|bf16]
(--loss NAME: the model's hip_train_loss - calculate_loss returns that objective of the executor instead of masked MAE,
value and gradient from matgcn_loss / matgcn_loss_grad)
(--region-weight W: the model's hip_region_loss_weight = W over ten random regions plus one whole-city group - calculate_loss
returns L(tracts) + W * L(region totals), ops.tract_region_loss)
(--deterministic: the model's hip_deterministic = True - the backward's sums in a fixed order, see matgcn_set_deterministic;
the summary line then also gives the bytes the train buffer grew by)
(--bf16x3: the model's hip_precision = "bf16x3_train" - the step's graph mixes, both directions, from three bf16 pieces,
see matgcn_set_train_bf16x3; a hip_precision argument wins over it)
(--device-dropout: the model's hip_dropout = "device" - the dropout in front of the head drawn inside the kernels that apply
it, no mask tensor and no F.dropout; see matgcn_forward_train_seeded)
(--clip: the recipe's clip_grad_norm_(parameters, 5) in front of the optimizer step;  --fused-optimizer: the step is
multistgraph_amd.optim.ClipAdam - with --clip its own global-norm clip, max_grad_norm = 5 - in place of torch.optim.Adam;
every step line and the summary also give the host's enqueue time of the whole step, perf_counter without a synchronisation)
(serial: matgcn_set_wavefront(0) - every kernel alone on one stream, so a profiler's durations are the kernels' own;
the last argument is the model's hip_precision; the last line gives the medians over the steps after the first three)"""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench
from multistgraph_amd import synthetic as syn
deterministic = "--deterministic" in sys.argv
if deterministic:
    sys.argv.remove("--deterministic")
bf16x3 = "--bf16x3" in sys.argv
if bf16x3:
    sys.argv.remove("--bf16x3")
device_dropout = "--device-dropout" in sys.argv
if device_dropout:
    sys.argv.remove("--device-dropout")
clip = "--clip" in sys.argv
if clip:
    sys.argv.remove("--clip")
fused_optimizer = "--fused-optimizer" in sys.argv
if fused_optimizer:
    sys.argv.remove("--fused-optimizer")
train_loss = "none"
if "--loss" in sys.argv:
    i = sys.argv.index("--loss")
    train_loss = sys.argv[i + 1]
    del sys.argv[i:i + 2]
region_weight = 0.0
if "--region-weight" in sys.argv:
    i = sys.argv.index("--region-weight")
    region_weight = float(sys.argv[i + 1])
    del sys.argv[i:i + 2]
name = sys.argv[1] if len(sys.argv) > 1 else "bm403"
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
w = dict(bench.WORKLOADS[name])
if len(sys.argv) > 4:
    w["batch"] = int(sys.argv[4])      # e.g. 16, the reference's shipped batch_size
dev = torch.device("cuda:0")
model, df, cfg = bench.build_model(w, dev, 0)
model.train()
model.hip_deterministic = deterministic
if bf16x3:
    model.hip_precision = "bf16x3_train"
if device_dropout:
    model.hip_dropout = "device"
if train_loss != "none":
    from multistgraph_amd.ops import train_loss_desc
    train_loss_desc(train_loss, 0.0, 1.0)      # a bad name stops here
    model.hip_train_loss = train_loss.lower()
if region_weight > 0.0:
    import numpy as np
    from multistgraph_amd.regions import RegionMap
    labels = np.random.default_rng(w["nodes"]).integers(0, 10, w["nodes"])
    groups = [np.flatnonzero(labels == g).tolist() for g in range(10)] + [list(range(w["nodes"]))]
    model.hip_train_regions, model.hip_region_loss_weight = RegionMap(w["nodes"], groups=groups), region_weight
if len(sys.argv) > 5:
    model.hip_precision = sys.argv[5]
if len(sys.argv) > 3 and sys.argv[3] == "serial":
    from multistgraph_amd import _lib
    _lib.load().matgcn_set_wavefront(0)
x_np, y_np = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
batch = {"X": torch.from_numpy(x_np).to(dev), "y": torch.from_numpy(y_np).to(dev)}
if fused_optimizer:
    from multistgraph_amd.optim import ClipAdam
    opt = ClipAdam(model.parameters(), lr=1e-3, max_grad_norm=5 if clip else None)
else:
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
times = []
for i in range(steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    opt.zero_grad()
    ev[0].record()
    loss = model.calculate_loss(batch)
    ev[1].record()
    loss.backward()
    ev[2].record()
    if clip and not fused_optimizer:
        torch.nn.utils.clip_grad_norm_(model.parameters(), 5)
    opt.step()
    ev[3].record()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    times.append((ev[0].elapsed_time(ev[3]), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]),
                  ev[2].elapsed_time(ev[3]), host_ms))
    print("step %d loss %.5f  forward %.2f ms  backward %.2f ms  adam %.2f ms  host enqueue %.2f ms" % (
        i, float(loss), ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2]), ev[2].elapsed_time(ev[3]), host_ms), flush=True)
print("train buffer %.2f GB  workspace %.2f GB  peak torch memory %.2f GB" % (
    next(iter(model._paths.values()))._train.numel() * 4 / 2**30,
    next(iter(model._paths.values())).workspace.numel() * 4 / 2**30, torch.cuda.max_memory_allocated() / 2**30))
if len(times) > 3:
    import statistics
    med = [statistics.median(t[k] for t in times[3:]) for k in range(5)]
    print("median of %d steps (%s, B = %d, %s%s%s%s%s%s%s): step %.3f ms  forward %.3f ms  backward %.3f ms  optimizer %.3f ms  "
          "host enqueue %.3f ms" % (
              len(times) - 3, name, w["batch"], model.hip_precision, ", deterministic" if deterministic else "",
              ", device dropout" if device_dropout else "", ", clip 5" if clip else "",
              ", ClipAdam" if fused_optimizer else "", ", loss %s" % model.hip_train_loss if train_loss != "none" else "",
              ", region weight %g" % region_weight if region_weight > 0.0 else "",
              med[0], med[1], med[2], med[3], med[4]))
if deterministic:
    import ctypes
    from multistgraph_amd import _lib
    hp, lib, nb = next(iter(model._paths.values())), _lib.load(), [ctypes.c_size_t(), ctypes.c_size_t()]
    for on in (0, 1):
        prev = lib.matgcn_set_deterministic(on)
        lib.matgcn_train_bytes(ctypes.byref(hp.dims), ctypes.byref(nb[on]))
        lib.matgcn_set_deterministic(prev)
    print("deterministic scratch: %d bytes (%.1f MB) behind a train buffer of %d" % (
        nb[1].value - nb[0].value, (nb[1].value - nb[0].value) / 2**20, nb[0].value))
