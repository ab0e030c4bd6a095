#!/usr/bin/env python3
"""The side line of a precision mode beside the fp32 headline of bench.py: inference forwards of a bench workload
(default Baltimore 403, B = 64) through the plugin surface (predict()) with the model's hip_precision set, each bracketed
by HIP events.  What tools/fwd_time.py does not do: it selects the precision mode, and it reports the prediction's distance
from the fp32 forward of the same model next to the time.
    python tools/precision_side_line.py --precision bf16x3 [--workload bm403] [--forwards 50] [--serial] [--batch 16]
--serial: matgcn_set_wavefront(0) - every kernel alone on one stream, so that a profiler's durations are the kernels' own
(the configuration of `rocprofv3 --kernel-trace --stats`).  The last line is one JSON object: median / p10 / p90 over the
forwards after the first three, the build id and the device."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="fp32", help="the model's hip_precision: fp32, bf16_mix, bf16 or bf16x3")
    ap.add_argument("--workload", default="bm403")
    ap.add_argument("--forwards", type=int, default=50)
    ap.add_argument("--serial", action="store_true")
    ap.add_argument("--batch", type=int, default=0, help="per-GPU batch override (16 = the reference's shipped batch_size)")
    args = ap.parse_args()
    from multistgraph_amd import _lib, build, synthetic as syn
    w = dict(bench.WORKLOADS[args.workload])
    if args.batch:
        w["batch"] = args.batch
    dev = torch.device("cuda:0")
    model, df, cfg = bench.build_model(w, dev, 0)
    model.eval()
    if args.serial:
        _lib.load().matgcn_set_wavefront(0)
    x_np, y_np = syn.make_batch_arrays(w["batch"], w["nodes"], w["out"], 0, feat=2)
    batch = {"X": torch.from_numpy(x_np).to(dev), "y": torch.from_numpy(y_np).to(dev)}
    with torch.no_grad():
        exact = model.predict(batch).clone()
        model.hip_precision = args.precision
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.forwards)]
        for e0, e1 in evs:
            e0.record()
            got = model.predict(batch)
            e1.record()
        torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in evs[3:]) or [float("nan")]
    print(json.dumps({
        "workload": args.workload, "batch": w["batch"], "schedule": "serial" if args.serial else "wave",
        "hip_precision": args.precision, "build": build.source_id(), "device": torch.cuda.get_device_name(dev),
        "forwards": len(ms), "median_ms": statistics.median(ms), "p10_ms": ms[len(ms) // 10],
        "p90_ms": ms[(len(ms) * 9) // 10], "min_ms": ms[0],
        "max_norm_err_vs_f32": float((got - exact).abs().max() / exact.abs().max()),
        "bit_identical_to_f32": bool(torch.equal(got, exact))}), flush=True)


if __name__ == "__main__":
    main()
