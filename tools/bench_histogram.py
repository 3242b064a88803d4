"""Time qcn_histc_f32 against qcn_minmax_f32 on the same tensor.

The min/max kernel is the existing observer kernel that reads the same bytes,
so the ratio says what a histogram calibration step costs over a MinMax one.
Tensor: conv1's output at batch 256, 256 x 64 x 32 x 32 fp32 (67 MB), once as
a normal input and once as its ReLU (the hot-bin case: half the elements are
exactly the range minimum).  HIP events around 10 back-to-back launches,
warm-up, median of the samples.  Prints one JSON line and writes it to --out.

  python tools/bench_histogram.py --out profiles/histogram_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "convnet-quantization_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)


REPS = 10   # launches per timed sample, back to back, so the queue never runs dry


def _time(fn, warmup, iters):
    """Per-launch time: `iters` samples, each REPS launches between two events."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / REPS)
    return {"median_us": statistics.median(ms) * 1e3, "min_us": min(ms) * 1e3,
            "max_us": max(ms) * 1e3, "samples": iters, "launches_per_sample": REPS}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shape", type=int, nargs=4, default=[256, 64, 32, 32])
    ap.add_argument("--bins", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters: at least 20 timed samples")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_histogram: no GPU (there is no CPU fallback to time)")
    from qconvnet import ops

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    normal = torch.randn(*args.shape, generator=gen).to(dev)
    inputs = {"normal": normal, "relu": torch.relu(normal)}
    hist = torch.zeros(args.bins, dtype=torch.int32, device=dev)
    res = {"shape": args.shape, "bins": args.bins, "bytes": normal.numel() * 4,
           "device": torch.cuda.get_device_name(0)}
    for name, x in inputs.items():
        obs = ops.MinMaxObserver(dev)
        mm = _time(lambda: obs(x), args.warmup, args.iters)
        hc = _time(lambda: ops.histc(x, obs.state, args.bins, out=hist), args.warmup, args.iters)
        # the timed launches all added into `hist`: a check that they counted
        hist.zero_()
        ops.histc(x, obs.state, args.bins, out=hist)
        counted = int(hist.cpu().numpy().view("uint32").astype("int64").sum())
        if counted != x.numel():
            raise SystemExit(f"bench_histogram: counted {counted} of {x.numel()} elements")
        res[name] = {"minmax": mm, "histc": hc,
                     "histc_over_minmax": hc["median_us"] / mm["median_us"],
                     "histc_GBps": res["bytes"] / hc["median_us"] * 1e-3,
                     "minmax_GBps": res["bytes"] / mm["median_us"] * 1e-3}
        hist.zero_()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
