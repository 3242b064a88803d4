"""Raw u8 image input against normalised fp32 input, on one GPU, in one process.

Three measurements at batch 1024 (u8 and fp32 samples alternated, medians and
quartiles reported, HIP events unless stated):

 1. device-resident one-launch convs: time per launch of convnet_convs (fp32
    NCHW in) and convnet_convs_u8 (u8 NHWC in), K back-to-back launches per
    sample;
 2. host-fed throughput: a pinned host batch, a double-buffered H2D copy on a
    side stream, the whole forward on the main stream; images/s for fp32 and
    u8 feeds (host clock around a run that ends in a synchronise), and the
    H2D rate of a plain pinned copy on this box;
 3. normalize_u8 at 1024 x 224 x 224: time per launch against its 15 B/pixel
    HBM bound (3 B read, 12 B written).

The model is the untrained synthetic SimpleConvNet (timing does not depend on
the weights; static int8, fast epilogue).  Prints one JSON line and writes it
to --out.

  python tools/bench_u8_input.py --out profiles/u8_input_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "convnet-quantization_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_BPS = 8.0e12        # MI355X HBM3E, spec
HBM_COPY_BPS = 6.29e12       # measured float4 copy rate on the same part


def summary(v, unit):
    q = statistics.quantiles(v, n=4)
    return {f"median_{unit}": statistics.median(v), f"q1_{unit}": q[0], f"q3_{unit}": q[2],
            f"iqr_{unit}": q[2] - q[0], f"min_{unit}": min(v), f"max_{unit}": max(v), "samples": len(v)}


def timed_us(fn, reps):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def alternate(fns, warmup, iters, reps):
    """{name: per-launch times in us}: one sample of each fn in turn, `iters` rounds."""
    import torch
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            out[k].append(timed_us(fn, reps))
    return out


def build_model(dev):
    import torch
    from models.baseline_model import synthetic_model
    from qconvnet import data
    from qconvnet.qmodel import QuantizedConvNet, build_qspec, calibrate, fold_state_dict
    calib = torch.from_numpy(data.synthetic_images(64, 1))
    fp = synthetic_model(0, calib)
    folded = fold_state_dict(fp.state_dict())
    ranges = calibrate(folded, [calib], "cpu", mode="static")
    return QuantizedConvNet(build_qspec(folded, ranges, "static"), dev)


def u8_batch(n, hw, seed):
    import numpy as np
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8))


def host_fed(model, host, steps):
    """images/s of `steps` forwards fed from the pinned host batch through two
    device buffers: the copy of batch k+1 (side stream) overlaps the forward of
    batch k (main stream)."""
    import torch
    dev = model.device
    main = torch.cuda.current_stream(dev)
    side = torch.cuda.Stream(dev)
    bufs = [torch.empty_like(host, device=dev) for _ in range(2)]
    copied = [torch.cuda.Event() for _ in range(2)]
    used = [torch.cuda.Event() for _ in range(2)]
    for e in used:
        e.record(main)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        i = k & 1
        with torch.cuda.stream(side):
            side.wait_event(used[i])          # the forward that read this buffer is done
            bufs[i].copy_(host, non_blocking=True)
            copied[i].record(side)
        main.wait_event(copied[i])
        model.run(bufs[i])
        used[i].record(main)
    torch.cuda.synchronize()
    return host.shape[0] * steps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--iters", type=int, default=40, help="timed samples per variant")
    ap.add_argument("--reps", type=int, default=20, help="back-to-back launches per sample (K)")
    ap.add_argument("--fed-steps", type=int, default=300)
    ap.add_argument("--fed-trials", type=int, default=9)
    ap.add_argument("--norm-batch", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters: at least 20 timed samples")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_u8_input: no GPU (there is no CPU fallback to time)")
    from qconvnet import data, ops, quant as Q

    dev = torch.device("cuda:0")
    n = args.batch
    model = build_model(dev)
    x8_host = u8_batch(n, 32, 0)
    xf_host = Q.expand_u8(x8_host, Q.normalize_table(data.CIFAR_MEAN, data.CIFAR_STD))
    x8, xf = x8_host.to(dev), xf_host.to(dev)
    res = {"device": torch.cuda.get_device_name(0), "batch": n,
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count}

    # the two feeds compute the same logits (checked here, at the timed size)
    want = model.run(xf).clone()
    if not torch.equal(model.run(x8), want):
        raise SystemExit("bench_u8_input: u8 and fp32 logits differ")
    res["kernels"] = list(model.kernel_names(x8.shape))

    # ---- 1. device-resident one-launch convs
    layers = ops.conv_layers(model.L, model.in_zp)
    b = model.buffers(n)
    head = model._head(n, False)
    a6 = b["a6k"] if head else b["a6"]

    def convs_f32():
        if not ops.convnet_convs(xf, model.in_scale, model.in_zp, layers, b["a2"], b["a4"], a6, kmajor=head):
            raise SystemExit("bench_u8_input: the one-launch convs do not take this batch")

    def convs_u8():
        if not ops.convnet_convs_u8(x8, model.qlut, model.in_zp, layers, b["a2"], b["a4"], a6, kmajor=head):
            raise SystemExit("bench_u8_input: the one-launch convs do not take this batch")

    t = alternate({"fp32": convs_f32, "u8": convs_u8}, args.warmup, args.iters, args.reps)
    f, u = summary(t["fp32"], "us"), summary(t["u8"], "us")
    res["convs_one_launch"] = {
        "launches_per_sample": args.reps, "fp32": f, "u8": u,
        "u8_minus_fp32_median_us": u["median_us"] - f["median_us"],
        "u8_above_fp32_by_more_than_fp32_iqr": u["median_us"] - f["median_us"] > f["iqr_us"],
        "input_bytes": {"fp32": xf.numel() * 4, "u8": x8.numel()}}

    # ---- 2. host-fed throughput
    pinned = {"fp32": xf_host.pin_memory(), "u8": x8_host.pin_memory()}
    big = torch.empty(64 << 20, dtype=torch.uint8).pin_memory()
    big_d = torch.empty_like(big, device=dev)
    h2d = [big.numel() / timed_us(lambda: big_d.copy_(big, non_blocking=True), 4) * 1e-3
           for _ in range(args.warmup + 10)][args.warmup:]
    for k in pinned:
        host_fed(model, pinned[k], 20)
    rates = {"fp32": [], "u8": []}
    for _ in range(args.fed_trials):
        for k in rates:
            rates[k].append(host_fed(model, pinned[k], args.fed_steps))
    fed = {k: summary(v, "img_s") for k, v in rates.items()}
    for k in fed:
        bytes_per_img = pinned[k].numel() * pinned[k].element_size() / n
        fed[k]["bytes_per_image"] = bytes_per_img
        fed[k]["h2d_GBps_at_median"] = fed[k]["median_img_s"] * bytes_per_img * 1e-9
    res["host_fed"] = {"steps_per_trial": args.fed_steps, "fp32": fed["fp32"], "u8": fed["u8"],
                       "u8_over_fp32": fed["u8"]["median_img_s"] / fed["fp32"]["median_img_s"],
                       "h2d_pinned_64MiB_GBps": summary(h2d, "GBps")}

    # ---- 3. normalize_u8 at norm_batch x 224 x 224
    nb = args.norm_batch
    img = u8_batch(nb, 224, 1).to(dev)
    ntab = Q.normalize_table(data.IMAGENET_MEAN, data.IMAGENET_STD).to(dev)
    out = torch.empty((nb, 3, 224, 224), dtype=torch.float32, device=dev)
    tn = alternate({"normalize_u8": lambda: ops.normalize_u8(img, ntab, out=out)}, args.warmup, args.iters, 5)
    s = summary(tn["normalize_u8"], "us")
    nbytes = nb * 224 * 224 * 15
    res["normalize_u8"] = {"shape": [nb, 224, 224, 3], "bytes": nbytes, "launches_per_sample": 5, **s,
                           "GBps_at_median": nbytes / s["median_us"] * 1e-3,
                           "bound_us_at_8.0TBps_spec": nbytes / HBM_PEAK_BPS * 1e6,
                           "bound_us_at_6.29TBps_copy": nbytes / HBM_COPY_BPS * 1e6,
                           "share_of_spec_bound": nbytes / HBM_PEAK_BPS * 1e6 / s["median_us"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
