"""Raw u8 images into the ResNet stem, on one GPU, in one process.

At 512 x 224 x 224 (samples of the variants alternated, medians and quartiles
from HIP events, K back-to-back launches per sample):

 (a) stem_fused on a resident fp32 NCHW batch;
 (b) normalize_u8 + stem_fused: the u8 path before the stem read the bytes;
 (c) stem_fused_u8 on the u8 NHWC batch;
 (d) the whole QuantizedResNet ResNet-50 forward (two interleaved stream
     slices, as the model call runs it at this batch) fed u8: the batch handed
     to the model as it is (the u8 stem), and forced onto the old path
     (normalize_u8 into a fresh fp32 tensor, then the fp32-fed forward, which
     is what the model did with a u8 batch before the stem read the bytes).

The model is the untrained synthetic ResNet-50 (timing does not depend on the
weights).  The variants' results are checked equal first, at the timed size.
Prints one JSON line and writes it to --out.

  python tools/bench_u8_stem.py --out profiles/u8_stem_bench.json
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
    """{name: per-call times in us}: one sample of each fn in turn, `iters` rounds."""
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


def u8_batch(n, hw, seed):
    import numpy as np
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    return torch.from_numpy(rng.integers(0, 256, (n, hw, hw, 3), dtype=np.uint8))


def build_model(dev, calib_images):
    import torch
    from models.resnet import synthetic_images, synthetic_resnet
    from qconvnet.resnet import quantize_resnet
    fp = synthetic_resnet(0, device="cpu", calib_images=calib_images)
    calib = [torch.from_numpy(synthetic_images(calib_images, 1))]
    return quantize_resnet(fp, calib, dev, per_channel=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30, help="timed samples per variant")
    ap.add_argument("--reps", type=int, default=10, help="back-to-back stem launches per sample (K)")
    ap.add_argument("--forward-reps", type=int, default=3, help="back-to-back forwards per sample")
    ap.add_argument("--calib-images", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters: at least 20 timed samples")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_u8_stem: no GPU (there is no CPU fallback to time)")
    from qconvnet import ops

    dev = torch.device("cuda:0")
    n, hw = args.batch, 224
    model = build_model(dev, args.calib_images)
    x8 = u8_batch(n, hw, 0).to(dev)
    xf = ops.normalize_u8(x8, model.ntab)          # resident fp32 input of (a)
    xf_b = torch.empty_like(xf)                      # (b) writes its own expansion
    y = torch.empty((n, hw // 4, hw // 4, 64), dtype=torch.uint8, device=dev)
    s, zp, stem, qlut, ntab = model.in_scale, model.in_zp, model.stem, model.qlut, model.ntab
    if not model._stem_fusable(x8):
        raise SystemExit("bench_u8_stem: the fused stem does not take this model")
    res = {"device": torch.cuda.get_device_name(0), "batch": n, "hw": hw,
           "cus": torch.cuda.get_device_properties(dev).multi_processor_count,
           "input_bytes": {"fp32": xf.numel() * 4, "u8": x8.numel()}}

    # ---- the stem alone: (a), (b), (c) write the same bytes
    def a_f32():
        ops.stem_fused(xf, s, zp, stem, out=y)

    def b_norm_f32():
        ops.normalize_u8(x8, ntab, out=xf_b)
        ops.stem_fused(xf_b, s, zp, stem, out=y)

    def c_u8():
        ops.stem_fused_u8(x8, qlut, zp, stem, out=y)

    want = ops.stem_fused(xf, s, zp, stem)
    for fn in (b_norm_f32, c_u8):
        y.zero_()
        fn()
        if not torch.equal(y, want):
            raise SystemExit(f"bench_u8_stem: {fn.__name__} differs from the fp32-fed stem")
    t = alternate({"a": a_f32, "b": b_norm_f32, "c": c_u8}, args.warmup, args.iters, args.reps)
    a, b, c = (summary(t[k], "us") for k in "abc")
    res["stem"] = {
        "launches_per_sample": args.reps,
        "a_stem_fused_fp32_resident": a, "b_normalize_u8_plus_stem_fused": b, "c_stem_fused_u8": c,
        "c_minus_b_median_us": c["median_us"] - b["median_us"],
        "c_below_b": c["median_us"] < b["median_us"],
        "c_minus_a_median_us": c["median_us"] - a["median_us"],
        "c_above_a_by_more_than_a_iqr": c["median_us"] - a["median_us"] > a["iqr_us"]}

    # ---- (d) the whole forward fed u8
    def new():
        return model.run_streams(x8, 2)

    def old():
        return model.run_streams(ops.normalize_u8(x8, ntab), 2)

    want = model.run_streams(xf, 2).clone()
    if not (torch.equal(new(), want) and torch.equal(old(), want)):
        raise SystemExit("bench_u8_stem: u8 and fp32 logits differ")
    t = alternate({"u8_stem": new, "normalize_u8": old}, args.warmup, args.iters, args.forward_reps)
    fn_, fo = summary(t["u8_stem"], "us"), summary(t["normalize_u8"], "us")
    d = fn_["median_us"] - fo["median_us"]
    res["forward_u8_fed"] = {
        "forwards_per_sample": args.forward_reps, "streams": 2, "u8_stem": fn_, "normalize_u8": fo,
        "u8_stem_minus_normalize_u8_median_us": d,
        "img_s_at_median": {"u8_stem": n / fn_["median_us"] * 1e6, "normalize_u8": n / fo["median_us"] * 1e6},
        "u8_stem_slower_by_more_than_both_iqrs": d > fn_["iqr_us"] + fo["iqr_us"]}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
