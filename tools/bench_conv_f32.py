"""Time the deterministic fp32 conv body of the dynamic models
(DynamicQuantConvNet(body="hip"): six ops.conv3x3_f32 launches) against the
torch body (F.conv2d through MIOpen, + ReLU and max-pool launches), in one
process with the two forms alternating.

``features()`` of both bodies at batch 32, 256 and 1024, and each of the six
layers alone at batch 1024 (conv + bias + ReLU [+ pool]; the torch form is
F.conv2d, F.relu, F.max_pool2d on NCHW): HIP events around REPS back-to-back
calls after warm-up of both forms, rounds alternating; median, min and max.
Per layer, the HIP kernel's share of the fp32 matrix peak, 2 * 9 * cin * cout
* h * w flop per image over 256 CUs x 256 flop/clock x 2.4 GHz = 157.3
TFLOP/s (the clock held during the run is not measured here; the time is the
event time of the calls, not a kernel trace).
Reproducibility: logits of 1024 images with granularity="sample" at batch 32
and at batch 1024, per body: rows that are not bit-equal.
Prints one JSON line and writes it to --out.

  python tools/bench_conv_f32.py --out profiles/conv_f32_bench.json
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

REPS = 5
BATCHES = (32, 256, 1024)
LAYER_BATCH = 1024
N_IMAGES = 1024
PEAK_FP32_MATRIX = 256 * 256 * 2.4e9   # flop/s


def _stats(xs):
    return {"median_us": statistics.median(xs), "min_us": min(xs), "max_us": max(xs), "samples": len(xs)}


def alternate(forms, rounds):
    """{name: [us per call]}: every form warmed, then ``rounds`` rounds in
    which the forms take turns."""
    import torch
    for _ in range(2):
        for fn in forms.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in forms}
    for _ in range(rounds):
        for k, fn in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / REPS)
    return us


def _result(us):
    res = {k: _stats(v) for k, v in us.items()}
    res["hip_over_torch"] = res["hip"]["median_us"] / res["torch"]["median_us"]
    return res


def build_models(dev, granularity="sample"):
    import torch
    from models.baseline_model import synthetic_model
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from qconvnet import data
    sd = synthetic_model(0, torch.from_numpy(data.synthetic_images(64, 1))).state_dict()
    return {b: DynamicQuantConvNet(sd, device=dev, granularity=granularity, body=b) for b in ("torch", "hip")}


def bench_features(models, rounds, dev):
    import torch
    out = []
    for n in BATCHES:
        x = torch.randn((n, 3, 32, 32), generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        res = {"batch": n, "calls_per_sample": REPS}
        res.update(_result(alternate({b: (lambda m=m: m.features(x)) for b, m in models.items()}, rounds)))
        out.append(res)
    return out


def bench_layers(models, rounds, dev):
    import torch
    import torch.nn.functional as F
    from models.baseline_model import CONV_TABLE
    from qconvnet import ops
    out, hw, n = [], 32, LAYER_BATCH
    for i, (cin, cout, pool) in enumerate(CONV_TABLE):
        w, b, _ = models["torch"].convs[i]
        wp = models["hip"].packed[i][0]
        g = torch.Generator(device=dev).manual_seed(i)
        xt = torch.randn((n, cin, hw, hw), generator=g, device=dev)
        xh = xt.permute(0, 2, 3, 1).contiguous()

        def torch_form():
            y = F.relu(F.conv2d(xt, w, b, padding=1))
            return F.max_pool2d(y, 2, 2) if pool else y
        res = {"layer": f"conv{i + 1}", "shape": [n, cin, cout, hw, hw, int(pool)], "calls_per_sample": REPS}
        res.update(_result(alternate({
            "torch": torch_form,
            "hip": lambda: ops.conv3x3_f32(xh, wp, cout, bias=b, relu=True, pool=pool)}, rounds)))
        flop = 2.0 * 9 * cin * cout * hw * hw * n
        res["hip_fraction_of_fp32_matrix_peak_at_2p4GHz"] = flop / (res["hip"]["median_us"] * 1e-6) / PEAK_FP32_MATRIX
        # NCHW torch result against the NHWC kernel result (orders of summation differ)
        res["max_abs_diff_between_forms"] = (torch_form().permute(0, 2, 3, 1) - ops.conv3x3_f32(
            xh, wp, cout, bias=b, relu=True, pool=pool)).abs().max().item()
        out.append(res)
        if pool:
            hw //= 2
    return out


def reproducibility(models, dev):
    import torch
    from qconvnet import data
    x = torch.from_numpy(data.synthetic_task(N_IMAGES, 2)[0]).to(dev)
    res = {"images": N_IMAGES, "granularity": "sample"}
    for b, m in models.items():
        small = torch.cat([m(x[i:i + 32]) for i in range(0, N_IMAGES, 32)])
        res[f"{b}_batch32_vs_batch1024_rows_not_bit_equal"] = int((small != m(x)).any(1).sum().item())
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10, help="alternating rounds per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_f32: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    models = build_models(dev)
    res = {"device": torch.cuda.get_device_name(0),
           "features": bench_features(models, args.rounds, dev),
           "layers": bench_layers(models, args.rounds, dev),
           "reproducibility": reproducibility(models, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
