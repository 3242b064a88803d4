"""Time the dynamically quantized int8 conv body of the dynamic models
(DynamicQuantConvNet(body="int8"): one ops.image_minmax and six
ops.conv3x3_dyn launches) against body="hip" (six ops.conv3x3_f32 launches)
and body="torch" (MIOpen), in one process with the forms alternating.

``features()`` of the three bodies at batch 32, 256 and 1024, and each of the
six layers alone at batch 1024 (conv + bias + ReLU [+ pool]; the int8 form
reads a ready per-image range record and writes its output's): HIP events
around REPS back-to-back calls after warm-up of every form, rounds
alternating; median, min and max.  Per layer, the int8 call's share of the
int8 matrix peak, 2 * 9 * cin * cout * h * w op per image over 256 CUs x 4
SIMDs x 2048 op/clock x 2.4 GHz = 5.03 POP/s (the clock held during the run is
not measured here; the time is the event time of the calls, not a kernel
trace).
Accuracy (reported, not asserted): rms and max error of the logits against
the fp32 CPU model on 256 synthetic images, for body="int8", body="hip", both
with granularity="sample", and body="torch" with granularity="batch".
Reproducibility: logits of 1024 images with granularity="sample" at batch 32
and at batch 1024 with body="int8": rows that are not bit-equal.
Prints one JSON line and writes it to --out.

  python tools/bench_conv_dyn.py --out profiles/conv_dyn_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "convnet-quantization_amd"), ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from bench_conv_f32 import BATCHES, LAYER_BATCH, N_IMAGES, REPS, _stats, alternate  # noqa: E402

PEAK_INT8_MATRIX = 256 * 4 * 2048 * 2.4e9   # op/s
BODIES = ("torch", "hip", "int8")


def _result(us):
    res = {k: _stats(v) for k, v in us.items()}
    res["int8_over_hip"] = res["int8"]["median_us"] / res["hip"]["median_us"]
    res["int8_over_torch"] = res["int8"]["median_us"] / res["torch"]["median_us"]
    return res


def state_dict():
    import torch
    from models.baseline_model import synthetic_model
    from qconvnet import data
    return synthetic_model(0, torch.from_numpy(data.synthetic_images(64, 1))).state_dict()


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
        wf = models["hip"].packed[i][0]
        wp, wsum, s_w, _, _ = models["int8"].qconvs[i]
        g = torch.Generator(device=dev).manual_seed(i)
        xt = torch.randn((n, cin, hw, hw), generator=g, device=dev)
        xh = xt.permute(0, 2, 3, 1).contiguous()
        stats = ops.image_minmax(xh)

        def torch_form():
            y = F.relu(F.conv2d(xt, w, b, padding=1))
            return F.max_pool2d(y, 2, 2) if pool else y
        res = {"layer": f"conv{i + 1}", "shape": [n, cin, cout, hw, hw, int(pool)], "calls_per_sample": REPS}
        res.update(_result(alternate({
            "torch": torch_form,
            "hip": lambda: ops.conv3x3_f32(xh, wf, cout, bias=b, relu=True, pool=pool),
            "int8": lambda: ops.conv3x3_dyn(xh, stats, wp, wsum, s_w, cout, bias=b, relu=True, pool=pool)},
            rounds)))
        op = 2.0 * 9 * cin * cout * hw * hw * n
        res["int8_fraction_of_int8_matrix_peak_at_2p4GHz"] = op / (res["int8"]["median_us"] * 1e-6) / PEAK_INT8_MATRIX
        out.append(res)
        if pool:
            hw //= 2
    return out


def accuracy(sd, dev):
    """rms / max error of the logits against the fp32 CPU model."""
    import torch
    from models.baseline_model import SimpleConvNet
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from qconvnet import data
    x = torch.from_numpy(data.synthetic_images(256, 41))
    fp = SimpleConvNet()
    fp.load_state_dict(sd)
    fp.eval()
    with torch.no_grad():
        want = fp(x)
    res = {"images": 256, "max_abs_logit": want.abs().max().item()}
    for body, gran in (("int8", "sample"), ("hip", "sample"), ("torch", "batch")):
        d = DynamicQuantConvNet(sd, device=dev, granularity=gran, body=body)(x.to(dev)).cpu() - want
        res[f"{body}_{gran}"] = {"rms": d.pow(2).mean().sqrt().item(), "max": d.abs().max().item()}
    return res


def reproducibility(model, dev):
    import torch
    from qconvnet import data
    x = torch.from_numpy(data.synthetic_task(N_IMAGES, 2)[0]).to(dev)
    small = torch.cat([model(x[i:i + 32]) for i in range(0, N_IMAGES, 32)])
    return {"images": N_IMAGES, "granularity": "sample",
            "int8_batch32_vs_batch1024_rows_not_bit_equal": int((small != model(x)).any(1).sum().item())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10, help="alternating rounds per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_dyn: no GPU (there is no CPU fallback to time)")
    from models.dynamic_ptq_model import DynamicQuantConvNet
    dev = torch.device("cuda:0")
    sd = state_dict()
    models = {b: DynamicQuantConvNet(sd, device=dev, granularity="sample", body=b) for b in BODIES}
    res = {"device": torch.cuda.get_device_name(0),
           "features": bench_features(models, args.rounds, dev),
           "layers": bench_layers(models, args.rounds, dev),
           "accuracy": accuracy(sd, dev),
           "reproducibility": reproducibility(models["int8"], dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
