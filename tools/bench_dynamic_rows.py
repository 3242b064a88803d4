"""Time the per-sample dynamic Linear (ops.linear_dynamic_rows: two launches)
against the per-batch form (ops.linear_dynamic: five launches), in one process
with the two forms alternating, and score both granularities against the fp32
model.

Per shape ([1024,4096]->512 and [1024,512]->10: fc1 and fc2 of SimpleConvNet
at batch 1024; [512,2048]->1000: ResNet-50's fc; [32,4096]->512: a small
batch), random normal fp32 rows, per-tensor weight scale, bias, caller's
workspace: HIP events around REPS back-to-back calls (device time including
the gaps between a call's own launches), after warm-up of both forms, rounds
alternating.  The same for DynamicQuantConvNet.classify (fc1 -> ReLU -> fc2)
in both granularities at 1024 rows.
Accuracy, on 1024 images of the synthetic 10-class task through the
random-init SimpleConvNet with recalibrated BN statistics (the other tools'
weights): per granularity and at batch 32 and batch 1024, the rms difference
of the logits from the fp32 model's and the argmax agreement with it; and how
far the logits of batch 32 are from those of batch 1024 (the whole model,
convolutions included: the fp32 convolutions may run a different algorithm
per batch size, so only ``classify`` is batch-invariant by construction).
Medians over alternating rounds; min and max are kept so the spread can be
judged.  Prints one JSON line and writes it to --out.

  python tools/bench_dynamic_rows.py --out profiles/dynamic_rows_bench.json
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

REPS = 10
SHAPES = ((1024, 4096, 512), (1024, 512, 10), (512, 2048, 1000), (32, 4096, 512))
N_IMAGES = 1024
BATCHES = (32, 1024)


def _stats(xs, unit):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs),
            "samples": len(xs)}


def alternate(forms, rounds):
    """{name: [us per call]} of the callables in ``forms``: every form warmed,
    then ``rounds`` rounds in which the forms take turns."""
    import torch
    for _ in range(3):
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
    res = {k: _stats(v, "us") for k, v in us.items()}
    res["sample_over_batch"] = res["sample"]["median_us"] / res["batch"]["median_us"]
    return res


def bench_shape(m, k, n, rounds, dev):
    import numpy as np
    import torch
    from qconvnet import ops
    rng = np.random.default_rng(m + k + n)
    x = torch.from_numpy(rng.standard_normal((m, k)).astype(np.float32)).to(dev)
    wq = rng.integers(-127, 128, (n, k), dtype=np.int8)
    w = torch.from_numpy(wq).to(dev)
    wsum = torch.from_numpy(wq.astype(np.int64).sum(1).astype(np.int32)).to(dev)
    s = torch.full((1,), 0.01, device=dev)
    b = torch.from_numpy(rng.standard_normal(n).astype(np.float32)).to(dev)
    yb, ys = (torch.empty((m, n), device=dev) for _ in range(2))
    wb = torch.empty(ops.lib().qcn_linear_dynamic_workspace_size(m, k), dtype=torch.uint8, device=dev)
    ws = torch.empty(ops.lib().qcn_linear_dynamic_rows_workspace_size(m, k), dtype=torch.uint8, device=dev)
    us = alternate({"batch": lambda: ops.linear_dynamic(x, w, s, wsum, b, workspace=wb, out=yb),
                    "sample": lambda: ops.linear_dynamic_rows(x, w, s, wsum, b, workspace=ws, out=ys)}, rounds)
    res = {"shape": [m, k, n], "launches": {"batch": 5, "sample": 2}, "calls_per_sample": REPS}
    res.update(_result(us))
    # normal rows have similar ranges: the two forms' outputs are close, not equal
    res["max_abs_diff_between_forms"] = (yb - ys).abs().max().item()
    return res


def build_models(dev):
    import torch
    from models.baseline_model import synthetic_model
    from models.dynamic_ptq_model import DynamicQuantConvNet
    from qconvnet import data
    fp = synthetic_model(0, torch.from_numpy(data.synthetic_images(64, 1)))
    sd = fp.state_dict()
    return fp.to(dev), {g: DynamicQuantConvNet(sd, device=dev, granularity=g) for g in ("batch", "sample")}


def bench_classify(models, rounds, dev):
    import torch
    feats = torch.randn((1024, 4096), generator=torch.Generator(device=dev).manual_seed(7), device=dev).relu()
    res = {"rows": 1024, "calls_per_sample": REPS}
    res.update(_result(alternate({g: (lambda m=m: m.classify(feats)) for g, m in models.items()}, rounds)))
    return res


def accuracy(fp, models, dev):
    import torch
    from qconvnet import data
    x, _ = data.synthetic_task(N_IMAGES, 2)
    x = torch.from_numpy(x).to(dev)
    with torch.no_grad():
        ref = torch.cat([fp(x[i:i + 256]) for i in range(0, N_IMAGES, 256)])
    res = {"images": N_IMAGES}
    for g, model in models.items():
        logits = {}
        for bs in BATCHES:
            y = torch.cat([model(x[i:i + bs]) for i in range(0, N_IMAGES, bs)])
            logits[bs] = y
            res[f"{g}_batch{bs}"] = {
                "rms_diff_vs_fp32": (y - ref).double().pow(2).mean().sqrt().item(),
                "argmax_agreement_vs_fp32": (y.argmax(1) == ref.argmax(1)).double().mean().item()}
        d = logits[BATCHES[0]] - logits[BATCHES[1]]
        res[f"{g}_batch{BATCHES[0]}_vs_batch{BATCHES[1]}"] = {
            "max_abs_diff": d.abs().max().item(), "rows_not_bit_equal": int((d != 0).any(1).sum().item()),
            "argmax_agreement": (logits[BATCHES[0]].argmax(1) == logits[BATCHES[1]].argmax(1))
            .double().mean().item()}
        # classify alone on the same features: batch-invariant by construction for "sample"
        f = model.features(x)
        c = torch.cat([model.classify(f[i:i + BATCHES[0]].contiguous()) for i in range(0, N_IMAGES, BATCHES[0])])
        res[f"{g}_classify_batch{BATCHES[0]}_vs_batch{BATCHES[1]}_rows_not_bit_equal"] = int(
            (c != model.classify(f)).any(1).sum().item())
    res["ref_rms_logit"] = ref.double().pow(2).mean().sqrt().item()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds per shape (x 10 calls each)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_dynamic_rows: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    fp, models = build_models(dev)
    res = {"device": torch.cuda.get_device_name(0),
           "shapes": [bench_shape(m, k, n, args.rounds, dev) for m, k, n in SHAPES],
           "classify": bench_classify(models, args.rounds, dev),
           "accuracy": accuracy(fp, models, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
