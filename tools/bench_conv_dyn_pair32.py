"""Time the 32 x 32 dynamic int8 conv pair (ops.conv3x3_dyn_pair32)
against the paths it replaces, in one process with the forms alternating (the
protocol of tools/bench_conv_dyn_pair.py: HIP events around REPS back-to-back
calls after warm-up of every form; median, min and max of the rounds).

``features()`` of DynamicQuantConvNet(body="int8") with pairs=True (min/max,
conv1, conv2 and two pair launches) and pairs="all" (min/max and three pair
launches) at batch 32, 256 and 1024, with pairs=False beside them; conv1 +
conv2 alone at batch 1024 (NCHW images in, bias + ReLU on both layers, the pool
on the second; a ready per-image range record in, the output's range record
out) as two ops.conv3x3_dyn calls and as one pair32 call.  The yardstick of
every ratio is the older path in the same run.
Reproducibility: logits of 1024 images with granularity="sample" at batch 32
and at batch 1024 with pairs="all": rows that are not bit-equal, and rows that
differ from pairs=False.
Prints one JSON line and writes it to --out.

  python tools/bench_conv_dyn_pair32.py --out profiles/conv_dyn_pair32_bench.json
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

from bench_conv_dyn import state_dict  # noqa: E402
from bench_conv_f32 import BATCHES, LAYER_BATCH, N_IMAGES, REPS, _stats, alternate  # noqa: E402


def bench_features(models, rounds, dev):
    import torch
    out = []
    for n in BATCHES:
        x = torch.randn((n, 3, 32, 32), generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        res = {"batch": n, "calls_per_sample": REPS}
        res.update({k: _stats(v) for k, v in
                    alternate({k: (lambda m=m: m.features(x)) for k, m in models.items()}, rounds).items()})
        res["all_over_true"] = res["pairs_all"]["median_us"] / res["pairs_true"]["median_us"]
        res["all_over_false"] = res["pairs_all"]["median_us"] / res["pairs_false"]["median_us"]
        out.append(res)
    return out


def bench_pair32(model, rounds, dev):
    import torch
    from models.baseline_model import CONV_TABLE
    from qconvnet import ops
    n, hw = LAYER_BATCH, 32
    cin, cmid, cout = CONV_TABLE[0][0], CONV_TABLE[0][1], CONV_TABLE[1][1]
    la, lb = (ops.DynLayer(q[0], q[1], q[2], CONV_TABLE[j][1], bias=q[3], relu=True)
              for j, q in enumerate(model.qconvs[:2]))
    x = torch.randn((n, cin, hw, hw), generator=torch.Generator(device=dev).manual_seed(1), device=dev)
    stats = ops.image_minmax(x)

    def two_calls():
        t, st = ops.conv3x3_dyn(x, stats, la.packed, la.wsum, la.w_scale, cmid, bias=la.bias, relu=True, x_nchw=True)
        return ops.conv3x3_dyn(t, st, lb.packed, lb.wsum, lb.w_scale, cout, bias=lb.bias, relu=True, pool=True)
    res = {"pair": "conv1+conv2", "shape": [n, hw, hw, cin, cmid, cout], "calls_per_sample": REPS}
    res.update({k: _stats(v) for k, v in alternate(
        {"two_calls": two_calls,
         "pair32": lambda: ops.conv3x3_dyn_pair32(x, stats, la, lb, pool=True, x_nchw=True)}, rounds).items()})
    res["pair32_over_two_calls"] = res["pair32"]["median_us"] / res["two_calls"]["median_us"]
    # the intermediate activation's fp32 store and load that the pair does not do
    res["hbm_bytes_not_moved"] = 2 * 4 * n * hw * hw * cmid
    return res


def reproducibility(models, dev):
    import torch
    from qconvnet import data
    x = torch.from_numpy(data.synthetic_task(N_IMAGES, 2)[0]).to(dev)
    small = torch.cat([models["pairs_all"](x[i:i + 32]) for i in range(0, N_IMAGES, 32)])
    whole = models["pairs_all"](x)
    return {"images": N_IMAGES, "granularity": "sample",
            "all_batch32_vs_batch1024_rows_not_bit_equal": int((small != whole).any(1).sum().item()),
            "all_vs_pairs_false_rows_not_bit_equal": int((whole != models["pairs_false"](x)).any(1).sum().item())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10, help="alternating rounds per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_dyn_pair32: no GPU (there is no CPU fallback to time)")
    from models.dynamic_ptq_model import DynamicQuantConvNet
    dev = torch.device("cuda:0")
    sd = state_dict()
    models = {k: DynamicQuantConvNet(sd, device=dev, granularity="sample", body="int8", pairs=p)
              for k, p in (("pairs_false", False), ("pairs_true", True), ("pairs_all", "all"))}
    res = {"device": torch.cuda.get_device_name(0),
           "features": bench_features(models, args.rounds, dev),
           "pair32": bench_pair32(models["pairs_all"], args.rounds, dev),
           "reproducibility": reproducibility(models, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
