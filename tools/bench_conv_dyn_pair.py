"""Time the dynamic int8 conv pairs (ops.conv3x3_dyn_pair) against
the two ops.conv3x3_dyn calls they replace, in one process with the forms
alternating (the protocol of tools/bench_conv_dyn.py: HIP events around REPS
back-to-back calls after warm-up of every form; median, min and max of the
rounds).

``features()`` of DynamicQuantConvNet(body="int8") with pairs=False (min/max +
six launches) and pairs=True (min/max, conv1, conv2 and two pair launches) at
batch 32, 256 and 1024; conv3 + conv4 and conv5 + conv6 alone at batch 1024
(bias + ReLU on both layers, the pool on the second; a ready per-image range
record in, the output's range record out).  The yardstick of every ratio is
the two-call form of the same run.
Reproducibility: logits of 1024 images with granularity="sample" at batch 32
and at batch 1024 with pairs=True: rows that are not bit-equal, and rows that
differ from pairs=False.
Prints one JSON line and writes it to --out.

  python tools/bench_conv_dyn_pair.py --out profiles/conv_dyn_pair_bench.json
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


def _result(us):
    res = {k: _stats(v) for k, v in us.items()}
    res["pair_over_two_calls"] = res["pair"]["median_us"] / res["two_calls"]["median_us"]
    return res


def bench_features(models, rounds, dev):
    import torch
    out = []
    for n in BATCHES:
        x = torch.randn((n, 3, 32, 32), generator=torch.Generator(device=dev).manual_seed(n), device=dev)
        res = {"batch": n, "calls_per_sample": REPS}
        res.update(_result(alternate({k: (lambda m=m: m.features(x)) for k, m in models.items()}, rounds)))
        out.append(res)
    return out


def bench_pairs(model, rounds, dev):
    import torch
    from models.baseline_model import CONV_TABLE
    from qconvnet import ops
    out, n = [], LAYER_BATCH
    for i, hw in ((2, 16), (4, 8)):
        cin, cmid, cout = CONV_TABLE[i][0], CONV_TABLE[i][1], CONV_TABLE[i + 1][1]
        la, lb = (ops.DynLayer(q[0], q[1], q[2], CONV_TABLE[j][1], bias=q[3], relu=True)
                  for j, q in ((i, model.qconvs[i]), (i + 1, model.qconvs[i + 1])))
        x = torch.randn((n, hw, hw, cin), generator=torch.Generator(device=dev).manual_seed(i), device=dev)
        stats = ops.image_minmax(x)

        def two_calls():
            t, st = ops.conv3x3_dyn(x, stats, la.packed, la.wsum, la.w_scale, cmid, bias=la.bias, relu=True)
            return ops.conv3x3_dyn(t, st, lb.packed, lb.wsum, lb.w_scale, cout, bias=lb.bias, relu=True, pool=True)
        res = {"pair": f"conv{i + 1}+conv{i + 2}", "shape": [n, hw, hw, cin, cmid, cout], "calls_per_sample": REPS}
        res.update(_result(alternate(
            {"two_calls": two_calls, "pair": lambda: ops.conv3x3_dyn_pair(x, stats, la, lb, pool=True)}, rounds)))
        # the intermediate activation's fp32 store and load that the pair does not do
        res["hbm_bytes_not_moved"] = 2 * 4 * n * hw * hw * cmid
        out.append(res)
    return out


def reproducibility(models, dev):
    import torch
    from qconvnet import data
    x = torch.from_numpy(data.synthetic_task(N_IMAGES, 2)[0]).to(dev)
    small = torch.cat([models["pair"](x[i:i + 32]) for i in range(0, N_IMAGES, 32)])
    whole = models["pair"](x)
    return {"images": N_IMAGES, "granularity": "sample",
            "pairs_batch32_vs_batch1024_rows_not_bit_equal": int((small != whole).any(1).sum().item()),
            "pairs_vs_two_calls_rows_not_bit_equal": int((whole != models["two_calls"](x)).any(1).sum().item())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=10, help="alternating rounds per case")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_conv_dyn_pair: no GPU (there is no CPU fallback to time)")
    from models.dynamic_ptq_model import DynamicQuantConvNet
    dev = torch.device("cuda:0")
    sd = state_dict()
    models = {k: DynamicQuantConvNet(sd, device=dev, granularity="sample", body="int8", pairs=p)
              for k, p in (("two_calls", False), ("pair", True))}
    res = {"device": torch.cuda.get_device_name(0),
           "features": bench_features(models, args.rounds, dev),
           "pairs": bench_pairs(models["pair"], args.rounds, dev),
           "reproducibility": reproducibility(models, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
