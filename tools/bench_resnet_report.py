"""Time the fp32-against-fp32 error kernel (qcn_qerror_f32_f32) against the
torch-op composition it replaces, and a whole ResNet-50 error report against
the same walk scored by torch, in one process with the paths alternating.

Per activation (fp32 NCHW reference on the device, fp32 activation; the block
outputs of ResNet-50 at batch 32 and a pooled vector):
  torch        the same statistics from torch ops: permute the NHWC activation
               to NCHW, subtract, square, |.|, the per-channel reductions
               (float64 accumulators), the compare, the max — several
               full-size fp32 temporaries;
  kernel_nhwc  qcn_qerror_f32_f32 with the activation NHWC (read straight from
               memory), the main launch and the finishing launch;
  kernel_nchw  the same with the activation NCHW (both tensors through the LDS
               transpose) — the alternative way of feeding y, for DESIGN §21.
All are timed with HIP events around REPS back-to-back calls after warm-up,
rounds alternating.  The kernel's bytes / time is reported against 8 bytes per
element (x and y read once) and beside the measured HBM copy rate.
End to end, 64 synthetic 224 x 224 images through CustomQuantizedResNet50 in
both modes at batch 32: layer_report against the same walk (layer_pairs: the
fp32 net and the kept int8 forward) scored by the torch compositions, host
clock around a call that ends in its one sync.  Medians over alternating
rounds; min and max are kept so the spread can be judged.  Nothing is gated on
these times.  Prints one JSON line and writes it to --out.

  python tools/bench_resnet_report.py --out profiles/resnet_report_bench.json
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "convnet-quantization_amd"), ROOT, os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

REPS = 5
SHAPES = (("layer1", (32, 256, 56, 56)), ("layer3", (32, 1024, 14, 14)), ("layer4", (32, 2048, 7, 7)),
          ("pool", (512, 2048)))
N_IMAGES, BATCH = 64, 32
HBM_COPY_TBS = 6.29     # measured float4 copy rate of the MI355X (the achievable roof)


def _stats(xs, unit):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs),
            "samples": len(xs)}


def torch_score_f32(x, y, acc=None):
    """The statistics of ops.qerror_f32 from torch ops: (counts [c,3] int64
    with the max as fp32 bits, sums [c,4] float64), added into ``acc``.
    ``y`` is NHWC for a 4-D ``x``."""
    import torch
    dims = (0, 2, 3) if x.dim() == 4 else (0,)
    yn = y.permute(0, 3, 1, 2) if x.dim() == 4 else y
    e = x - yn
    counts = torch.stack([
        torch.full((x.shape[1],), x.numel() // x.shape[1], dtype=torch.int64, device=x.device),
        (x != yn).sum(dims), e.abs().amax(dims).view(torch.int32).to(torch.int64)], 1)
    sums = torch.stack([(x * x).sum(dims, dtype=torch.float64), (e * e).sum(dims, dtype=torch.float64),
                        e.abs().sum(dims, dtype=torch.float64), e.sum(dims, dtype=torch.float64)], 1)
    if acc is None:
        return counts, sums
    acc[0][:, :2] += counts[:, :2]
    acc[0][:, 2] = torch.maximum(acc[0][:, 2], counts[:, 2])
    acc[1] += sums
    return acc


def bench_shape(name, shape, rounds, dev):
    import torch
    from qconvnet import ops
    gen = torch.Generator(device=dev).manual_seed(sum(shape))
    c = shape[1]
    x = torch.randn(shape, generator=gen, device=dev).relu_()          # a post-ReLU activation
    yn = x + 0.05 * torch.randn(shape, generator=gen, device=dev)
    yn = torch.where(x == 0, x, yn).contiguous()                       # NCHW
    y = yn.permute(0, 2, 3, 1).contiguous() if len(shape) == 4 else yn  # NHWC
    counts, sums = ops.qerror_f32_buffers(c, dev)
    ws = torch.empty(ops.qerror_f32_workspace_size(*(shape if len(shape) == 4 else shape + (1, 1))),
                     dtype=torch.uint8, device=dev)
    paths = {"torch_ops": lambda: torch_score_f32(x, y),
             "kernel_nhwc": lambda: ops.qerror_f32(x, y, counts, sums, nhwc=True, workspace=ws),
             "kernel_nchw": lambda: ops.qerror_f32(x, yn, counts, sums, nhwc=False, workspace=ws)}
    for _ in range(3):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in paths}
    for _ in range(rounds):
        for k, fn in paths.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                fn()
            b.record()
            b.synchronize()
            us[k].append(a.elapsed_time(b) * 1e3 / REPS)
    # the paths must agree: counts exactly (torch's e is the same fp32
    # subtraction), sums to fp32-product accuracy; NHWC and NCHW bit for bit
    tc, ts = torch_score_f32(x, y)
    got = {}
    for k, nhwc, yy in (("nhwc", True, y), ("nchw", False, yn)):
        counts.zero_()
        sums.zero_()
        ops.qerror_f32(x, yy, counts, sums, nhwc=nhwc, workspace=ws)
        got[k] = (counts.clone(), sums.clone())
        if not torch.equal(tc, counts):
            raise SystemExit(f"bench_resnet_report: counts differ from the torch composition's at {name}")
    if not torch.equal(got["nhwc"][1].view(torch.int64), got["nchw"][1].view(torch.int64)):
        raise SystemExit(f"bench_resnet_report: NHWC and NCHW sums differ at {name}")
    sums = got["nhwc"][1]
    rel = ((ts[:, :3] - sums[:, :3]).abs() / ts[:, :3].abs().clamp_min(1e-300)).max().item()
    sgn = ((ts[:, 3] - sums[:, 3]).abs() / ts[:, 2].clamp_min(1e-300)).max().item()
    if rel > 1e-5 or sgn > 1e-5:
        raise SystemExit(f"bench_resnet_report: sums differ from the torch composition's at {name} ({rel}, {sgn})")
    elems = x.numel()
    k = statistics.median(us["kernel_nhwc"])
    kn = statistics.median(us["kernel_nchw"])
    return {"layer": name, "shape": list(shape), "elements": elems, "bytes_read_once": 8 * elems,
            "workspace_bytes": ws.numel(), "calls_per_sample": REPS, "calls": rounds * REPS,
            "torch_ops": _stats(us["torch_ops"], "us"), "kernel_nhwc": _stats(us["kernel_nhwc"], "us"),
            "kernel_nchw": _stats(us["kernel_nchw"], "us"),
            "kernel_nhwc_gbytes_per_s": 8 * elems / k / 1e3, "kernel_nchw_gbytes_per_s": 8 * elems / kn / 1e3,
            "kernel_nhwc_share_of_hbm_copy_rate": 8 * elems / k / 1e3 / (HBM_COPY_TBS * 1e3),
            "torch_over_kernel_nhwc": statistics.median(us["torch_ops"]) / k,
            "max_rel_diff_of_sums_vs_torch_fp32": rel, "max_diff_of_sum_e_over_sum_abs_e": sgn}


def torch_report(mod, qmodel, weights, images, batch):
    """layer_report's walk scored by the torch compositions; one sync at the end."""
    import torch
    from bench_qerror import torch_score
    from qconvnet.qerror import summarize, summarize_f32
    acc = {}
    for name, x, y, scale, zp, _ in mod.layer_pairs(qmodel, weights, images, batch):
        u8 = y.dtype == torch.uint8
        if name not in acc:
            c = x.shape[1]
            acc[name] = [torch.zeros((c, 5 if u8 else 3), dtype=torch.int64, device=x.device),
                         torch.zeros((c, 3 if u8 else 4), dtype=torch.float64, device=x.device)]
        if u8:
            torch_score(x, y, float(scale), int(zp), acc[name])
        else:
            torch_score_f32(x, y, acc[name])
    return {k: (summarize if c.shape[1] == 5 else summarize_f32)(c.cpu().numpy(), s.cpu().numpy())
            for k, (c, s) in acc.items()}


def bench_report(mode, rounds, dev):
    import torch
    from models.custom_quantization_model import CustomQuantizedResNet50
    from models.resnet import synthetic_images, synthetic_resnet
    from qconvnet import resnet, resnet_qdq
    fp = synthetic_resnet(0, device=dev)
    calib = [torch.from_numpy(synthetic_images(16, 1))]
    w = CustomQuantizedResNet50(fp, calibration_batches=calib, device=dev, mode=mode,
                                calibration_device=str(dev))
    qm = w.quantized_model
    if mode == "static":
        mod, weights = resnet, resnet.fold_state_dict(fp.state_dict())
    else:
        mod, weights = resnet_qdq, resnet_qdq.unfolded_state(fp.state_dict())
    x = torch.from_numpy(synthetic_images(N_IMAGES, 2)).to(dev)
    runs = {"layer_report": lambda: mod.layer_report(qm, weights, x, BATCH),
            "torch_report": lambda: torch_report(mod, qm, weights, x, BATCH)}
    ms = {k: [] for k in runs}
    for r in range(rounds + 1):          # one warm-up round
        for k, fn in runs.items():       # the paths alternate inside a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                         # each ends in its device-to-host copies
            dt = time.perf_counter() - t0
            if r >= 1:
                ms[k].append(dt * 1e3)
    a, b = runs["layer_report"](), runs["torch_report"]()
    differ = [f"{name}.{k}" for name in a for k in ("count", "differ")
              if a[name]["tensor"][k] != b[name]["tensor"][k]]
    res = {"images": N_IMAGES, "batch": BATCH, "mode": mode, "names": len(a),
           "fields_differing_from_torch_report": differ,
           "note": "both walks include the fp32 net and the kept int8 forward; only the scoring differs",
           "layer_report": _stats(ms["layer_report"], "ms"),
           "torch_report": _stats(ms["torch_report"], "ms"),
           "sqnr_db": {name: float(r["tensor"]["sqnr_db"]) for name, r in a.items()}}
    res["torch_over_layer_report"] = res["torch_report"]["median_ms"] / res["layer_report"]["median_ms"]
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=20, help="alternating rounds per shape (x 5 calls each)")
    ap.add_argument("--e2e-rounds", type=int, default=5)
    ap.add_argument("--shapes-only", action="store_true",
                    help="the kernel shapes alone (e.g. for a variant library loaded with QCN_LIB)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resnet_report: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "hbm_copy_tbytes_per_s": HBM_COPY_TBS, "shapes": [],
           "reports": []}
    for n, s in SHAPES:
        res["shapes"].append(bench_shape(n, s, args.rounds, dev))
        print("done:", n, file=sys.stderr, flush=True)
    for m in () if args.shapes_only else ("reference", "static"):
        res["reports"].append(bench_report(m, args.e2e_rounds, dev))
        print("done: report", m, file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    bad = [(r["mode"], r["fields_differing_from_torch_report"]) for r in res["reports"]
           if r["fields_differing_from_torch_report"]]
    if bad:
        raise SystemExit(f"bench_resnet_report: the two reports differ at {bad}")


if __name__ == "__main__":
    main()
