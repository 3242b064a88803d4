"""Time the device scorer (qcn_eval_topk_f32) against the host scoring it
replaces, in one process with the two paths alternating.

Per batch of logits ([1024,10], [8192,10], [512,1000] fp32 on the device):
  host    what ModelEvaluator does per batch with counts="host": out.cpu(),
          topk(5), torch.max and two bincounts on the host — host clock, the
          .cpu() is its sync;
  device  qcn_eval_topk_f32 into device counters (with and without the
          confusion matrix): kernel time from HIP events around REPS
          back-to-back launches of the C entry (at least 200 launches in all;
          a few microseconds each, so the figure still holds the launch
          cadence and is an upper bound), and the host clock over a queue of
          ops.eval_topk calls closed by one sync (what a caller pays per
          batch).
End to end, 10 240 random uint8 [32,32,3] images through a calibrated
StaticPTQModel at batch 1024, in images/s: ModelEvaluator(device="cuda")
(host counts: evaluate_accuracy, one pass; and evaluate_accuracy +
evaluate_class_accuracy, the two passes top-k plus per-class cost there)
against evaluate(streams=1) and evaluate(streams=2) (one pass: top-1, top-5,
per-class), with pinned host input and with device-resident input.
Medians over alternating rounds after warm-up; min and max are kept so the
spread can be judged.  Prints one JSON line and writes it to --out.

  python tools/bench_eval.py --out profiles/eval_bench.json
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

REPS = 20            # launches per event pair, back to back
SHAPES = ((1024, 10), (8192, 10), (512, 1000))
N_IMAGES, BATCH = 10240, 1024


def _stats(xs, unit):
    return {f"median_{unit}": statistics.median(xs), f"min_{unit}": min(xs), f"max_{unit}": max(xs),
            "samples": len(xs)}


def _host_score(out, labels, n):
    """The per-batch host scoring of ModelEvaluator(counts="host"):
    evaluate_accuracy's and _class_counts' bodies on one batch."""
    import torch
    out = out.cpu()
    _, pred = out.topk(5, 1, True, True)
    pred = pred.t()
    correct = pred.eq(labels.view(1, -1).expand_as(pred))
    c1, c5 = correct[0].sum().item(), correct.sum().item()
    _, predicted = torch.max(out, 1)
    total = torch.bincount(labels, minlength=n)[:n].double()
    hit = torch.bincount(labels[predicted == labels], minlength=n)[:n].double()
    return c1, c5, total, hit


def bench_shape(rows, cols, rounds, dev):
    import torch
    from qconvnet import ops
    gen = torch.Generator().manual_seed(rows + cols)
    # quantised-looking logits, as the static int8 head produces them
    logits = (0.25 * (torch.randint(0, 64, (rows, cols), generator=gen) - 32)).float().to(dev)
    labels = torch.randint(0, cols, (rows,), generator=gen)
    labels_d = labels.to(dev)
    counters = torch.zeros(ops.eval_counters_len(cols), dtype=torch.int64, device=dev)
    confusion = torch.zeros((cols, cols), dtype=torch.int64, device=dev)

    def device(conf):
        ops.eval_topk(logits, labels_d, 5, counters, confusion if conf else None)

    # the kernel legs call the C ABI with prebuilt arguments: the tensor
    # checks of ops.eval_topk cost more host time than these kernels run, and
    # events around such a queue would time the enqueue
    entry = ops.lib().qcn_eval_topk_f32
    ptr = ops._ptr
    direct = {conf: (ptr(logits), rows, cols, ptr(labels_d), 5, ptr(counters),
                     ptr(confusion) if conf else None, None, ops._stream())
              for conf in (False, True)}

    for _ in range(5):
        _host_score(logits, labels, cols)
        device(False)
        device(True)
    torch.cuda.synchronize()
    host_us, kern_us, kern_conf_us, queue_us = [], [], [], []
    for _ in range(rounds):
        t0 = time.perf_counter()
        _host_score(logits, labels, cols)
        host_us.append((time.perf_counter() - t0) * 1e6)
        for conf, sink in ((False, kern_us), (True, kern_conf_us)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(REPS):
                entry(*direct[conf])
            b.record()
            b.synchronize()
            sink.append(a.elapsed_time(b) * 1e3 / REPS)
        t0 = time.perf_counter()
        for _ in range(REPS):
            device(False)
        torch.cuda.synchronize()
        queue_us.append((time.perf_counter() - t0) * 1e6 / REPS)
    # the timed launches all added into `counters`: a check that they counted
    counters.zero_()
    device(False)
    got = counters.cpu()
    c1, c5, total, hit = _host_score(logits, labels, cols)
    # (top-1 against the torch.max hits: topk's order among tied values is unspecified)
    if (int(got[0]) != rows or int(got[1]) != int(hit.sum())
            or not torch.equal(got[4:4 + cols].double(), total)):
        raise SystemExit(f"bench_eval: device counts differ from the host's at {rows}x{cols}")
    return {"rows": rows, "cols": cols, "logits_bytes": rows * cols * 4,
            "launches_per_sample": REPS, "launches": rounds * REPS,
            "host_per_batch": _stats(host_us, "us"),
            "device_kernel": _stats(kern_us, "us"),
            "device_kernel_with_confusion": _stats(kern_conf_us, "us"),
            "device_per_batch_queued_host_clock": _stats(queue_us, "us"),
            "host_over_device_kernel": statistics.median(host_us) / statistics.median(kern_us),
            "host_over_device_queued": statistics.median(host_us) / statistics.median(queue_us),
            "top5_host": c5, "top5_device": int(got[2])}


def bench_end_to_end(rounds, dev):
    import torch
    from models.baseline_model import SimpleConvNet
    from models.static_ptq_model import StaticPTQModel
    from qconvnet.evaluate import evaluate
    from utils.model_evaluator import ModelEvaluator
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(1)
    img = torch.randint(0, 256, (N_IMAGES, 32, 32, 3), generator=gen, dtype=torch.uint8)
    lab = torch.randint(0, 10, (N_IMAGES,), generator=gen)
    ptq = StaticPTQModel(device=dev)
    ptq.load_state_dict(SimpleConvNet().state_dict())
    model = ptq.quantize(img[:256])
    classes = [str(i) for i in range(10)]
    inputs = {"host_input": img.pin_memory(), "device_input": img.to(dev)}
    res = {"images": N_IMAGES, "batch": BATCH}
    for name, x in inputs.items():
        loader = [(x[a:a + BATCH], lab[a:a + BATCH]) for a in range(0, N_IMAGES, BATCH)]
        ev = ModelEvaluator(loader, device=str(dev))

        def one_pass():
            return ev.evaluate_accuracy(model, verbose=False)

        def two_passes():
            ev.evaluate_accuracy(model, verbose=False)
            return ev.evaluate_class_accuracy(model, classes, verbose=False)

        runs = {"model_evaluator_host_counts_top1_top5": one_pass,
                "model_evaluator_host_counts_top5_and_per_class": two_passes,
                "evaluate_streams1": lambda: evaluate(model, x, lab, BATCH, 5, 1),
                "evaluate_streams2": lambda: evaluate(model, x, lab, BATCH, 5, 2)}
        rate = {k: [] for k in runs}
        for r in range(rounds + 2):          # two warm-up rounds
            for k, fn in runs.items():       # the paths alternate inside a round
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                         # each ends in its own sync (.cpu() / result())
                dt = time.perf_counter() - t0
                if r >= 2:
                    rate[k].append(N_IMAGES / dt)
        got = evaluate(model, x, lab, BATCH, 5, 2)
        per_class = two_passes()
        mine = {classes[c]: 100.0 * int(got["class_correct"][c]) / int(got["class_total"][c])
                for c in range(10) if got["class_total"][c] > 0}
        if got["rows"] != N_IMAGES or mine != per_class:
            raise SystemExit("bench_eval: evaluate() and ModelEvaluator disagree per class")
        res[name] = {k: _stats(v, "images_per_s") for k, v in rate.items()}
        base = res[name]["model_evaluator_host_counts_top1_top5"]["median_images_per_s"]
        for k in ("evaluate_streams1", "evaluate_streams2"):
            res[name][k + "_over_host_counts"] = res[name][k]["median_images_per_s"] / base
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=40,
                    help="alternating rounds per shape (x 20 launches each)")
    ap.add_argument("--e2e-rounds", type=int, default=15)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.rounds * REPS < 200:
        ap.error("--rounds: at least 200 timed launches (10 rounds)")

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval: no GPU (there is no CPU fallback to time)")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0),
           "shapes": [bench_shape(r, c, args.rounds, dev) for r, c in SHAPES],
           "end_to_end": bench_end_to_end(args.e2e_rounds, dev)}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
