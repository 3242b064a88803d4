"""Benchmark: images/sec of the full static-PTQ int8 SimpleConvNet at batch 1024
(3x32x32) per MI355X — BASELINE.json's metric on configs[2] (N=1) and
configs[3] (batch 8192 = 8 x 1024 sharded, RCCL all-gather of logits, N=8).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    torchrun --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N ...

A step = one forward of the whole int8 net over this rank's 1024 resident
images (fp32 NCHW in HBM -> quantize+conv1 ... fc2 -> fp32 logits) plus, for
N > 1, the all-gather of every rank's logits.  Weak scaling: 1024 images per
GPU.  Weights: random-init SimpleConvNet with BN statistics recalibrated on
synthetic CIFAR-normalised images (no trained checkpoint or dataset offline),
calibrated once on rank 0 and broadcast.

Prints ONE JSON line on rank 0 with value (whole-job images/sec) and
ms_per_step over the K timed steps.  A plain run does only that: set up, warm
up, time the K steps, print.  ``--dump-outputs DIR`` also writes the logits of
the last timed step to DIR/logits.npy (fp32; the inputs and the model are the
same from run to run, so two builds compare output for output).  ``--full``
adds everything else the line can carry: ``sustained``, a ``roofline`` object
for the dominant kernel (HIP-event per-kernel timing over a second timed pass,
rocprofv3 counter passes, the in-kernel clock), at N > 1 the all-gather's own
time, at N = 1 ``cpu_baseline`` (the reference's StaticPTQModel path — torch.ao
quantize_dynamic — timed on the host cores), ``top1`` and ``configs_extra``.
"""
from __future__ import annotations

import argparse
import contextlib
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.join(ROOT, "convnet-quantization_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "images/sec at batch 1024 (3×32×32) int8 static-PTQ, 1/2/4/8 MI355X; top-1 delta"
METRIC_QDQ = "images/sec at batch 256 (3×32×32) per-layer QDQ int8 conv (CustomQuantizationModel), 1 MI355X"
PEAK_INT8_TOPS = 5033.0   # 256 CU x 4 SIMD x 2048 int8 op/clk x 2.4 GHz (dense)
PEAK_HBM_GBS = 8000.0
# MAC per image per kernel
MAC_PER_IMAGE = {"conv1": 1_769_472, "conv2": 37_748_736, "conv3": 18_874_368,
                 "conv4": 37_748_736, "conv5": 18_874_368, "conv6": 37_748_736,
                 "fc1": 2_097_152, "fc2": 5_120}
MAC_PER_IMAGE["conv12"] = MAC_PER_IMAGE["conv1"] + MAC_PER_IMAGE["conv2"]
MAC_PER_IMAGE["fc12"] = MAC_PER_IMAGE["fc1"] + MAC_PER_IMAGE["fc2"]
MAC_PER_IMAGE["conv34"] = MAC_PER_IMAGE["conv3"] + MAC_PER_IMAGE["conv4"]
MAC_PER_IMAGE["conv56"] = MAC_PER_IMAGE["conv5"] + MAC_PER_IMAGE["conv6"]
MAC_PER_IMAGE["net"] = sum(MAC_PER_IMAGE[f"conv{i}"] for i in range(1, 7))
MAC_PER_IMAGE["conv1_6"] = MAC_PER_IMAGE["net"]   # the one-launch conv1 .. conv6
MAC_PER_IMAGE["conv3_6"] = MAC_PER_IMAGE["conv34"] + MAC_PER_IMAGE["conv56"]   # conv3 .. conv6, one launch
# algorithmic HBM bytes per image (u8 activations, fp32 input/logits)
BYTES_PER_IMAGE = {"conv1": 3 * 32 * 32 * 4 + 32 * 32 * 64,
                   "conv2": 32 * 32 * 64 + 16 * 16 * 64,
                   "conv3": 16 * 16 * 64 + 16 * 16 * 128,
                   "conv4": 16 * 16 * 128 + 8 * 8 * 128,
                   "conv5": 8 * 8 * 128 + 8 * 8 * 256,
                   "conv6": 8 * 8 * 256 + 4 * 4 * 256,
                   "fc1": 4096 + 512, "fc2": 512 + 10 + 40,
                 "conv12": 3 * 32 * 32 * 4 + 16 * 16 * 64,
                 "fc12": 4096 + 512 + 10 + 40,
                 "conv34": 16 * 16 * 64 + 8 * 8 * 128,
                 "conv56": 8 * 8 * 128 + 4 * 4 * 256,
                 "net": 3 * 32 * 32 * 4 + 4 * 4 * 256,
                 # one launch: fp32 input, a6 out, and the a2 / a4 hand-offs it
                 # writes and reads back through memory
                 "conv1_6": 3 * 32 * 32 * 4 + 4 * 4 * 256 + 2 * (16 * 16 * 64 + 8 * 8 * 128),
                 # conv3 .. conv6 in one launch: a2 in, a6 out, a4 written and read back
                 "conv3_6": 16 * 16 * 64 + 4 * 4 * 256 + 2 * 8 * 8 * 128}
HBM_BOUND = {"conv1"}
# launch name -> the kernel symbols it runs (rocprofv3 Kernel_Name substrings)
KERNEL_SYMBOLS = {"conv1_6": ("convnet_convs16_kernel", "convnet_convs_kernel", "convnet_convs_sm_kernel"),
                  "conv12": ("conv12p_kernel",),
                  "conv3_6": ("convs36_w4_kernel",),
                  # (the persistent wave-specialised kernel from two images per CU
                  # (four for conv5+6), the per-tile pair kernels below)
                  "conv34": ("convpair_ws_kernel<qcn::ConvCfg<64, 128", "convpair_kernel<qcn::ConvCfg<64, 128"),
                  # (one form runs per batch size: the split form at <= 1 image per CU)
                  "conv56": ("convpair_ws_kernel<qcn::ConvCfg<128, 256", "convpair_ga_kernel",
                             "convpair_ga_split_kernel"),
                  # the two-launch head: "fc_finish" matches fc_finish_kernel (static)
                  # and fc_finish_qdq_kernel (QDQ)
                  "fc12": ("fc_splitk_kernel", "fc_finish"),
                  "fc1": ("linear_u8s8_kernel",), "fc2": ("linear_f32_kernel",)}


# The parent hands its model to the counter-pass children through a file in a
# no-code format: torch.save of tensors / dicts / lists / primitives only, read
# back with torch.load(weights_only=True).  numpy arrays and scalars are tagged
# so they come back with their exact dtype.
def _enc(o):
    if isinstance(o, np.ndarray):
        return {"__nd__": torch.from_numpy(np.ascontiguousarray(o))}
    if isinstance(o, np.generic):
        return {"__np__": str(o.dtype), "v": o.item()}
    if isinstance(o, dict):
        return {"__dict__": [[_enc(k), _enc(v)] for k, v in o.items()]}
    if isinstance(o, (list, tuple)):
        return {"__seq__": type(o).__name__, "v": [_enc(x) for x in o]}
    if isinstance(o, torch.Tensor):
        return {"__t__": o.detach().cpu()}
    if o is None or isinstance(o, (bool, int, float, str)):
        return o
    raise TypeError(f"payload: cannot encode {type(o).__name__}")


def _dec(o):
    if isinstance(o, dict):
        if "__nd__" in o:
            return o["__nd__"].numpy()
        if "__np__" in o:
            return np.dtype(o["__np__"]).type(o["v"])
        if "__dict__" in o:
            return {_dec(k): _dec(v) for k, v in o["__dict__"]}
        if "__seq__" in o:
            v = [_dec(x) for x in o["v"]]
            return tuple(v) if o["__seq__"] == "tuple" else v
        if "__t__" in o:
            return o["__t__"]
    return o


def save_payload(path, payload):
    torch.save(_enc(payload), path)


def load_payload(path):
    return _dec(torch.load(path, weights_only=True))


DUMP_MAX_BYTES = 64 << 20   # --dump-outputs writes at most this much in all


def dump_outputs(directory, arrays, max_bytes=DUMP_MAX_BYTES):
    """--dump-outputs: write what the timed step returned, {name: tensor}, as
    DIR/<name>.npy in fp32.  An output over its share of ``max_bytes`` is cut to
    a fixed, seeded sample of its rows (the same rows in every run)."""
    os.makedirs(directory, exist_ok=True)
    share = max_bytes // max(1, len(arrays))
    for name, t in arrays.items():
        a = np.ascontiguousarray(t.detach().cpu().numpy(), dtype=np.float32)
        if a.nbytes > share:
            a = a.reshape(a.shape[0], -1) if a.ndim > 1 else a.reshape(-1, 1)
            rows = max(1, share // (a.shape[1] * 4))
            keep = np.sort(np.random.default_rng(0).choice(a.shape[0], size=min(rows, a.shape[0]),
                                                           replace=False))
            a = np.ascontiguousarray(a[keep])
        np.save(os.path.join(directory, name + ".npy"), a)


WARMUP_MIN_S = 0.1   # untimed forwards after the W warmup steps, at least this long


def ramp_warmup(step, drain, warmup, world, dev, min_s=WARMUP_MIN_S, sync=None):
    """The W warmup steps, then more untimed steps until at least min_s of
    back-to-back forwards have run.  After an idle spell the chip needs a few
    ms of load to reach the throughput it then holds: on one box the headline
    read 6.2-6.5 M img/s after 10 warmup steps and 7.1-7.2 M after 200 (or
    over 300-1000 timed steps), profiles/r03_diag_warmup.txt.  The extra step
    count comes from a 5-step probe and is the max over ranks, so every rank
    runs the same number of steps (their logits all-gathers pair up).
    Returns the number of warmup steps run.  ``sync`` waits for the device
    (default torch.cuda.synchronize)."""
    sync = sync or torch.cuda.synchronize
    for _ in range(warmup):
        step()
    drain()
    sync()
    t0 = time.perf_counter()
    for _ in range(5):
        step()
    drain()
    sync()
    per = (time.perf_counter() - t0) / 5
    extra = max(0, int(np.ceil(min_s / max(per, 1e-6))) - warmup - 5)
    if world > 1:
        tdev = dev if dist.get_backend() == "nccl" else "cpu"
        t = torch.tensor([extra], dtype=torch.int64, device=tdev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        extra = int(t.item())
    for _ in range(extra):
        step()
    drain()
    sync()
    return warmup + 5 + extra


def under_profiler():
    """True when this process already runs under rocprofv3 (its preloaded tool
    library initialised the GPU before main): a nested rocprofv3 child would then
    be an exec from a GPU-initialised process tree, which the box refuses."""
    pre = os.environ.get("LD_PRELOAD", "")
    return ("rocprof" in pre or any(k.startswith(("ROCPROF", "ROCP_")) for k in os.environ))


def build_model(rank, device, per_channel=False, spec_file=None, mode="static"):
    from models.baseline_model import trained_synthetic_model
    from qconvnet import data
    from qconvnet.dist import broadcast_object
    from qconvnet.qmodel import QuantizedConvNet, build_qspec, calibrate, fold_state_dict
    payload = None
    if spec_file:   # a counter pass: the parent's model, written by this script
        payload = load_payload(spec_file)
    elif rank == 0:
        # trained on the synthetic 10-class task (no CIFAR-10 / checkpoint offline)
        x_cal, _ = data.synthetic_task(512, 1)
        calib = torch.from_numpy(x_cal)
        fp = trained_synthetic_model(0, device=device)
        folded = fold_state_dict(fp.state_dict())
        ranges = calibrate(folded, [calib], "cpu")
        # host copies: the payload is pickled to every rank, and GPU tensors
        # would unpickle onto rank 0's device in every process
        payload = (build_qspec(folded, ranges, mode, per_channel),
                   {k: v.detach().cpu() for k, v in fp.state_dict().items()})
    spec, sd = broadcast_object(payload)
    return QuantizedConvNet(spec, device), sd


def cpu_baselines(state_dict, qmodel_gpu, seconds):
    """Reference CPU paths on the host cores (rank 0, N = 1 only)."""
    if qmodel_gpu.mode == "qdq":
        return cpu_baseline_qdq(state_dict, qmodel_gpu, seconds)
    from oracle import torch_ref
    from qconvnet import data
    fp = torch_ref.SimpleConvNetRef()
    fp.load_state_dict(state_dict)
    fp.eval()
    threads = torch.get_num_threads()
    out = {}
    # (1) BASELINE configs[0]: StaticPTQModel as the reference builds it
    #     (static_ptq_model.py:19-34: quantize_dynamic({Linear, Conv2d}, qint8) ->
    #     fp32 convs + dynamic int8 fc), timed on the CPU through the build's own
    #     harness, InferenceBenchmark.measure_throughput(batch_size=32)
    #     (utils/inference_benchmark.py:81-105), sized to ~`seconds` of CPU work
    from utils.inference_benchmark import InferenceBenchmark
    sp = torch_ref.build_static_ptq_cpu(fp)
    bs = 32
    x = torch.from_numpy(data.synthetic_images(bs, 11))
    harness = InferenceBenchmark([(x, torch.zeros(bs, dtype=torch.long))], device="cpu")
    with contextlib.redirect_stdout(sys.stderr):   # stdout carries only the JSON line
        harness.warm_up(sp, num_iterations=3)
        probe = harness.measure_throughput(sp, batch_size=bs, num_iterations=20, verbose=False)
        iters = max(20, int(seconds * probe / bs))
        thr = harness.measure_throughput(sp, batch_size=bs, num_iterations=iters, verbose=False)
    out["static_ptq"] = {"value": thr, "unit": "images/sec", "cores": threads,
                         "cpu_count": os.cpu_count(), "kind": "port",
                         "sample": f"BASELINE configs[0]: reference StaticPTQModel path (torch.ao "
                                   f"quantize_dynamic {{Linear,Conv2d}} qint8 on our SimpleConvNet "
                                   f"restatement), batch {bs} x {iters} iters through "
                                   f"utils.inference_benchmark.InferenceBenchmark.measure_throughput"}
    # (1b) the same harness at the GPU batch sizes BASELINE.md §4 names (256,
    #      1024), a third of the budget each
    out["static_ptq_batches"] = {}
    for bsb in (256, 1024):
        xb = torch.from_numpy(data.synthetic_images(bsb, 13))
        hb = InferenceBenchmark([(xb, torch.zeros(bsb, dtype=torch.long))], device="cpu")
        with contextlib.redirect_stdout(sys.stderr):
            hb.warm_up(sp, num_iterations=1)
            pr = hb.measure_throughput(sp, batch_size=bsb, num_iterations=2, verbose=False)
            it_b = max(2, int(seconds / 3 * pr / bsb))
            tb = hb.measure_throughput(sp, batch_size=bsb, num_iterations=it_b, verbose=False)
        out["static_ptq_batches"][str(bsb)] = {
            "value": tb, "unit": "images/sec", "cores": threads, "cpu_count": os.cpu_count(),
            "sample": f"reference StaticPTQModel path, batch {bsb} x {it_b} iters through "
                      f"InferenceBenchmark.measure_throughput"}
    # (2) full static int8 on the CPU (torch.ao eager, fbgemm) — apples to apples
    calib = torch.from_numpy(data.synthetic_task(512, 1)[0])   # the GPU model's calibration set
    q = torch_ref.build_static_int8_cpu(fp, [calib])
    bs2 = 256
    x2 = torch.from_numpy(data.synthetic_images(bs2, 12))
    with torch.no_grad():
        q(x2)
        total, iters = 0.0, 0
        while total < seconds / 2:
            t0 = time.time()
            q(x2)
            total += time.time() - t0
            iters += 1
    out["static_int8"] = {"value": bs2 * iters / total, "unit": "images/sec", "cores": threads,
                          "cpu_count": os.cpu_count(), "kind": "port",
                          "sample": f"torch.ao eager static int8 (fbgemm), batch {bs2} x {iters} iters"}
    # (3) top-1 on a held-out synthetic test set with true labels (the fp32
    #     model was trained on the same task; CIFAR-10 is not available offline)
    xe_np, ye_np = data.synthetic_task(4096, 77)
    xe, lab = torch.from_numpy(xe_np), torch.from_numpy(ye_np)
    with torch.no_grad():
        fp_pred = fp(xe).argmax(1)
        ref_pred = sp(xe).argmax(1)
        gpu_pred = qmodel_gpu(xe).argmax(1)
        cpu_int8_pred = q(xe).argmax(1)
    # the reference's own StaticPTQModel semantics on the GPU (fp32 convs +
    # HIP dynamic int8 Linear, models/static_ptq_model.py mode="reference")
    from models.static_ptq_model import StaticPTQModel
    rm = StaticPTQModel(device=qmodel_gpu.device, mode="reference")
    rm.load_state_dict(state_dict)
    rq = rm.quantize()
    with torch.no_grad():
        gpu_ref_pred = rq(xe.to(qmodel_gpu.device)).argmax(1).cpu()

    def acc(p):
        return (p == lab).float().mean().item() * 100

    out["top1"] = {"labels": "true labels of 4096 held-out images of the synthetic 10-class task "
                             "the fp32 SimpleConvNet was trained on (qconvnet.data.synthetic_task)",
                   "fp32": acc(fp_pred), "gpu_int8_static": acc(gpu_pred),
                   "cpu_reference_static_ptq": acc(ref_pred),
                   "cpu_torchao_static_int8": acc(cpu_int8_pred),
                   "gpu_reference_mode_static_ptq": acc(gpu_ref_pred),
                   "delta_vs_reference_pct": acc(gpu_pred) - acc(ref_pred),
                   "delta_reference_mode_pct": acc(gpu_ref_pred) - acc(ref_pred),
                   "gpu_int8_equals_torchao_static_int8": bool(torch.equal(gpu_pred, cpu_int8_pred)),
                   "agreement_gpu_int8_vs_fp32_pct": (gpu_pred == fp_pred).float().mean().item() * 100}
    return out


def cpu_baseline_qdq(state_dict, qmodel_gpu, seconds):
    """configs[1]'s CPU counterpart: the per-layer QDQ net (every conv and fc1
    QuantStub -> int8 op -> DeQuantStub, fp32 ReLU / pool / fc2,
    custom_quantization_model.py:202-261) with its stubs converted by torch.ao
    (fbgemm), batch 256, on the host cores; and the top-1 of both on the
    held-out synthetic set."""
    from oracle import torch_ref
    from qconvnet import data
    fp = torch_ref.SimpleConvNetRef()
    fp.load_state_dict(state_dict)
    fp.eval()
    threads = torch.get_num_threads()
    calib = torch.from_numpy(data.synthetic_task(512, 1)[0])
    q = torch_ref.build_qdq_cpu(fp, [calib])
    bs = 256
    x = torch.from_numpy(data.synthetic_images(bs, 12))
    with torch.no_grad():
        q(x)
        total, iters = 0.0, 0
        while total < seconds:
            t0 = time.time()
            q(x)
            total += time.time() - t0
            iters += 1
    out = {"static_ptq": {"value": bs * iters / total, "unit": "images/sec", "cores": threads,
                          "cpu_count": os.cpu_count(), "kind": "port",
                          "sample": f"BASELINE configs[1] on the CPU: per-layer QDQ SimpleConvNet "
                                    f"(torch.ao fbgemm, stubs converted), batch {bs} x {iters} iters"}}
    xe_np, ye_np = data.synthetic_task(4096, 77)
    xe, lab = torch.from_numpy(xe_np), torch.from_numpy(ye_np)
    with torch.no_grad():
        fp_pred = fp(xe).argmax(1)
        gpu_pred = qmodel_gpu(xe).argmax(1)
        cpu_pred = q(xe).argmax(1)

    def acc(p):
        return (p == lab).float().mean().item() * 100

    out["top1"] = {"labels": "true labels of 4096 held-out images of the synthetic 10-class task",
                   "fp32": acc(fp_pred), "gpu_int8_qdq": acc(gpu_pred),
                   "cpu_torchao_qdq": acc(cpu_pred),
                   "delta_vs_cpu_qdq_pct": acc(gpu_pred) - acc(cpu_pred),
                   "argmax_agreement_gpu_vs_cpu_qdq_pct": (gpu_pred == cpu_pred).float().mean().item() * 100}
    return out


# ------------------------------------------------------------ PMC passes
# HBM traffic, MFMA busy and the clock the chip holds come from rocprofv3
# counter passes over a child run of this script (same model, same batch),
# collected the way MI355X_MICROARCH.md's HBM/rocprofv3 section prescribes:
# one pass per counter group, FETCH_SIZE doubled on gfx950 (it tallies 128-B
# requests at 64 B), WRITE_SIZE as is, both in KiB per dispatch; the clock as
# mfma_busy as SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x GRBM_GUI_ACTIVE / 8) of
# the same batch-B dispatch.  GRBM_GUI_ACTIVE / 8 / wall time reads high on
# dispatches shorter than ~0.3 ms (MI355X_MICROARCH.md 'DVFS give-back'), so the
# clock the chip holds is measured in-kernel instead (tools/clock: s_memtime /
# s_memrealtime around each workgroup of a diagnostic build, see clock_pass()).
PMC_PASSES = (("fetch", ("FETCH_SIZE",), None),
              ("write", ("WRITE_SIZE", "SQ_VALU_MFMA_BUSY_CYCLES", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE"), None))


def _pmc_child(counters, batch, spec_file, per_channel, timeout, mode="static", extra=(), totals=False):
    """One rocprofv3 --pmc pass over `bench.py --no-cpu --no-pmc` as a child
    process (never an exec).  Returns ({kernel: {counter: mean per dispatch}},
    the child's JSON line) or raises; with totals, {kernel: {counter: [sum
    over dispatches, dispatches]}} instead of the means."""
    exe = shutil.which("rocprofv3")
    if exe is None:
        raise RuntimeError("rocprofv3 not on PATH")
    out = tempfile.mkdtemp(prefix="qcn_pmc_", dir="/tmp")
    cmd = [exe, "--pmc", *counters, "--kernel-include-regex", "qcn::", "-f", "csv", "-d", out,
           "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--steps", "3", "--warmup",
           "1", "--warmup-min-ms", "0", "--no-cpu", "--no-pmc", "--no-extra", "--batch", str(batch)]
    if spec_file:
        cmd += ["--spec-file", spec_file]
    if per_channel:
        cmd.append("--per-channel")
    if mode == "qdq":
        cmd += ["--workload", "qdq"]
    cmd += list(extra)
    env = dict(os.environ, TMPDIR="/tmp")
    p = subprocess.Popen(cmd, cwd="/tmp", env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, start_new_session=True)
    try:
        so, se = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        shutil.rmtree(out, ignore_errors=True)
        raise RuntimeError(f"rocprofv3 pass {counters} timed out")
    try:
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 pass {counters} exit {p.returncode}: {se[-400:]}")
        files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            raise RuntimeError(f"rocprofv3 pass {counters}: no counter csv")
        agg = {}
        for f in files:
            for r in csv.DictReader(open(f)):
                d = agg.setdefault(r["Kernel_Name"], {}).setdefault(r["Counter_Name"], [])
                d.append(float(r["Counter_Value"]))
        child = next((json.loads(ln) for ln in so.splitlines() if ln.startswith("{")), None)
        if totals:
            return {k: {c: [float(np.sum(v)), len(v)] for c, v in dd.items()} for k, dd in agg.items()}, child
        return {k: {c: float(np.mean(v)) for c, v in dd.items()} for k, dd in agg.items()}, child
    finally:
        shutil.rmtree(out, ignore_errors=True)


def _per_launch(agg, launch, counter):
    """Sum over the launch's kernels of the mean per-dispatch counter value."""
    tot, seen = 0.0, False
    for sym in KERNEL_SYMBOLS[launch]:
        for k, dd in agg.items():
            if sym in k and counter in dd:
                tot += dd[counter]
                seen = True
                break
    return tot if seen else None


def clock_pass(spec_file, args, mode, timeout=240):
    """The in-kernel clock of the conv launches: tools/clock_probe.py as a plain
    child process (no profiler) on the diagnostic library with stamped copies
    of the conv kernels, same model and batch.  Returns {launch: {...}}."""
    probe = os.path.join(ROOT, "tools", "clock_probe.py")
    lib = os.path.join(ROOT, "tools", "clock", "libqconvnet_clock.so")
    if not os.path.exists(lib):
        raise RuntimeError("tools/clock/libqconvnet_clock.so not built (__graft_entry__.build())")
    cmd = [sys.executable, probe, "--batch", str(args.batch), "--spec-file", spec_file,
           "--workload", "qdq" if mode != "static" else "convnet"]
    p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"clock probe exit {p.returncode}: {p.stderr[-400:]}")
    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
    if line is None:
        raise RuntimeError("clock probe printed no JSON line")
    return json.loads(line)["kernels"]


def pmc_counters(model, sd, args, names, timeout=150):
    """Counter passes for every launch; returns ({launch: {...}}, error text)."""
    fd, spec_file = tempfile.mkstemp(prefix="qcn_spec_", suffix=".pt", dir="/tmp")
    os.close(fd)
    save_payload(spec_file, (model.spec, sd))
    res = {n: {} for n in names}
    errors = []
    try:
        for tag, counters, batch in PMC_PASSES:
            try:
                agg, child = _pmc_child(counters, batch or args.batch, spec_file, args.per_channel,
                                        timeout, model.mode)
            except Exception as e:   # a failed pass leaves its fields null
                errors.append(f"{tag}: {e}")
                continue
            for n in names:
                if tag == "fetch":
                    v = _per_launch(agg, n, "FETCH_SIZE")
                    res[n]["fetch_bytes"] = None if v is None else 2.0 * v * 1024
                    if v is None:
                        errors.append(f"{tag}: no counter row matched launch {n}")
                elif tag == "write":
                    v = _per_launch(agg, n, "WRITE_SIZE")
                    res[n]["write_bytes"] = None if v is None else v * 1024
                    busy = _per_launch(agg, n, "SQ_VALU_MFMA_BUSY_CYCLES")
                    gui = _per_launch(agg, n, "GRBM_GUI_ACTIVE")
                    res[n]["sq_valu_mfma_busy_cycles"] = busy
                    res[n]["sq_insts_valu"] = _per_launch(agg, n, "SQ_INSTS_VALU")
                    if busy is not None and gui:
                        # per SIMD: busy cycles / (1024 SIMDs x dispatch cycles per XCD)
                        res[n]["mfma_busy_gui"] = busy / (1024.0 * gui / 8.0)
                    if v is None:
                        errors.append(f"{tag}: no counter row matched launch {n}")
        try:
            clk = clock_pass(spec_file, args, model.mode)
            for n in names:
                c = clk.get(n, {})
                if "clock_ghz" in c:
                    res[n]["clock_ghz"] = c["clock_ghz"]
                    res[n]["mfma_issue_at_clock"] = c["mfma_issue_at_clock"]
                    res[n]["clock_probe_ms"] = c["ms"]
                if "phase_table" in c:
                    res[n]["phase_table"] = c["phase_table"]
                if "layer_table" in c:
                    res[n]["layer_table"] = c["layer_table"]
        except Exception as e:
            errors.append(f"clock: {e}")
    finally:
        os.unlink(spec_file)
    for n in names:
        r = res[n]
        if r.get("fetch_bytes") is not None and r.get("write_bytes") is not None:
            r["traffic_bytes"] = r["fetch_bytes"] + r["write_bytes"]
    return res, "; ".join(errors) or None


class StepLoop:
    """The timed step of the metric: one forward over this rank's resident
    batch, plus at N > 1 the all-gather of its logits, issued asynchronously
    (qconvnet.dist.gather_logits_async: RCCL runs it on its own stream behind
    the batch's forward while the next batch computes into the model's other
    buffer slot; a slot's gather is waited for before the slot is reused, and
    every gather before the clock stops).  ``forward(marks=None, slot=0)``
    launches one forward and returns its logits; ``sync`` waits for the device
    (torch.cuda.synchronize; a no-op on CPU, where tests drive this loop over
    gloo).  The timed regions are bracketed by a barrier and sync on both
    sides and report the max over ranks."""

    def __init__(self, forward, world, dev, sync=lambda: None, graph=False):
        from qconvnet import dist as qd
        self.qd, self.forward, self.world, self.dev = qd, forward, world, dev
        self.sync, self.graph = sync, graph
        self.gathered = None     # two [world * B, classes] buffers, allocated at the first step
        self.pending = [None, None]
        self.nstep = 0
        self.last_slot = 0
        self.last_logits = None   # what the latest step's forward returned

    def _tdev(self):
        return self.dev if dist.get_backend() == "nccl" else "cpu"

    def step(self, marks=None):
        world = self.world
        slot = self.nstep % 2 if world > 1 else 0
        if self.pending[slot] is not None:
            self.pending[slot].wait()
            self.pending[slot] = None
        logits = self.forward(marks=marks, slot=slot)
        if world > 1:
            if self.gathered is None:
                self.gathered = [torch.empty((world * logits.shape[0],) + tuple(logits.shape[1:]),
                                             dtype=logits.dtype, device=logits.device) for _ in range(2)]
            self.pending[slot] = self.qd.gather_logits_async(logits, self.gathered[slot])
            if self.graph:   # the graph has one logits buffer: done before the next replay
                self.pending[slot].wait()
                self.pending[slot] = None
        self.last_slot = slot
        self.last_logits = logits
        self.nstep += 1
        return logits

    def outputs(self):
        """What a caller of the latest step receives, after drain() and sync():
        the whole job's logits (at N > 1 every rank's, gathered in rank order)."""
        return {"logits": self.gathered[self.last_slot] if self.world > 1 else self.last_logits}

    def drain(self):   # every outstanding all-gather has completed on the current stream
        for i in range(2):
            if self.pending[i] is not None:
                self.pending[i].wait()
                self.pending[i] = None

    def barrier(self):
        if self.world > 1:
            dist.barrier()

    def _max_over_ranks(self, v, dtype=torch.float64, op=None):
        t = torch.tensor([v], dtype=dtype, device=self._tdev())
        dist.all_reduce(t, op=op or dist.ReduceOp.MAX)
        return t.item()

    def timed(self, steps):
        """Region A: ``steps`` back-to-back steps; returns (seconds = max over
        ranks, every rank's ms per step or None at N = 1)."""
        self.barrier()
        self.sync()
        t0 = time.perf_counter()
        for _ in range(steps):
            self.step()
        self.drain()
        self.sync()
        self.barrier()
        elapsed = time.perf_counter() - t0
        rank_ms = None
        if self.world > 1:
            # every rank's own step time (the spread separates slow ranks from the
            # collective), then the max over ranks for the metric
            t = torch.tensor([elapsed], dtype=torch.float64, device=self._tdev())
            allt = [torch.zeros_like(t) for _ in range(self.world)]
            dist.all_gather(allt, t)
            rank_ms = [a.item() / steps * 1e3 for a in allt]
            elapsed = max(a.item() for a in allt)
        return elapsed, rank_ms

    def sustained(self, per_step, steps, batch, seconds=1.0):
        """Region S: the same step back to back for >= ``seconds`` right after
        region A (a field beside the metric, never the metric)."""
        n_sus = max(steps, int(np.ceil(seconds / max(per_step, 1e-6))))
        if self.world > 1:
            n_sus = int(self._max_over_ranks(n_sus, torch.int64))
        self.barrier()
        self.sync()
        t0s = time.perf_counter()
        for _ in range(n_sus):
            self.step()
        self.drain()
        self.sync()
        self.barrier()
        el_s = time.perf_counter() - t0s
        if self.world > 1:
            el_s = float(self._max_over_ranks(el_s))
        return {"value": self.world * batch * n_sus / el_s, "steps": n_sus, "seconds": el_s,
                "ms_per_step": el_s / n_sus * 1e3,
                "note": f"the same step back to back for >= {seconds:g} s right after the timed region; "
                        "reported beside the metric, not as it"}

    def allgather_timing(self, logits, reps):
        """The logits all-gather on its own: a blocking all_gather_into_tensor of
        one batch's logits, timed around device syncs (HIP events on the launch
        stream on the GPU): the collective's latency as the timed step would see
        it if nothing hid it."""
        out = torch.empty((self.world * logits.shape[0],) + tuple(logits.shape[1:]), dtype=logits.dtype,
                          device=logits.device)
        gms = []
        cuda = logits.is_cuda
        for _ in range(reps):
            self.barrier()
            if cuda:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.qd.gather_logits(logits, out)
                e1.record()
                self.sync()
                gms.append(e0.elapsed_time(e1))
            else:
                self.sync()
                t0 = time.perf_counter()
                self.qd.gather_logits(logits, out)
                self.sync()
                gms.append((time.perf_counter() - t0) * 1e3)
        return {"ms_mean": float(np.mean(gms)), "ms_min": float(np.min(gms)),
                "bytes_per_rank": int(logits.numel() * logits.element_size()),
                "note": "blocking all_gather_into_tensor of one batch's fp32 logits, HIP events "
                        "on the launch stream; in the timed step it runs asynchronously behind "
                        "the next batch's forward"}


def launch_ranks(argv, n):
    """``--gpus N`` (N > 1) without torchrun's env: start N ranks through
    torch.distributed.run as a CHILD process, from a parent that has not
    touched the GPU (no exec), and return its exit code.  Rank 0 of the child
    prints the one JSON line.  Never run one rank and label it N."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr=127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + list(argv)
    return subprocess.call(cmd)


def main_rehearse(args):
    """--rehearse: the multi-rank harness on CPU over gloo (launcher, barrier,
    StepLoop with the asynchronous logits all-gather, max-over-ranks timing,
    the N > 1 fields of the line).  Each rank's "forward" is a fixed fp32
    matmul of its shard standing in for the model: the line it prints is a
    rehearsal of the plumbing, not a measurement of the int8 path."""
    from qconvnet import dist as qd
    rank, world, _ = qd.init("gloo")
    B = args.batch
    g = torch.Generator().manual_seed(100 + rank)
    x = torch.rand((B, 3 * 32 * 32), generator=g)
    w = torch.rand((3 * 32 * 32, 10), generator=torch.Generator().manual_seed(0))

    def forward(marks=None, slot=0):
        return x @ w

    loop = StepLoop(forward, world, "cpu")
    warm_run = ramp_warmup(loop.step, loop.drain, args.warmup, world, "cpu", 0.0, sync=loop.sync)
    elapsed, rank_ms = loop.timed(args.steps)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, loop.outputs())
    result = {"metric": "harness rehearsal (CPU, gloo): not the int8 path", "value": world * B * args.steps / elapsed,
              "unit": "rows/sec", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
              "warmup_steps_run": warm_run, "ms_per_step": elapsed / args.steps * 1e3,
              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32",
              "data": "rehearsal", "config": {"workload": "rehearsal", "global_batch": world * B,
                                              "per_gpu_batch": B, "parallelism": f"dp{world}"}}
    if world > 1:
        result["rank_ms_per_step"] = rank_ms
        if args.full:
            result["allgather"] = loop.allgather_timing(forward(), 3)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1,
                    help="ranks, one per GPU; without torchrun's WORLD_SIZE, N > 1 starts "
                         "torch.distributed.run with N ranks as a child process")
    ap.add_argument("--rehearse", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps K (default 400 for the SimpleConvNet workloads, 50 for "
                         "ResNet-50: each timed region pays ~0.15-0.2 ms of start-up after its "
                         "synchronize, 2-4 %% of a 50-step region of 0.07-0.14 ms steps)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the logits the last of them returned (at "
                         "N > 1 the gathered logits of every rank) to DIR/logits.npy in fp32")
    ap.add_argument("--full", action="store_true",
                    help="beside the metric also measure and check everything else the line can "
                         "carry: sustained, per-kernel HIP events and the roofline, the rocprofv3 "
                         "counter and clock passes, the all-gather's own time, the CPU baselines "
                         "and top-1, configs_extra (--no-cpu / --no-pmc / --no-extra drop parts "
                         "of it).  A plain run times the K steps and prints the line")
    ap.add_argument("--warmup-min-ms", type=float, default=WARMUP_MIN_S * 1e3,
                    help="after the W warmup steps, keep running untimed forwards until this many ms "
                         "of them have run (0: exactly W); see ramp_warmup()")
    ap.add_argument("--batch", type=int, default=None,
                    help="images per GPU (default 1024; 256 for --workload qdq, 512 for resnet50)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-pmc", action="store_true",
                    help="skip the rocprofv3 counter passes (traffic, MFMA busy, held clock)")
    ap.add_argument("--spec-file", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--per-channel", action="store_true")
    ap.add_argument("--graph", action="store_true",
                    help="replay the forward as one HIP graph (measured slower: config 2 3.04 vs "
                         "3.11 M img/s, headline 5.9 vs 6.3 M img/s, profiles/r03_diag_graph_ab.txt)")
    ap.add_argument("--pipeline", type=int, default=0,
                    help="with --full: also time the forward with this many batches in flight on as many "
                         "HIP streams (QuantizedConvNet.run_pipelined, each batch its own buffers "
                         "and the full forward at its own batch size): a serving-throughput "
                         "field beside the metric, never the metric itself")
    ap.add_argument("--streams", type=int, default=2,
                    help="resnet50: split the batch over this many HIP streams, launches "
                         "interleaved layer by layer (QuantizedResNet.run_streams; measured "
                         "1/2/3/4: 81.7/86.7/86.3/72.1 K img/s at batch 512)")
    ap.add_argument("--separate-reduce", action="store_true",
                    help="resnet50: run layer 1's reduce convs as their own launches instead of "
                         "inside the expand + join launch (QuantizedResNet.fuse_reduce = False; A/B)")
    ap.add_argument("--no-extra", action="store_true",
                    help="convnet workload: skip the configs[1] / configs[4] child runs "
                         "(configs_extra on the line)")
    ap.add_argument("--extra-timeout", type=float, default=240.0)
    ap.add_argument("--workload", choices=("convnet", "qdq", "resnet50"), default="convnet",
                    help="convnet: BASELINE configs[2]/[3] (the metric); qdq: configs[1] (per-layer "
                         "QDQ CustomQuantizationModel, batch 256); resnet50: configs[4]")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = {"convnet": 1024, "qdq": 256, "resnet50": 512}[args.workload]
    if args.steps is None:
        args.steps = 50 if args.workload == "resnet50" else 400
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(launch_ranks(sys.argv[1:], args.gpus))
    if args.rehearse:
        return main_rehearse(args)
    if args.workload == "resnet50":
        return main_resnet(args)

    from qconvnet import data
    from qconvnet import dist as qd

    rank, world, local = qd.init()
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE {world}: the line would mislabel the run")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    mode = "qdq" if args.workload == "qdq" else "static"
    model, sd = build_model(rank, dev, args.per_channel, args.spec_file, mode)
    B = args.batch
    x = torch.from_numpy(data.synthetic_images(B, 100 + rank)).to(dev)
    use_graph = args.graph
    if use_graph:   # the forward's launches as one HIP graph (same kernels, no launch gaps)
        model.capture_graph(x)

    def forward(marks=None, slot=0):
        if marks is None and use_graph:
            return model.replay(B)
        return model.run(x, marks=marks, slot=slot)

    loop = StepLoop(forward, world, dev, sync=torch.cuda.synchronize, graph=use_graph)
    step, drain = loop.step, loop.drain

    def barrier():
        if world > 1:
            dist.barrier()

    warm_run = ramp_warmup(step, drain, args.warmup, world, dev, args.warmup_min_ms * 1e-3)

    # ---- timed region A: the metric
    elapsed, rank_ms = loop.timed(args.steps)
    images = world * B * args.steps
    value = images / elapsed
    if args.dump_outputs and rank == 0:   # the last timed step's logits
        dump_outputs(args.dump_outputs, loop.outputs())

    result = {
        "metric": METRIC if mode == "static" else METRIC_QDQ, "value": value, "unit": "images/sec", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "warmup_steps_run": warm_run,
        "warmup_note": (f"the W warmup steps, then untimed steps until >= {args.warmup_min_ms:.0f} ms of "
                        "back-to-back forwards have run (ramp_warmup; --warmup-min-ms 0 runs exactly W), "
                        "so the timed region starts at the throughput the chip holds under load"),
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "int8", "data": "synthetic", "hip_graph": bool(use_graph),
        "config": {"workload": ("full static-PTQ SimpleConvNet, all conv+linear int8 (u8 x s8 -> i32), "
                                "NHWC, per-tensor weights" if mode == "static" else
                                "per-layer QDQ SimpleConvNet (CustomQuantizationModel, BASELINE configs[1]): "
                                "every conv and fc1 int8 with the dequantize/ReLU/pool/quantize hand-off "
                                "fused, fp32 fc2") + (" [per-channel]" if args.per_channel else ""),
                   "global_batch": world * B, "per_gpu_batch": B, "image": [3, 32, 32],
                   "parallelism": f"dp{world}", "collective": "all_gather logits (RCCL)" if world > 1 else None},
    }
    if world > 1:
        result["rank_ms_per_step"] = rank_ms
        result["rank_ms_spread"] = max(rank_ms) - min(rank_ms)
    if not args.full:   # a plain run: the metric and nothing beside it
        if rank == 0:
            print(json.dumps(result))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # ---- region S: sustained throughput, >= 1 s of back-to-back steps (a
    # field beside the metric, never the metric: `value` is the K-step region)
    sustained = loop.sustained(elapsed / max(1, args.steps), args.steps, B)

    # ---- optional region C: batches in flight on several streams (serving)
    pipelined = None
    if args.pipeline > 1 and world == 1:
        S = args.pipeline
        streams = [torch.cuda.Stream(device=dev) for _ in range(S)]
        xs = [x] + [torch.from_numpy(data.synthetic_images(B, 200 + i)).to(dev) for i in range(S - 1)]
        batches = [xs[k % S] for k in range(args.steps)]
        model.run_pipelined(batches[:S], streams)   # buffers for every slot
        torch.cuda.synchronize()
        t0c = time.perf_counter()
        model.run_pipelined(batches, streams)
        torch.cuda.synchronize()
        tc = time.perf_counter() - t0c
        pipelined = {"streams": S, "value": B * args.steps / tc, "ms_per_batch": tc / args.steps * 1e3,
                     "note": "batches of the same size in flight on S HIP streams, each with its own "
                             "activation buffers and the whole forward; a serving-throughput figure, "
                             "not the metric (value is one stream, one batch after another)"}

    # ---- timed region B: per-kernel HIP events (same steps, same stream).
    # Each interval includes the dependent-launch boundary before its kernel
    # (a device-side gap: queueing the step behind a device sleep so the host
    # is ahead changed nothing, profiles/r03_diag_graph_ab.txt)
    marks_all = []
    barrier()
    torch.cuda.synchronize()
    for _ in range(args.steps):
        m = []
        step(m)
        marks_all.append(m)
    drain()
    torch.cuda.synchronize()
    names = model.kernel_names(x.shape)
    per = {n: [] for n in names}
    for m in marks_all:
        for i, n in enumerate(names):
            per[n].append(m[i].elapsed_time(m[i + 1]))
    kern = {}
    for n in names:
        ms = float(np.mean(per[n]))
        ops_ = 2.0 * MAC_PER_IMAGE[n] * B
        byts = BYTES_PER_IMAGE[n] * B
        kern[n] = {"ms": ms, "tops": ops_ / (ms * 1e-3) / 1e12,
                   "gbs": byts / (ms * 1e-3) / 1e9,
                   "bound": "hbm" if n in HBM_BOUND else "mfma"}
        kern[n]["frac"] = (kern[n]["gbs"] / PEAK_HBM_GBS if n in HBM_BOUND
                           else kern[n]["tops"] / PEAK_INT8_TOPS)
    # N > 1: the logits all-gather on its own (HIP events on the launch stream
    # around a blocking all_gather_into_tensor of this batch's logits: the
    # collective's latency as the timed step would see it if nothing hid it)
    gather = None
    if world > 1:
        gather = loop.allgather_timing(model.run(x), max(3, min(args.steps, 20)))
    dom = max(names, key=lambda n: kern[n]["ms"])
    k = kern[dom]
    if k["bound"] == "mfma":
        roof = {"kernel": dom, "bound": "mfma", "achieved": k["tops"], "peak": PEAK_INT8_TOPS,
                "unit": "TFLOP/s", "frac": k["frac"], "traffic": None,
                "note": f"int8 TOPS reported in the TFLOP/s slot; achieved = 2*MAC*{B} / mean HIP-event duration"}
    else:
        roof = {"kernel": dom, "bound": "hbm", "achieved": k["gbs"], "peak": PEAK_HBM_GBS,
                "unit": "GB/s", "frac": k["frac"], "traffic": None}
    pmc_err = "skipped (--no-pmc or N > 1)"
    if rank == 0 and world == 1 and not args.no_pmc and under_profiler():
        pmc_err = ("skipped: this run is itself under rocprofv3 (LD_PRELOAD / ROCPROF* env), "
                   "so no nested counter passes are started")
    elif rank == 0 and world == 1 and not args.no_pmc:
        pmc, pmc_err = pmc_counters(model, sd, args, names)
        for n in names:
            kern[n].update({kk: vv for kk, vv in pmc[n].items() if vv is not None})
            kn = kern[n]
            if kn.get("sq_valu_mfma_busy_cycles") and kn.get("clock_ghz") and kn.get("ms"):
                # issued MFMA cycles per SIMD over the launch's own SIMD cycles at the
                # clock the chip holds in it (GRBM_GUI_ACTIVE / 8 reads high on
                # dispatches this short, so mfma_busy_gui under-reads); equals
                # frac * 2.4 / clock when a kernel issues exactly its algorithmic MFMAs
                kn["mfma_busy"] = kn["sq_valu_mfma_busy_cycles"] / (1024.0 * kn["clock_ghz"] * 1e6 * kn["ms"])
        p = kern[dom]
        roof["traffic"] = p.get("traffic_bytes")
        roof["traffic_note"] = ("HBM bytes per launch from rocprofv3 --pmc passes of a child run "
                                "(same model, batch): 2 x FETCH_SIZE + WRITE_SIZE (gfx950 correction); "
                                f"algorithmic bytes per launch {BYTES_PER_IMAGE[dom] * B}")
        if p.get("mfma_busy") is not None:
            roof["mfma_busy"] = p["mfma_busy"]
            roof["mfma_busy_note"] = ("SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x in-kernel clock x mean "
                                      "HIP-event duration); counts issued MFMAs (32 cycles each), so it "
                                      "exceeds mfma_issue_at_clock where a kernel recomputes (config 2's "
                                      "split conv5+6 issues conv5 twice: 4/3)")
        if p.get("clock_ghz"):
            # the clock the chip holds in this kernel (in-kernel s_memtime /
            # s_memrealtime of a stamped diagnostic copy after >= 2 s of back-to-back
            # forwards, tools/clock_probe.py) and the MFMA issue fraction at it
            roof["clock_ghz_in_kernel"] = p["clock_ghz"]
            roof["mfma_issue_at_clock"] = roof["frac"] * 2.4 / p["clock_ghz"]
    if pmc_err:
        roof["pmc_error"] = pmc_err

    result.update({
        "sustained": sustained,
        "roofline": roof,
        "kernels": {n: {kk: round(vv, 4) if isinstance(vv, float) else vv for kk, vv in kern[n].items()}
                    for n in names},
    })
    if pipelined is not None:
        result["pipelined"] = pipelined
    if world > 1:
        result["allgather"] = gather
    ph = kern.get("conv1_6", {}).get("phase_table")
    if ph:
        result["phases"] = {
            "note": ("the one-launch conv1 .. conv6 phase by phase (SURVEY §8(d): conv4 and conv6 with "
                     "every layer against its own bound): median workgroup cycles and us of each phase "
                     "from the stamped diagnostic copy (tools/clock_probe.py), its MFMA cycles per SIMD, "
                     "MFMA issue at the clock the chip holds in it, and frac = issue x clock / 2.4 GHz"),
            **{k: {kk: round(vv, 4) for kk, vv in v.items()} for k, v in ph.items()}}
        lt = kern.get("conv1_6", {}).get("layer_table")
        if lt:
            result["phases"]["layers"] = {
                "note": ("conv1 .. conv6 each against its own bound (SURVEY §8(d)): inside the one launch the two "
                         "convs of a phase run on different waves of the same SIMDs at once, so a layer's row is "
                         "its role's busy cycles (stamped diagnostic copy, median over workgroups), its MFMA cycles "
                         "per SIMD, the MFMA issue while busy and frac = issue x the phase's held clock / 2.4 GHz; "
                         "conv1 is HBM-bound and its frac is its algorithmic bytes per busy time over 8 TB/s "
                         "(tools/clock_probe.py layer_table)"),
                **{k: {kk: (round(vv, 4) if isinstance(vv, float) else vv) for kk, vv in v.items()}
                   for k, v in lt.items()}}
    if rank == 0 and world == 1 and not args.no_cpu:
        cb = cpu_baselines(sd, model, args.cpu_seconds)
        result["cpu_baseline"] = cb["static_ptq"]
        if "static_ptq_batches" in cb:
            result["cpu_static_ptq_batches"] = cb["static_ptq_batches"]
        if "static_int8" in cb:
            result["cpu_static_int8"] = cb["static_int8"]
        result["top1"] = cb["top1"]
        result["gpu_vs_cpu_ratio"] = value / cb["static_ptq"]["value"]
    if rank == 0 and world == 1 and args.workload == "convnet" and not args.no_extra:
        if under_profiler():
            result["configs_extra"] = {"skipped": "this run is itself under rocprofv3: no child runs"}
        else:
            result["configs_extra"] = extra_configs(args)
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def extra_configs(args):
    """BASELINE configs[1] and configs[4] measured in the same run, each by its
    own child `bench.py --workload ...` (same rules: resident synthetic input,
    warmup, K timed steps; roofline with PMC traffic), so the driver's one
    default run carries them.  Extra keys beside the metric, never it."""
    out = {}
    for key, wl in (("configs[1]", "qdq"), ("configs[4]", "resnet50")):
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", wl, "--full", "--no-cpu"]
        # the ResNet child's own two rocprofv3 counter passes would not fit its
        # time limit beside its run: its line keeps HIP-event times only
        if args.no_pmc or wl == "resnet50":
            cmd.append("--no-pmc")
        t0 = time.perf_counter()
        try:
            p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                               timeout=args.extra_timeout)
            line = next((ln for ln in p.stdout.splitlines() if ln.startswith("{")), None)
            if p.returncode != 0 or line is None:
                out[key] = {"error": f"exit {p.returncode}: {p.stderr[-300:]}"}
                continue
            d = json.loads(line)
        except subprocess.TimeoutExpired:   # the metric above stands without these fields
            out[key] = {"error": f"timeout: the child ran past --extra-timeout {args.extra_timeout:.0f} s"}
            continue
        except Exception as e:
            out[key] = {"error": f"{type(e).__name__}: {e}"}
            continue
        keep = ("metric", "value", "unit", "steps", "warmup", "ms_per_step", "sustained", "config",
                "roofline", "kernels", "launch_ms", "conv_gmac_per_image", "conv_algorithmic_bytes_per_image")
        out[key] = {k: d[k] for k in keep if k in d}
        out[key]["child_seconds"] = time.perf_counter() - t0
    return out


# ============================================================ configs[4]
METRIC_RESNET = "images/sec at batch 512 (3×224×224) ResNet-50 bottleneck blocks, per-channel int8"


def resnet_cpu_baseline(model_fp, seconds):
    """torch.ao FX static int8 (fbgemm, per-channel weights) of the same
    ResNet-50 on the host cores, and the fp32 model the reference's
    CustomQuantizedResNet50 effectively runs (its stubs are never converted)."""
    from torch.ao.quantization import get_default_qconfig_mapping
    from torch.ao.quantization.quantize_fx import convert_fx, prepare_fx
    from models.resnet import synthetic_images
    fp = model_fp.cpu().eval()
    threads = torch.get_num_threads()
    xc = torch.from_numpy(synthetic_images(8, 21))
    with torch.no_grad():
        pq = prepare_fx(fp, get_default_qconfig_mapping("fbgemm"), example_inputs=(xc,))
        pq(xc)
        q = convert_fx(pq)
    bs = 32
    x = torch.from_numpy(synthetic_images(bs, 22))
    out = {}
    for name, m, budget in (("static_int8", q, seconds), ("fp32", fp, seconds / 2)):
        with torch.no_grad():
            m(x)
            total, iters = 0.0, 0
            while total < budget:
                t0 = time.time()
                m(x)
                total += time.time() - t0
                iters += 1
        out[name] = {"value": bs * iters / total, "unit": "images/sec", "cores": threads,
                     "cpu_count": os.cpu_count(), "kind": "port", "sample": f"batch {bs} x {iters} iters"}
    out["static_int8"]["sample"] = ("torch.ao FX static int8 (fbgemm, per-channel) of the same "
                                    "ResNet-50, " + out["static_int8"]["sample"])
    out["fp32"]["sample"] = ("fp32 ResNet-50 (what CustomQuantizedResNet50 runs: its stubs are "
                             "never converted), " + out["fp32"]["sample"])
    return out, q


RESNET_CONV_SYMBOLS = ("stem_fused_kernel", "conv_gemm_kernel", "conv1x1_stream_kernel", "conv3x3_img_kernel")


def resnet_traffic(batch, timeout=240):
    """HBM bytes per forward of the ResNet-50 conv launches (all four conv
    kernel families): rocprofv3 --pmc passes over a single-stream child run
    (FETCH_SIZE doubled per MI355X_MICROARCH.md's gfx950 correction,
    WRITE_SIZE as is), summed over the conv dispatches and divided by the
    forwards the child ran (one stem dispatch each)."""
    tot = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        agg, _ = _pmc_child((ctr,), batch, None, True, timeout, "resnet50",
                            extra=("--workload", "resnet50", "--streams", "1"), totals=True)
        fwd = next((v[ctr][1] for k, v in agg.items() if "stem_fused_kernel" in k and ctr in v), 0)
        if not fwd:
            raise RuntimeError(f"{ctr}: no stem dispatch counted")
        kib = sum(v[ctr][0] for k, v in agg.items() if ctr in v and any(sy in k for sy in RESNET_CONV_SYMBOLS))
        tot[ctr] = kib * 1024 / fwd * (2.0 if ctr == "FETCH_SIZE" else 1.0)
    return {"traffic": tot["FETCH_SIZE"] + tot["WRITE_SIZE"], "fetch_bytes": tot["FETCH_SIZE"],
            "write_bytes": tot["WRITE_SIZE"],
            "traffic_note": "HBM bytes per forward of the conv launches (batch as on the line), from "
                            "rocprofv3 --pmc passes of a single-stream child run: 2 x FETCH_SIZE + WRITE_SIZE"}


def main_resnet(args):
    from models.resnet import synthetic_images, synthetic_resnet
    from qconvnet import dist as qd
    from qconvnet.resnet import quantize_resnet

    rank, world, local = qd.init()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    B = args.batch
    # the fp32 net's BN statistics pass runs on the host, like the calibration:
    # on the GPU it differed from process to process, and with it the model
    fp = synthetic_resnet(0, device="cpu", calib_images=32)
    calib = [torch.from_numpy(synthetic_images(32, 1 + i)) for i in range(2)]
    model = quantize_resnet(fp, calib, dev, per_channel=True)
    model.fuse_reduce = not args.separate_reduce
    x = torch.from_numpy(synthetic_images(B, 100 + rank)).to(dev)
    gathered = torch.empty((world * B, model.num_classes), dtype=torch.float32,
                           device=dev) if world > 1 else None

    use_graph = args.graph
    if use_graph:   # the forward's launches as one HIP graph (same kernels, no launch gaps)
        model.capture_graph(x)

    def step(marks=None):
        if marks is None and use_graph:
            logits = model.replay(B)
        elif marks is None and args.streams > 1:
            logits = model.run_streams(x, args.streams)
        else:
            logits = model.run(x, marks=marks)
        if world > 1:
            qd.gather_logits(logits, gathered)
        return gathered if world > 1 else logits

    def barrier():
        if world > 1:
            dist.barrier()

    warm_run = ramp_warmup(step, lambda: None, args.warmup, world, dev, args.warmup_min_ms * 1e-3)
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = None
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([elapsed], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    value = world * B * args.steps / elapsed
    if args.dump_outputs and rank == 0 and out is not None:   # the last timed step's logits
        dump_outputs(args.dump_outputs, {"logits": out})
    result = {
        "metric": METRIC_RESNET, "value": value, "unit": "images/sec", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "warmup_steps_run": warm_run,
        "ms_per_step": elapsed / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "int8",
        "data": "synthetic",
        "config": {"workload": "ResNet-50 (stem, 16 bottleneck blocks, avgpool, fc) static int8, "
                               "per-channel weights, u8 NHWC activations",
                   "global_batch": world * B, "per_gpu_batch": B, "image": [3, 224, 224],
                   "parallelism": f"dp{world}", "streams": args.streams},
    }
    if not args.full:   # a plain run: the metric and nothing beside it
        if rank == 0:
            print(json.dumps(result))
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    # MACs per image of every conv launch, in forward order
    convs = model.conv_layers()
    hh = (x.shape[2] + 2 * convs[0].py - convs[0].kh) // convs[0].sy + 1   # stem output
    sizes = [hh * hh]
    hh = (hh - 1) // 2 + 1                                                   # maxpool
    for b in model.blocks:   # launch order: [ds], c1, c2, c3 (conv_layers())
        ho = (hh + 2 * b["c2"].py - b["c2"].kh) // b["c2"].sy + 1
        sizes += ([ho * ho] if b["ds"] is not None else []) + [hh * hh, ho * ho, ho * ho]
        hh = ho
    mac_img = [sz * d.cout * d.w.shape[0] * 32 for sz, d in zip(sizes, convs)]  # K = chunks*32
    # algorithmic HBM bytes per image of the conv launches, layer by layer: the
    # stem reads the fp32 image and writes its max-pooled map; every other conv
    # reads its u8 input map and writes its u8 output (the expand conv also
    # reads the block's identity for the residual join)
    hh = (x.shape[2] + 2 * convs[0].py - convs[0].kh) // convs[0].sy + 1
    hh = (hh - 1) // 2 + 1
    cin = convs[0].cout
    conv_bytes = 3 * x.shape[2] * x.shape[3] * 4 + hh * hh * cin
    for b in model.blocks:
        ho = (hh + 2 * b["c2"].py - b["c2"].kh) // b["c2"].sy + 1
        c1, c2, c3 = b["c1"].cout, b["c2"].cout, b["c3"].cout
        if b["ds"] is not None:
            conv_bytes += hh * hh * cin + ho * ho * c3
        conv_bytes += hh * hh * cin + hh * hh * c1          # c1 (1x1)
        conv_bytes += hh * hh * c1 + ho * ho * c2           # c2 (3x3, the block's stride)
        conv_bytes += ho * ho * c2 + 2 * ho * ho * c3       # c3 (1x1) + identity read
        hh, cin = ho, c3
    per_name = {}
    n_rep = max(3, min(args.steps, 10))
    conv_ms = []
    for _ in range(n_rep):
        m = []
        step(m)
        torch.cuda.synchronize()
        tot_conv = 0.0
        for (_, e0), (n1, e1) in zip(m[:-1], m[1:]):
            ms = e0.elapsed_time(e1)
            per_name.setdefault(n1, []).append(ms)
            if n1 == "conv":
                tot_conv += ms
        conv_ms.append(tot_conv)
    conv_ms = float(np.mean(conv_ms))
    conv_ops = 2.0 * sum(mac_img) * B
    tops = conv_ops / (conv_ms * 1e-3) / 1e12
    roof = {"kernel": "conv_gemm_kernel / conv1x1_stream_kernel (every conv launch; layer 1's three "
                      "expand + join launches also run the next reduce conv)", "bound": "mfma", "achieved": tops,
            "peak": PEAK_INT8_TOPS, "unit": "TFLOP/s", "frac": tops / PEAK_INT8_TOPS, "traffic": None,
            "algorithmic_bytes": conv_bytes * B,
            "note": "int8 TOPS in the TFLOP/s slot; achieved = 2*sum(conv MAC)*batch / summed "
                    "HIP-event conv time; stem MACs counted at the packed K=224 actually issued; "
                    "algorithmic_bytes counts every conv's input and output layer by layer, including "
                    "the three fused reduces' 256-channel inputs, which in the fused launches never "
                    "leave the chip"}
    if rank == 0 and world == 1 and not args.no_pmc:
        if under_profiler():
            roof["pmc_error"] = "skipped: this run is itself under rocprofv3"
        else:
            try:
                roof.update(resnet_traffic(B))
            except Exception as e:   # the fields stay null
                roof["pmc_error"] = f"{type(e).__name__}: {e}"
    result.update({
        "roofline": roof,
        "launch_ms": {k: round(float(np.sum(v) / n_rep), 4) for k, v in per_name.items()},
        "conv_gmac_per_image": sum(mac_img) / 1e9,
        "conv_algorithmic_bytes_per_image": conv_bytes,
    })
    if rank == 0 and world == 1 and not args.no_cpu:
        cb, q_cpu = resnet_cpu_baseline(fp, args.cpu_seconds)
        result["cpu_baseline"] = cb["static_int8"]
        result["cpu_fp32"] = cb["fp32"]
        xe = synthetic_images(64, 31)
        with torch.no_grad():
            lab = fp.cpu()(torch.from_numpy(xe)).argmax(1)
            g = model(torch.from_numpy(xe)).argmax(1)
            c = q_cpu(torch.from_numpy(xe)).argmax(1)
        result["top1_vs_fp32"] = {"gpu_int8": (g == lab).float().mean().item() * 100,
                                  "cpu_torchao_int8": (c == lab).float().mean().item() * 100,
                                  "images": 64}
    if rank == 0:
        print(json.dumps(result))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
