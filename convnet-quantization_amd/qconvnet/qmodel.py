"""The int8 SimpleConvNet executor on MI355X.

``QuantizedConvNet`` holds the quantized model in HBM (packed s8 weights,
per-channel fp32 epilogue constants, int32 zero-point corrections) and runs the
forward as a fixed sequence of hand-written HIP kernels on the current stream:

  static (full int8, BASELINE config 3):
    conv1_f32 (quantize + conv1 + ReLU)  -> conv2(+pool) -> conv3 -> conv4(+pool)
    -> conv5 -> conv6(+pool) -> fc1(+ReLU) -> fc2 (+ DeQuantStub, fp32 logits)
  qdq (per-layer QDQ, BASELINE config 2 — custom_quantization_model.py:202-261
       with its stubs live):
    every conv requantizes to its own output qparams, then the epilogue does
    dequantize -> ReLU -> quantize(next layer's input qparams); fc1 likewise,
    then the fp32 fc2.

Activations stay u8 NHWC in HBM between layers; nothing is staged through the
host.  A forward at a fixed batch can be captured into a HIP graph
(``capture_graph``) so a step is one graph launch.

Reference interfaces mirrored: SURVEY.md §8(a) A0-A11; the quantize() flow of
/root/reference/models/custom_quantization_model.py:169-195 (eval, cpu, fold)
plus torch.ao prepare/convert with MinMax observers (observer.py:349-427).
"""
from __future__ import annotations


import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from . import quant as Q
from .data import CIFAR_MEAN, CIFAR_STD

F32 = np.float32
CONV_TABLE = ((3, 64, False), (64, 64, True), (64, 128, False), (128, 128, True),
              (128, 256, False), (256, 256, True))


# ============================================================ fp32 folding
def fold_state_dict(sd):
    """BN-fold a SimpleConvNet state_dict (fuse_modules of
    custom_quantization_model.py:180-190): conv_i+bn_i, fc1+bn7; fc2 as is."""
    g = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in sd.items()}
    out = {}
    for i in range(1, 7):
        out[f"conv{i}.w"], out[f"conv{i}.b"] = Q.fold_bn(
            g[f"conv{i}.weight"], g.get(f"conv{i}.bias"), g[f"bn{i}.running_mean"],
            g[f"bn{i}.running_var"], g[f"bn{i}.weight"], g[f"bn{i}.bias"])
    out["fc1.w"], out["fc1.b"] = Q.fold_linear_bn(
        g["fc1.weight"], g.get("fc1.bias"), g["bn7.running_mean"], g["bn7.running_var"],
        g["bn7.weight"], g["bn7.bias"])
    out["fc2.w"] = np.asarray(g["fc2.weight"], F32)
    out["fc2.b"] = np.asarray(g["fc2.bias"], F32)
    return out


# ============================================================ raw u8 input
def normalized_input(x, device, ntab):
    """The fp32 NCHW tensor a model consumes, on ``device``.  fp32 input is
    moved as it is.  A uint8 batch must be NHWC [N,H,W,3] (ValueError
    otherwise — raw bytes are never cast to float); its bytes are moved and
    then expanded through ``ntab`` (Q.normalize_table): by the HIP kernel on
    the GPU, by indexing on the CPU, both bit-equal to ToTensor + Normalize."""
    dev = torch.device(device)
    if x.dtype != torch.uint8:
        return x.to(dev, torch.float32)
    Q.check_u8_images(x)
    x = x.to(dev)
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            return ops.normalize_u8(x, ntab.to(dev))
    return Q.expand_u8(x, ntab)


# ============================================================ calibration
class _Range:
    """Running min/max of one activation; device observer kernel on GPU,
    torch.aminmax on CPU (observer.py:558-569)."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.obs = ops.MinMaxObserver(self.dev) if self.dev.type == "cuda" else None
        self.lo, self.hi = np.float32(np.inf), np.float32(-np.inf)

    def __call__(self, x):
        if x.numel() == 0:
            return
        if self.obs is not None:
            self.obs(x.contiguous())
        else:
            lo, hi = torch.aminmax(x.detach())
            self.lo = min(self.lo, np.float32(lo.item()))
            self.hi = max(self.hi, np.float32(hi.item()))

    def values(self):
        return self.obs.values() if self.obs is not None else (self.lo, self.hi)


class _HistRange:
    """torch.ao's HistogramObserver(reduce_range=False) on one activation
    (observer.py:1289-1370): the HIP histogram kernel on GPU, torch.aminmax +
    torch.histc on CPU, the same host combine and search behind both.
    values() is the searched clipping range, not the raw min/max."""

    def __init__(self, device):
        self.dev = torch.device(device)
        self.obs = ops.HistogramObserver(self.dev) if self.dev.type == "cuda" else \
            Q.HistogramState()

    def __call__(self, x):
        if x.numel() == 0:
            return
        if self.dev.type == "cuda":
            self.obs(x.contiguous())
        else:
            self.obs.observe_host(x)

    def values(self):
        return self.obs.values() if self.dev.type == "cuda" else self.obs.search()


_OBSERVERS = {"minmax": _Range, "histogram": _HistRange}


def _observed_names(mode):
    """The observers build_qspec(mode) reads; all of them for mode None."""
    convs = [f"conv{i}" for i in range(1, 7)]
    if mode is None:
        return ["x"] + [f"{c}_{s}" for c in convs for s in ("in", "out")] + \
            ["fc1_in", "fc1_out", "fc2_out"]
    if mode == "static":
        return ["x"] + [f"{c}_out" for c in convs] + ["fc1_out", "fc2_out"]
    if mode == "qdq":
        return [f"{c}_{s}" for c in convs for s in ("in", "out")] + ["fc1_in", "fc1_out"]
    raise ValueError(f"unknown mode {mode!r}")


def calibrate(folded, batches, device="cpu", observer="minmax", mode=None, mean=CIFAR_MEAN,
              std=CIFAR_STD):
    """Run the BN-folded fp32 net over calibration batches and record the
    range of every observer ``mode`` needs ("static", "qdq"; None: those of
    both) as {name: (lo, hi)} for build_qspec.  Batches are normalised fp32
    NCHW, or raw uint8 NHWC [N,32,32,3] images, normalised here with
    ``mean`` / ``std`` (the ranges equal those of the fp32-fed calibration
    bit for bit).

    observer="minmax" (default): the running min/max.  observer="histogram":
    torch.ao's default HistogramObserver (2048 bins, reduce_range=False); the
    range is its searched clipping range, so Q.qparams_affine of it is
    calculate_qparams().  A histogram cannot be clamped after the fact the way
    build_qspec's _relu_range clamps a min/max, so with mode="static" the
    conv{i}_out / fc1_out histogram observers see the POST-ReLU tensor, as the
    output observers of torch.ao's fused ConvReLU2d / LinearReLU do (and
    _relu_range is then a no-op); with mode="qdq" they see the pre-ReLU
    output, as the per-layer stubs do.  The mode is therefore required."""
    if observer not in _OBSERVERS:
        raise ValueError(f"unknown observer {observer!r} (expected one of {sorted(_OBSERVERS)})")
    if observer == "histogram" and mode is None:
        raise ValueError("observer='histogram' needs mode='static' or 'qdq'")
    names = _observed_names(mode)
    post_relu = observer == "histogram" and mode == "static"
    dev = torch.device(device)
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in folded.items()}
    rng = {n: _OBSERVERS[observer](dev) for n in names}
    ntab = Q.normalize_table(mean, std).to(dev)

    def see(name, x):
        if name in rng:
            rng[name](x)

    with torch.no_grad():
        for xb in batches:
            x = normalized_input(xb, dev, ntab)
            see("x", x)
            for i, (_, _, pool) in enumerate(CONV_TABLE, start=1):
                see(f"conv{i}_in", x)
                x = F.conv2d(x, t[f"conv{i}.w"], t[f"conv{i}.b"], padding=1)
                if not post_relu:
                    see(f"conv{i}_out", x)
                x = F.relu(x)
                if post_relu:
                    see(f"conv{i}_out", x)
                if pool:
                    x = F.max_pool2d(x, 2, 2)
            x = x.reshape(x.shape[0], -1)
            see("fc1_in", x)
            x = F.linear(x, t["fc1.w"], t["fc1.b"])
            if not post_relu:
                see("fc1_out", x)
            x = F.relu(x)
            if post_relu:
                see("fc1_out", x)
            x = F.linear(x, t["fc2.w"], t["fc2.b"])
            see("fc2_out", x)
    return {n: r.values() for n, r in rng.items()}


def _relu_range(lo_hi):
    lo, hi = lo_hi
    return max(F32(lo), F32(0.0)), max(F32(hi), F32(0.0))


def _weight_scale(w, per_channel):
    if per_channel:
        flat = w.reshape(w.shape[0], -1)
        return Q.qparams_symmetric(flat.min(1), flat.max(1))
    return Q.qparams_symmetric(w.min(), w.max())


def build_qspec(folded, ranges, mode="static", per_channel=False):
    """Host quantized-model description (numpy) from folded fp32 weights and
    observed ranges.  Layer entries: w (s8 OIHW / OI), b, s_w, s_x, z_x, s_y,
    z_y, relu (+ next (s2, z2) for the QDQ hand-off)."""
    spec = {"mode": mode, "per_channel": bool(per_channel)}
    if mode == "static":
        s_in, z_in = Q.qparams_affine(*ranges["x"])
        spec["in"] = (s_in, z_in)
        s_x, z_x = s_in, z_in
        for i in range(1, 7):
            w = folded[f"conv{i}.w"]
            s_w = _weight_scale(w, per_channel)
            s_y, z_y = Q.qparams_affine(*_relu_range(ranges[f"conv{i}_out"]))
            spec[f"conv{i}"] = dict(w=Q.quantize_weight(w, s_w), b=folded[f"conv{i}.b"], s_w=s_w,
                                    s_x=s_x, z_x=z_x, s_y=s_y, z_y=z_y, relu=True)
            s_x, z_x = s_y, z_y
        w = folded["fc1.w"]
        s_w = _weight_scale(w, per_channel)
        s_y, z_y = Q.qparams_affine(*_relu_range(ranges["fc1_out"]))
        spec["fc1"] = dict(w=Q.quantize_weight(w, s_w), b=folded["fc1.b"], s_w=s_w, s_x=s_x,
                           z_x=z_x, s_y=s_y, z_y=z_y, relu=True)
        w = folded["fc2.w"]
        s_w = _weight_scale(w, per_channel)
        s_y2, z_y2 = Q.qparams_affine(*ranges["fc2_out"])
        spec["fc2"] = dict(w=Q.quantize_weight(w, s_w), b=folded["fc2.b"], s_w=s_w, s_x=s_y,
                           z_x=z_y, s_y=s_y2, z_y=z_y2, relu=False)
    elif mode == "qdq":
        for i in range(1, 7):
            w = folded[f"conv{i}.w"]
            s_w = _weight_scale(w, per_channel)
            s_x, z_x = Q.qparams_affine(*ranges[f"conv{i}_in"])
            s_y, z_y = Q.qparams_affine(*ranges[f"conv{i}_out"])
            spec[f"conv{i}"] = dict(w=Q.quantize_weight(w, s_w), b=folded[f"conv{i}.b"], s_w=s_w,
                                    s_x=s_x, z_x=z_x, s_y=s_y, z_y=z_y, relu=False)
        w = folded["fc1.w"]
        s_w = _weight_scale(w, per_channel)
        s_x, z_x = Q.qparams_affine(*ranges["fc1_in"])
        s_y, z_y = Q.qparams_affine(*ranges["fc1_out"])
        spec["fc1"] = dict(w=Q.quantize_weight(w, s_w), b=folded["fc1.b"], s_w=s_w, s_x=s_x,
                           z_x=z_x, s_y=s_y, z_y=z_y, relu=False)
        spec["fc2"] = dict(w=folded["fc2.w"], b=folded["fc2.b"])
        for i in range(1, 6):
            spec[f"conv{i}"]["next"] = (spec[f"conv{i + 1}"]["s_x"], spec[f"conv{i + 1}"]["z_x"])
        spec["conv6"]["next"] = (spec["fc1"]["s_x"], spec["fc1"]["z_x"])
    else:
        raise ValueError(f"unknown mode {mode!r}")
    return spec


def qspec_from_torch_ao(q):
    """Import a torch.ao-converted full-int8 SimpleConvNet (quant stub, fused
    Conv(ReLU)2d conv1..conv6, LinearReLU fc1, Linear fc2) — the model a
    reference user builds with prepare/convert — into a static qspec."""
    spec = {"mode": "static", "per_channel": False,
            "in": (F32(q.quant.scale.item()), int(q.quant.zero_point.item()))}
    s_x, z_x = spec["in"]
    for name in [f"conv{i}" for i in range(1, 7)] + ["fc1", "fc2"]:
        m = getattr(q, name)
        wq = m.weight()
        if wq.qscheme() in (torch.per_tensor_symmetric, torch.per_tensor_affine):
            s_w = F32(wq.q_scale())
        else:
            s_w = wq.q_per_channel_scales().numpy().astype(F32)
            spec["per_channel"] = True
        spec[name] = dict(w=wq.int_repr().numpy(), b=m.bias().detach().numpy().astype(F32), s_w=s_w,
                          s_x=s_x, z_x=z_x, s_y=F32(m.scale), z_y=int(m.zero_point),
                          relu=name != "fc2")
        s_x, z_x = F32(m.scale), int(m.zero_point)
    return spec


# ============================================================ device model
def cuda_device(device):
    """torch.device with an explicit index ("cuda" -> the current device), so
    launches can enter it and inputs can be checked against it."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the int8 path runs on the GPU (HIP); pass a cuda device")
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


class _DevLayer:
    pass


class QuantizedConvNet:
    """Duck-typed int8 model object (the surface of the reference's models.*:
    eval(), to() in place, cpu(), __call__; fp32 [N,3,32,32] in, fp32 [N,10] out).

    Raw images are accepted too: a uint8 NHWC batch [N,32,32,3] is normalised
    with ``mean`` / ``std`` and quantized by table lookups inside the conv1+conv2
    stage (a quarter of the input bytes, no host preprocessing); the logits
    equal those of the normalised fp32 batch bit for bit."""

    def __init__(self, spec, device="cuda", fuse12=True, mean=CIFAR_MEAN, std=CIFAR_STD):
        self.spec = spec
        self.mean, self.std = tuple(mean), tuple(std)
        self.mode = spec["mode"]
        self.device = cuda_device(device)
        self.quantized = True
        self.is_custom_quantized = self.mode == "qdq"
        self.host_io = False
        self.fuse12 = fuse12
        self.fuse_pairs = True   # conv3+conv4 / conv5+conv6 as one launch each
        self.fc_head = True      # fc1 -> fc2 as the split-K head (False: two linear launches)
        # QuantStub + conv1 .. conv6 as one persistent launch where the library
        # takes it (>= 4 images per CU; False: conv12 + the two pair launches)
        self.fuse_convs = True
        # conv12 as its own launch, then conv3 .. conv6 in one launch of
        # one-wave-per-SIMD workgroups (qcn_convs36_u8s8, r06) instead of the
        # one-launch conv1 .. conv6 (fuse_convs), from 4 images per CU
        self.convs_w4 = False
        self._plans = {}         # (input shape, keep, the five switches) -> launch plan
        self._conv_layers = None
        self._bufs = {}
        self._graphs = {}
        self._upload()

    # --------------------------------------------------------------- setup
    def _t(self, a, dtype=None):
        t = torch.from_numpy(np.ascontiguousarray(a))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device)

    def _upload(self):
        sp = self.spec
        self.L = []
        for i, (cin, cout, pool) in enumerate(CONV_TABLE, start=1):
            e = sp[f"conv{i}"]
            d = _DevLayer()
            d.cin, d.cout, d.pool, d.relu = cin, cout, pool, e["relu"]
            if i == 1:
                packed, wsum = ops.pack_conv1(e["w"])
            else:
                packed, wsum = ops.pack_conv3x3(e["w"])
            u, v, mult = Q.epilogue_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])
            d.w = self._t(packed)
            d.u, d.v, d.mult = self._t(u), self._t(v), self._t(mult)
            d.corr = self._t(((128 - int(e["z_x"])) * wsum.astype(np.int64)).astype(np.int32))
            d.z_x, d.z_y, d.s_x, d.s_y = int(e["z_x"]), int(e["z_y"]), F32(e["s_x"]), F32(e["s_y"])
            d.qdq = ops.qdq_struct(e["s_y"], e["z_y"], *e["next"]) if "next" in e else None
            self.L.append(d)
        if self.mode == "static":
            self.in_scale, self.in_zp = sp["in"]
        else:
            self.in_scale, self.in_zp = sp["conv1"]["s_x"], sp["conv1"]["z_x"]
        # u8 image input: ToTensor + Normalize per (channel, byte), and the
        # QuantStub of that with the input qparams
        ntab = Q.normalize_table(self.mean, self.std)
        self.ntab = ntab.to(self.device)
        self.qlut = Q.quantize_table(ntab, self.in_scale, self.in_zp).to(self.device)
        perm = Q.nhwc_flatten_perm()
        for name in ("fc1", "fc2"):
            e = sp[name]
            d = _DevLayer()
            if self.mode == "qdq" and name == "fc2":
                d.w = self._t(np.asarray(e["w"], F32))
                d.b = self._t(np.asarray(e["b"], F32))
                setattr(self, name, d)
                continue
            w = np.asarray(e["w"], np.int8)
            if name == "fc1":
                w = np.ascontiguousarray(w[:, perm])  # NHWC flatten order
            wsum = w.astype(np.int64).sum(1)
            u, v, mult = Q.epilogue_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])
            d.w = self._t(w)
            if name == "fc1" and w.shape[1] % 32 == 0:
                d.wk = self._t(ops.pack_fc_kmajor(w))   # classifier-head layout
            d.u, d.v, d.mult = self._t(u), self._t(v), self._t(mult)
            d.corr = self._t(((128 - int(e["z_x"])) * wsum).astype(np.int32))
            d.z_x, d.z_y, d.s_y, d.relu = int(e["z_x"]), int(e["z_y"]), F32(e["s_y"]), e["relu"]
            setattr(self, name, d)

    def buffers(self, n, slot=0):
        """The device activation buffers run() used for batch size n (slot:
        run_pipelined's buffer set): a2, a4, a6 / a6k, f1, q, logits, ..."""
        return self._bufs[(n, slot)]

    def _buffers(self, n, slot=0):
        b = self._bufs.get((n, slot))
        if b is None:
            dev = self.device
            b = {"a1": torch.empty((n, 32, 32, 64), dtype=torch.uint8, device=dev),
                 "a2": torch.empty((n, 16, 16, 64), dtype=torch.uint8, device=dev),
                 "a3": torch.empty((n, 16, 16, 128), dtype=torch.uint8, device=dev),
                 "a4": torch.empty((n, 8, 8, 128), dtype=torch.uint8, device=dev),
                 "a5": torch.empty((n, 8, 8, 256), dtype=torch.uint8, device=dev),
                 "a6": torch.empty((n, 4, 4, 256), dtype=torch.uint8, device=dev),
                 "f1": torch.empty((n, 512), dtype=torch.uint8, device=dev),
                 "f1f": torch.empty((n, 512), dtype=torch.float32, device=dev),
                 "q": torch.empty((n, 10), dtype=torch.uint8, device=dev),
                 "logits": torch.empty((n, 10), dtype=torch.float32, device=dev)}
            self._bufs[(n, slot)] = b
        return b

    def _lazy(self, b, name):
        """A buffer only some plans use (conv6's chunk-major output, the
        normalised fp32 copy of raw images, the head's workspace), made on
        its first use in buffer set ``b``."""
        t = b.get(name)
        if t is None:
            n = b["a2"].shape[0]
            if name == "a6k":
                t = torch.empty((128, n, 32), dtype=torch.uint8, device=self.device)
            elif name == "xf":
                t = torch.empty((n, 3, 32, 32), dtype=torch.float32, device=self.device)
            else:
                t = ops.classifier_workspace(n, self.fc1.w.shape[0], self.device)
            b[name] = t
        return t

    # --------------------------------------------------------------- forward
    def kernel_names(self, x_shape, keep=False):
        """Names of the launches run() marks, in order (conv1+conv2 are one
        launch when fused, conv3+conv4 / conv5+conv6 one launch each when
        paired, fc1+fc2 one "fc12" slot for the fused head)."""
        return tuple(name for name, _ in self._plan(x_shape, keep))

    def _pairs(self, keep):
        """conv3+conv4 and conv5+conv6 as fused block launches (their middle
        activation stays in LDS); keep=True runs them per layer so every
        activation is inspectable."""
        return self.fuse_pairs and not keep

    def _head_fused(self, n):
        f1, f2 = self.fc1, self.fc2
        if not self.fc_head:
            return False
        c6 = self.L[5]
        common = (n % 128 == 0 and f1.w.shape[0] == 512 and f1.w.shape[1] == 4096 and
                  hasattr(f1, "wk") and f2.w.shape[0] <= 16 and c6.cout == 256 and c6.pool)
        if self.mode == "qdq":   # conv6's QDQ hand-off writes fc1's u8 input chunk-major
            return common
        return common and self.mode == "static" and f2.z_x == f1.z_y and c6.qdq is None

    def _head(self, n, keep):
        """The split-K classifier head runs (in QDQ mode only behind the conv5+6
        pair, whose epilogue applies conv6's QDQ hand-off to the chunk-major
        output; the per-layer chunk-major conv6 has no hand-off)."""
        return self._head_fused(n) and (self.mode != "qdq" or self._pairs(keep))

    def _fused(self, x_shape):
        # fp32 NCHW or raw u8 NHWC images
        return self.fuse12 and tuple(x_shape[1:]) in ((3, 32, 32), (32, 32, 3))

    def _convs_form(self, n, head):
        """The library's host query (no launch) for the one-launch convs at
        batch n: 1 one image per workgroup, 2 persistent, 0 not taken."""
        if self._conv_layers is None:
            self._conv_layers = ops.conv_layers(self.L, self.in_zp)
        with torch.cuda.device(self.device):
            return ops.convnet_convs_form(n, self.in_scale, self.in_zp, self._conv_layers, kmajor=head)

    def _plan(self, x_shape, keep):
        """The launch plan of a forward: a tuple of (name, step), one per
        launch run() marks, each step a callable of (input, buffer set).
        Built once per input shape, keep and switch setting (tests and tools
        flip the switches between forwards), so a later forward asks the
        library nothing."""
        key = (tuple(x_shape), keep, self.fuse12, self.fuse_pairs, self.fc_head, self.fuse_convs, self.convs_w4)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._plans[key] = self._build_plan(key[0], keep)
        return plan

    def _build_plan(self, x_shape, keep):
        n, L = x_shape[0], self.L
        fused, pairs, head = self._fused(x_shape), self._pairs(keep), self._head(n, keep)
        out6 = "a6k" if head else "a6"   # conv6 writes the head's chunk-major input
        acts = ["a1", "a2", "a3", "a4", "a5", "a6"]
        steps = []

        def step(name):
            def add(fn):
                steps.append((name, fn))
            return add

        def must(ok, what):
            if not ok:
                raise RuntimeError(f"{what} rejected a launch the plan chose")

        # the one-launch forms take what the library's plan function takes:
        # form 1 (one image per workgroup) or 2 (persistent, all of conv3 ..
        # conv6 on one epilogue form); the conv3 .. conv6 launch is form 2's
        form = self._convs_form(n, head) if fused and pairs and (self.fuse_convs or self.convs_w4) else 0
        w4 = self.convs_w4 and form == 2
        if self.fuse_convs and form > 0 and not w4:
            @step("conv1_6")
            def _(x, b):
                if x.dtype == torch.uint8:
                    ok = ops.convnet_convs_u8(x, self.qlut, self.in_zp, self._conv_layers, b["a2"], b["a4"],
                                              self._lazy(b, out6), kmajor=head)
                else:
                    ok = ops.convnet_convs(x, self.in_scale, self.in_zp, self._conv_layers, b["a2"], b["a4"],
                                           self._lazy(b, out6), kmajor=head)
                must(ok, "one-launch convs")
            first = 6
        elif fused:
            @step("conv12")
            def _(x, b):
                if x.dtype == torch.uint8:
                    ops.conv12_fused_u8(x, self.qlut, self.in_zp, L[0], L[1], out=b["a2"])
                else:
                    ops.conv12_fused(x, self.in_scale, self.in_zp, L[0], L[1], out=b["a2"])
            first = 2
        else:
            @step("conv1")
            def _(x, b):
                d = L[0]
                if x.dtype == torch.uint8:   # the stand-alone conv1 has no u8 stage: normalise first
                    x = ops.normalize_u8(x, self.ntab, out=self._lazy(b, "xf"))
                ops.conv1_f32(x, self.in_scale, self.in_zp, d.w, d.u, d.v, d.mult, d.corr, d.z_y, d.relu, d.qdq,
                              out=b["a1"])
            first = 1
        if w4:
            @step("conv3_6")
            def _(x, b):
                must(ops.convs36(b["a2"], self._conv_layers, b["a4"], self._lazy(b, out6), kmajor=head),
                     "conv3 .. conv6 launch")
            first = 6

        def conv_pair(i, src, dst):   # conv3+conv4, conv5+conv6 in one launch each
            @step(f"conv{i + 1}{i + 2}")
            def _(x, b):
                must(ops.conv_pair(b[src], L[i], L[i + 1], self._lazy(b, dst), kmajor=dst == "a6k"), "fused conv pair")

        def conv(i, src, dst):
            d = L[i]

            @step(f"conv{i + 1}")
            def _(x, b):
                if dst == "a6k":   # conv6 writes the classifier's chunk-major input
                    must(ops.conv3x3_kmajor(b[src], d.z_x, d.w, d.cout, d.u, d.v, d.mult, d.corr, d.z_y, d.relu,
                                            d.pool, self._lazy(b, dst)), "chunk-major conv6")
                else:
                    ops.conv3x3(b[src], d.z_x, d.w, d.cout, d.u, d.v, d.mult, d.corr, d.z_y, d.relu, d.pool,
                                d.qdq, out=b[dst])

        i = first
        while i < 6:   # L[i] is conv i+1: it reads acts[i - 1]
            if pairs and i in (2, 4):
                conv_pair(i, acts[i - 1], out6 if i == 4 else acts[i + 1])
                i += 2
            else:
                conv(i, acts[i - 1], out6 if i == 5 else acts[i])
                i += 1

        f1, f2 = self.fc1, self.fc2
        if head:
            @step("fc12")
            def _(x, b):
                must(self._classifier(b["a6k"], b), "classifier head")
                if keep:  # NHWC view of conv6's output for inspection / parity tests
                    b["a6"].copy_(ops.from_kmajor(b["a6k"]).view(n, 4, 4, 256))
        elif self.mode == "static":
            @step("fc1")
            def _(x, b):
                ops.linear_u8(b["a6"].view(n, 4096), f1.z_x, f1.w, f1.u, f1.v, f1.mult, f1.corr, f1.z_y, True,
                              out=b["f1"])

            @step("fc2")
            def _(x, b):
                ops.linear_u8(b["f1"], f2.z_x, f2.w, f2.u, f2.v, f2.mult, f2.corr, f2.z_y, False,
                              y_scale=f2.s_y, want_fp32=True, out=b["q"], out_f=b["logits"])
        else:
            @step("fc1")
            def _(x, b):
                ops.linear_u8(b["a6"].view(n, 4096), f1.z_x, f1.w, f1.u, f1.v, f1.mult, f1.corr, f1.z_y, False,
                              y_scale=f1.s_y, want_fp32=True, out=b["f1"], out_f=b["f1f"])

            @step("fc2")
            def _(x, b):
                ops.linear_f32(b["f1f"], f2.w, f2.b, relu_in=True, out=b["logits"])
        return tuple(steps)

    def run(self, x, keep=False, marks=None, slot=0):
        """Launch the whole int8 forward on the current stream of the model's
        device (no sync).
        Returns the fp32 logits tensor (a reused buffer); with keep=True also
        the dict of intermediate u8 activations.  ``marks``: a list that
        receives one timing event before the first launch and one after each
        launch named by kernel_names(x.shape).  ``x``: fp32 NCHW
        [N,3,32,32], or raw uint8 NHWC [N,32,32,3] images."""
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        if x.dtype == torch.uint8:
            Q.check_u8_images(x, 32)
            x = x.contiguous()
        with torch.cuda.device(self.device):   # ops launch on this device's current stream
            return self._run(x, keep, marks, slot)

    def _run(self, x, keep, marks, slot=0):
        b = self._buffers(x.shape[0], slot)

        def mark():
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append(ev)

        mark()
        for _, step in self._plan(x.shape, keep):
            step(x, b)
            mark()
        if keep:
            return b["logits"], b
        return b["logits"]

    def _classifier(self, xk, b):
        """fc1+ReLU -> fc2 -> dequantize in two launches (split-K fc1 on the
        chunk-major conv6 output + a per-row finisher); in QDQ mode fc1's
        dequantize, ReLU and the fp32 fc2 run in the finisher."""
        f1, f2 = self.fc1, self.fc2
        ws = self._lazy(b, "ws")
        if self.mode == "qdq":
            return ops.classifier_qdq(xk, f1, f2, ws, b["f1"], b["logits"])
        f1.relu, f2.relu = True, False
        return ops.classifier(xk, f1, f2, ws, b["f1"], b["q"], b["logits"])

    def run_pipelined(self, batches, streams):
        """Forward a sequence of batches with len(streams) of them in flight:
        batch k runs on streams[k % S] with its own activation buffers (slot
        k % S), so one batch's launches fill the ramp / drain of another's
        (every batch still goes through every layer at its own batch size).
        Returns the logits tensors (reused buffers, one per slot); no sync."""
        S = len(streams)
        cur = torch.cuda.current_stream(self.device)
        for s in streams:
            s.wait_stream(cur)
        outs = []
        for k, x in enumerate(batches):
            with torch.cuda.stream(streams[k % S]):
                outs.append(self.run(x, slot=k % S))
        for s in streams:
            cur.wait_stream(s)
        return outs

    def capture_graph(self, x_static):
        """Capture run(x_static) into a HIP graph; replay with replay(n)."""
        n = x_static.shape[0]
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self.run(x_static)  # warm-up: kernel attributes, buffers
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = self.run(x_static)
        self._graphs[n] = (g, x_static, out)
        return g

    def replay(self, n):
        g, _, out = self._graphs[n]
        g.replay()
        return out

    @torch.no_grad()
    def forward(self, x):
        host = not x.is_cuda
        if x.dtype == torch.uint8:   # raw images: the bytes go to the device as they are
            Q.check_u8_images(x, 32)
            xd = x.to(self.device, non_blocking=False).contiguous()
        else:
            xd = x.to(self.device, torch.float32, non_blocking=False).contiguous()
        out = self.run(xd).clone()
        if host or self.host_io:
            return out.cpu()
        # the reference harness times model(data) with time.time() and no device
        # sync (utils/inference_benchmark.py:94-98): finish the work here.
        torch.cuda.current_stream(self.device).synchronize()
        return out

    __call__ = forward

    # ------------------------------------------------- nn.Module-like surface
    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise RuntimeError("QuantizedConvNet is inference-only")
        return self

    def to(self, device):
        # compute stays on the GPU; "cpu" only switches the I/O to host tensors,
        # and moving back to cuda switches it back
        self.host_io = torch.device(device).type == "cpu"
        return self

    def cpu(self):
        """The reference evaluator calls model.cpu() and feeds CPU tensors
        (utils/model_evaluator.py:20,30-31): keep compute on the GPU and accept /
        return host tensors."""
        self.host_io = True
        return self

    def cuda(self, device=None):
        self.host_io = False
        return self

    def state_dict(self):
        return {k: v for k, v in self.spec.items()}

    def model_size_bytes(self):
        total = 0
        for name in [f"conv{i}" for i in range(1, 7)] + ["fc1", "fc2"]:
            e = self.spec[name]
            total += np.asarray(e["w"]).nbytes + np.asarray(e["b"]).nbytes
        return total
