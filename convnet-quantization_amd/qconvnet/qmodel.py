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
        self._w4_ok = {}         # batch size -> whether the conv3 .. conv6 launch ran
        self._convs_ok = {}      # batch size -> whether the one-launch convs ran
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

    # --------------------------------------------------------------- forward
    KERNELS = ("conv1", "conv2", "conv3", "conv4", "conv5", "conv6", "fc1", "fc2")
    KERNELS_FUSED = ("conv12", "conv3", "conv4", "conv5", "conv6", "fc1", "fc2")

    def kernel_names(self, x_shape, keep=False):
        """Names of the launches run() marks, in order (conv1+conv2 are one
        launch when fused, conv3+conv4 / conv5+conv6 one launch each when
        paired, fc1+fc2 one "fc12" slot for the fused head)."""
        if self._w4(x_shape, keep):
            return ("conv12", "conv3_6", "fc12") if self._head(x_shape[0], keep) else ("conv12", "conv3_6", "fc1", "fc2")
        if self._convs(x_shape, keep) and self._convs_form(x_shape[0], keep):
            return ("conv1_6", "fc12") if self._head(x_shape[0], keep) else ("conv1_6", "fc1", "fc2")
        names = list(self.KERNELS_FUSED if self._fused(x_shape) else self.KERNELS)
        if self._pairs(keep):
            names[names.index("conv3"):names.index("conv6") + 1] = ["conv34", "conv56"]
        if self._head(x_shape[0], keep):
            names = names[:-2] + ["fc12"]
        return tuple(names)

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

    def _convs_form(self, n, keep=False):
        """Whether the library takes the one-launch convs at batch n: what a
        run() recorded, else the library's host query (no launch), so
        kernel_names() is right before the first forward at a batch size."""
        ok = self._convs_ok.get(n)
        if ok is None:
            if self._conv_layers is None:
                self._conv_layers = ops.conv_layers(self.L, self.in_zp)
            with torch.cuda.device(self.device):
                ok = ops.convnet_convs_form(n, self.in_scale, self.in_zp, self._conv_layers,
                                            kmajor=self._head(n, keep)) > 0
        return ok

    def _w4(self, x_shape, keep):
        """conv12 + the one-wave-per-SIMD conv3 .. conv6 launch applies: from 4
        images per CU (below that its 4-image conv5+6 tiles are mostly empty),
        unless the library declined this batch size before."""
        n = x_shape[0]
        if not (self.convs_w4 and self._fused(x_shape) and self._pairs(keep) and self._w4_ok.get(n, True)):
            return False
        ncu = torch.cuda.get_device_properties(self.device).multi_processor_count
        return n >= 4 * ncu

    def _convs(self, x_shape, keep):
        """The one-launch conv1 .. conv6 applies to this forward (the library
        may still decline the batch size: _convs_ok records that per size)."""
        return self.fuse_convs and self._fused(x_shape) and self._pairs(keep)

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
        n = x.shape[0]
        b = self._buffers(n, slot)
        L = self.L

        def mark():
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append(ev)

        mark()
        d = L[0]
        names = ["a2", "a3", "a4", "a5", "a6"]
        u8 = x.dtype == torch.uint8

        def conv12():
            if u8:
                ops.conv12_fused_u8(x, self.qlut, self.in_zp, L[0], L[1], out=b["a2"])
            else:
                ops.conv12_fused(x, self.in_scale, self.in_zp, L[0], L[1], out=b["a2"])

        head = self._head(n, keep)
        convs_done = conv12_done = False
        if self._w4(x.shape, keep):
            if self._conv_layers is None:
                self._conv_layers = ops.conv_layers(L, self.in_zp)
            conv12()
            mark()
            if head and "a6k" not in b:
                b["a6k"] = torch.empty((128, n, 32), dtype=torch.uint8, device=self.device)
            out6 = b["a6k"] if head else b["a6"]
            w4_done = ops.convs36(b["a2"], self._conv_layers, b["a4"], out6, kmajor=head)
            self._w4_ok[n] = w4_done
            if w4_done:
                mark()
                prev, first, convs_done = b["a6"], 6, True
            else:   # (mixed epilogue forms) the pair launches from a2
                prev, first, conv12_done = b["a2"], 2, True
        elif self._convs(x.shape, keep) and self._convs_ok.get(n, True):
            if head and "a6k" not in b:
                b["a6k"] = torch.empty((128, n, 32), dtype=torch.uint8, device=self.device)
            if self._conv_layers is None:
                self._conv_layers = ops.conv_layers(L, self.in_zp)
            out6 = b["a6k"] if head else b["a6"]
            if u8:
                convs_done = ops.convnet_convs_u8(x, self.qlut, self.in_zp, self._conv_layers, b["a2"],
                                                  b["a4"], out6, kmajor=head)
            else:
                convs_done = ops.convnet_convs(x, self.in_scale, self.in_zp, self._conv_layers, b["a2"],
                                               b["a4"], out6, kmajor=head)
            self._convs_ok[n] = convs_done
            if convs_done:
                mark()
                prev, first = b["a6"], 6
        if convs_done or conv12_done:
            pass
        elif self._fused(x.shape):
            conv12()
            mark()
            prev, first = b["a2"], 2
        else:
            if u8:   # the stand-alone conv1 has no u8 stage: normalise first
                if "xf" not in b:
                    b["xf"] = torch.empty((n, 3, 32, 32), dtype=torch.float32, device=self.device)
                x = ops.normalize_u8(x, self.ntab, out=b["xf"])
            ops.conv1_f32(x, self.in_scale, self.in_zp, d.w, d.u, d.v, d.mult, d.corr, d.z_y,
                          d.relu, d.qdq, out=b["a1"])
            mark()
            prev, first = b["a1"], 1
        pairs = self._pairs(keep)
        for i in range(first, 6):
            d = L[i]
            if pairs and i in (2, 4):   # conv3+conv4, conv5+conv6 in one launch each
                nb = L[i + 1]
                if i == 4 and head:
                    if "a6k" not in b:
                        b["a6k"] = torch.empty((128, n, 32), dtype=torch.uint8, device=self.device)
                    out, km = b["a6k"], True
                else:
                    out, km = b[names[i]], False
                if not ops.conv_pair(prev, d, nb, out, kmajor=km):
                    raise RuntimeError("fused conv pair rejected a supported shape")
                mark()
                prev = out
                continue
            if pairs and i in (3, 5):
                continue
            if i == 5 and head:   # conv6 writes the classifier's chunk-major input
                if "a6k" not in b:
                    b["a6k"] = torch.empty((128, n, 32), dtype=torch.uint8, device=self.device)
                if not ops.conv3x3_kmajor(prev, d.z_x, d.w, d.cout, d.u, d.v, d.mult, d.corr,
                                          d.z_y, d.relu, d.pool, b["a6k"]):
                    raise RuntimeError("chunk-major conv6 rejected a supported shape")
                mark()
                continue
            ops.conv3x3(prev, d.z_x, d.w, d.cout, d.u, d.v, d.mult, d.corr, d.z_y, d.relu, d.pool,
                        d.qdq, out=b[names[i - 1]])
            mark()
            prev = b[names[i - 1]]
        f1, f2 = self.fc1, self.fc2
        if head:
            if not self._classifier(b["a6k"], b):
                raise RuntimeError("classifier head rejected a supported shape")
            if keep:  # NHWC view of conv6's output for inspection / parity tests
                b["a6"].copy_(ops.from_kmajor(b["a6k"]).view(n, 4, 4, 256))
        elif self.mode == "static":
            flat = prev.view(n, 4096)
            ops.linear_u8(flat, f1.z_x, f1.w, f1.u, f1.v, f1.mult, f1.corr, f1.z_y, True,
                          out=b["f1"])
            mark()
            ops.linear_u8(b["f1"], f2.z_x, f2.w, f2.u, f2.v, f2.mult, f2.corr, f2.z_y, False,
                          y_scale=f2.s_y, want_fp32=True, out=b["q"], out_f=b["logits"])
        else:
            flat = prev.view(n, 4096)
            ops.linear_u8(flat, f1.z_x, f1.w, f1.u, f1.v, f1.mult, f1.corr, f1.z_y, False,
                          y_scale=f1.s_y, want_fp32=True, out=b["f1"], out_f=b["f1f"])
            mark()
            ops.linear_f32(b["f1f"], f2.w, f2.b, relu_in=True, out=b["logits"])
        mark()
        if keep:
            return b["logits"], b
        return b["logits"]

    def _classifier(self, xk, b):
        """fc1+ReLU -> fc2 -> dequantize in two launches (split-K fc1 on the
        chunk-major conv6 output + a per-row finisher); in QDQ mode fc1's
        dequantize, ReLU and the fp32 fc2 run in the finisher."""
        f1, f2 = self.fc1, self.fc2
        n = xk.shape[1]
        if "ws" not in b:
            b["ws"] = ops.classifier_workspace(n, f1.w.shape[0], self.device)
        if self.mode == "qdq":
            return ops.classifier_qdq(xk, f1, f2, b["ws"], b["f1"], b["logits"])
        f1.relu, f2.relu = True, False
        return ops.classifier(xk, f1, f2, b["ws"], b["f1"], b["q"], b["logits"])

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
