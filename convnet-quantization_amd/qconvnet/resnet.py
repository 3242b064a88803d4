"""Static int8 ResNet (bottleneck blocks, per-channel weights) on MI355X —
SURVEY §8(f)2, BASELINE config 5.

Reference: ``CustomQuantizedBottleneck`` / ``CustomQuantizedResNet50``
(models/custom_quantization_model.py:60-148) around torchvision's ResNet-50
(models/dynamic_ptq_model.py:194-195).  Semantics, as for the SimpleConvNet
static path (qmodel.py): BN folded into each conv (custom_quantization_model.py
:264-291 fuses the same Conv-BN(-ReLU) triples), ReLU fused into the requant,
per-channel symmetric s8 weights, u8 per-tensor affine activations with
MinMax ranges observed on calibration data.  The residual join keeps the
reference's float-domain add (:94-101): both operands are dequantized, added
in fp32, ReLU'd and quantized with the block output's qparams.

Device pipeline per forward (all u8 NHWC, every launch a hand-written HIP
kernel on the current stream, capturable into a HIP graph):
  stem_pack (QuantStub + 7-tap row im2col) -> conv 7x1 (the 7x7/2 stem) ->
  maxpool 3x3/2 (one launch, stem_fused, at 224x224 and 64x64; both forms
  read fp32 NCHW or the raw uint8 NHWC images) -> 16 x [conv1x1+ReLU -> conv3x3(/2)+ReLU -> conv1x1
  (-> downsample conv1x1(/2)) -> add+ReLU] -> avgpool (u8, qparams kept) -> fc (fp32 logits)
"""
from __future__ import annotations

import re

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from . import quant as Q
from .data import IMAGENET_MEAN, IMAGENET_STD
from .qmodel import _OBSERVERS, _DevLayer, _weight_scale, cuda_device, normalized_input

F32 = np.float32


# ============================================================ fp32 folding
def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _fold(g, conv, bn):
    return Q.fold_bn(g[conv + ".weight"], g.get(conv + ".bias"), g[bn + ".running_mean"],
                     g[bn + ".running_var"], g[bn + ".weight"], g[bn + ".bias"])


def fold_state_dict(sd):
    """BN-fold a torchvision-layout ResNet state_dict.  Returns
    {"stem": (w, b), "blocks": [{"c1","c2","c3"[, "ds"]: (w, b, stride, pad)}],
     "fc": (w, b)}; strides follow torchvision (first block of layer2..4
    strides its 3x3 conv and its downsample)."""
    g = {k: _np(v) for k, v in sd.items()}
    out = {"stem": _fold(g, "conv1", "bn1"), "blocks": []}
    keys = sorted({(int(m.group(1)), int(m.group(2)))
                   for k in g for m in [re.match(r"layer(\d)\.(\d+)\.conv1\.weight$", k)] if m})
    for li, bi in keys:
        p = f"layer{li}.{bi}."
        s = 2 if (bi == 0 and li > 1) else 1
        blk = {}
        for j, (st, pad) in enumerate(((1, 0), (s, 1), (1, 0)), start=1):
            w, b = _fold(g, p + f"conv{j}", p + f"bn{j}")
            blk[f"c{j}"] = (w, b, st, pad)
        if p + "downsample.0.weight" in g:
            w, b = _fold(g, p + "downsample.0", p + "downsample.1")
            blk["ds"] = (w, b, s, 0)
        out["blocks"].append(blk)
    out["fc"] = (np.asarray(g["fc.weight"], F32), np.asarray(g["fc.bias"], F32))
    return out


# ============================================================ calibration
def calibrate(folded, batches, device="cpu", mean=IMAGENET_MEAN, std=IMAGENET_STD,
              observer="minmax"):
    """fp32 forward of the folded net recording every observer's range
    (batches: normalised fp32 NCHW, or raw uint8 NHWC images normalised here
    with ``mean`` / ``std``):
    x, stem (post-ReLU), per block c1/c2 (post-ReLU), c3 and ds (pre-add),
    out (post add+ReLU), fc.  On the CPU (the default) the ranges are those
    torch.ao's observers record on the same host (same fp32 ops, same folded
    weights) and do not change from run to run; device="cuda" uses the HIP
    min/max observer behind MIOpen's fp32 convs (faster, not bit-stable).

    observer="histogram": torch.ao's default HistogramObserver (2048 bins,
    reduce_range=False) at the same points; the range is its searched
    clipping range, so Q.qparams_affine of it is calculate_qparams().  The
    points are where torch.ao's output observers of the fused ConvReLU2d /
    Conv2d modules and the stubs sit (stem, c1, c2 after their ReLU; c3, ds,
    fc raw; out after add + ReLU), so no observation point moves.  On
    device="cuda" the histogram is ops.HistogramObserver (qcn_histc_f32)."""
    if observer not in _OBSERVERS:
        raise ValueError(f"unknown observer {observer!r} (expected one of {sorted(_OBSERVERS)})")
    make = _OBSERVERS[observer]
    dev = torch.device(device)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    stem = [t(a) for a in folded["stem"]]
    blocks = [{k: (t(v[0]), t(v[1]), v[2], v[3]) for k, v in b.items()} for b in folded["blocks"]]
    fc = [t(a) for a in folded["fc"]]
    rng = {"x": make(dev), "stem": make(dev), "fc": make(dev)}
    ntab = Q.normalize_table(mean, std).to(dev)
    for i, b in enumerate(blocks):
        for k in list(b) + ["out"]:
            rng[f"b{i}.{k}"] = make(dev)
    with torch.no_grad():
        for xb in batches:
            x = normalized_input(xb, dev, ntab)
            rng["x"](x)
            x = F.relu(F.conv2d(x, stem[0], stem[1], stride=2, padding=3))
            rng["stem"](x)
            x = F.max_pool2d(x, 3, 2, 1)
            for i, b in enumerate(blocks):
                def cv(inp, k):
                    w, bb, s, p = b[k]
                    return F.conv2d(inp, w, bb, stride=s, padding=p)
                y = F.relu(cv(x, "c1"))
                rng[f"b{i}.c1"](y)
                y = F.relu(cv(y, "c2"))
                rng[f"b{i}.c2"](y)
                y = cv(y, "c3")
                rng[f"b{i}.c3"](y)
                idn = x
                if "ds" in b:
                    idn = cv(x, "ds")
                    rng[f"b{i}.ds"](idn)
                x = F.relu(y + idn)
                rng[f"b{i}.out"](x)
            x = x.mean((2, 3))   # (the int8 net pools the quantized map, qparams kept)
            x = F.linear(x, fc[0], fc[1])
            rng["fc"](x)
    return {k: r.values() for k, r in rng.items()}


# ============================================================ quantized spec
def build_spec(folded, ranges, per_channel=True):
    """Host description of the int8 net (numpy), the format
    oracle.qref.resnet_int8_forward reads."""
    def layer(wb, s_x, z_x, name, relu):
        w, b, st, pad = wb
        s_w = _weight_scale(w, per_channel)
        s_y, z_y = Q.qparams_affine(*ranges[name])
        return dict(w=Q.quantize_weight(w, s_w), b=np.asarray(b, F32), s_w=s_w, s_x=s_x, z_x=z_x,
                    s_y=s_y, z_y=z_y, relu=relu, stride=(st, st), pad=(pad, pad))

    spec = {"per_channel": bool(per_channel), "blocks": []}
    s_x, z_x = Q.qparams_affine(*ranges["x"])
    spec["in"] = (s_x, z_x)
    w, b = folded["stem"]
    spec["stem"] = layer((w, b, 2, 3), s_x, z_x, "stem", True)
    s_x, z_x = spec["stem"]["s_y"], spec["stem"]["z_y"]
    for i, blk in enumerate(folded["blocks"]):
        e = {"c1": layer(blk["c1"], s_x, z_x, f"b{i}.c1", True)}
        e["c2"] = layer(blk["c2"], e["c1"]["s_y"], e["c1"]["z_y"], f"b{i}.c2", True)
        e["c3"] = layer(blk["c3"], e["c2"]["s_y"], e["c2"]["z_y"], f"b{i}.c3", False)
        e["ds"] = layer(blk["ds"], s_x, z_x, f"b{i}.ds", False) if "ds" in blk else None
        e["out"] = Q.qparams_affine(*ranges[f"b{i}.out"])
        spec["blocks"].append(e)
        s_x, z_x = e["out"]
    # avgpool runs on the quantized map and keeps its qparams (torch.ao's
    # quantized adaptive_avg_pool2d), so the fc's input qparams are the last
    # block's output qparams
    w, b = folded["fc"]
    s_w = _weight_scale(w, per_channel)
    s_y, z_y = Q.qparams_affine(*ranges["fc"])
    spec["fc"] = dict(w=Q.quantize_weight(w, s_w), b=np.asarray(b, F32), s_w=s_w,
                      s_x=s_x, z_x=z_x, s_y=s_y, z_y=z_y, relu=False)
    return spec


def quantize_resnet(model, calib_batches, device="cuda", per_channel=True, calibration_device="cpu",
                    mean=IMAGENET_MEAN, std=IMAGENET_STD, observer="minmax"):
    """fp32 ResNet (models.resnet / torchvision layout) -> QuantizedResNet on
    `device`; calibration runs on `calibration_device` (CPU: deterministic).
    ``mean`` / ``std`` normalise raw uint8 images (calibration and inference);
    ``observer``: "minmax" or "histogram" (calibrate)."""
    folded = fold_state_dict(model.state_dict())
    ranges = calibrate(folded, calib_batches, calibration_device, mean, std, observer)
    return QuantizedResNet(build_spec(folded, ranges, per_channel), device, mean, std)


# ============================================================ device model
class QuantizedResNet:
    """Duck-typed int8 ResNet (eval / cpu / to / __call__ like the reference's
    models.*): fp32 [N,3,H,W] in, fp32 [N,num_classes] logits out.  Raw uint8
    NHWC images [N,H,W,3] go to the stem as they are: ToTensor -> Normalize
    (``mean`` / ``std``) -> QuantStub is the 3 x 256 byte table ``qlut`` the
    stem kernels look the image bytes up in."""

    def __init__(self, spec, device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.spec = spec
        self.device = cuda_device(device)
        self.ntab = Q.normalize_table(mean, std).to(self.device)
        self.quantized = True
        self.host_io = False
        self._graphs = {}
        # the layer-1 expand + join launches also run the next block's reduce
        # conv (qcn_conv1x1_join_reduce_u8s8_nhwc); False: separate launches
        self.fuse_reduce = True
        self._upload()

    def _t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _layer(self, e, stem=False):
        d = _DevLayer()
        w = np.asarray(e["w"], np.int8)
        if stem:
            w = ops.stem_weight_rows(w)
            d.sy, d.sx, d.py, d.px = e["stride"][0], 1, e["pad"][0], 0
        else:
            (d.sy, d.sx), (d.py, d.px) = e["stride"], e["pad"]
        packed, wsum = ops.pack_conv_kmajor(w)
        d.cout, _, d.kh, d.kw = w.shape
        u, v, mult = Q.epilogue_constants(e["s_x"], e["s_w"], e["s_y"], e["b"])
        d.w = self._t(packed)
        d.u, d.v, d.mult = self._t(u), self._t(v), self._t(mult)
        d.corr = self._t(((128 - int(e["z_x"])) * wsum.astype(np.int64)).astype(np.int32))
        d.z_x, d.z_y, d.s_y, d.relu = int(e["z_x"]), int(e["z_y"]), F32(e["s_y"]), e["relu"]
        d.cin = w.shape[1]
        d.w64 = None
        if (d.kh, d.kw, d.sy, d.sx, d.py, d.px) == (3, 3, 1, 1, 1, 1) and w.shape[1] % 64 == 0:
            # the patch-staged 3x3 kernel's layout ([tap * cin/64 + cb][cout][64])
            d.w64 = self._t(ops.pack_conv3x3(w)[0])
        return d

    # 3x3 stride-1 convs (hw, cin, cout) that run on the patch-staged ring
    # kernel (qcn_conv3x3_u8s8_nhwc): the input band is staged once in LDS and
    # read by all nine taps, instead of a gathered im2col row per tap
    HALO_SHAPES = {(56, 64, 64), (28, 128, 128)}

    def _conv3x3_halo(self, y, d):
        n, h, w, cin = y.shape
        if d.w64 is None or h != w or (h, cin, d.cout) not in self.HALO_SHAPES:
            return None
        return ops.conv3x3(y, d.z_x, d.w64, d.cout, d.u, d.v, d.mult, d.corr, d.z_y, d.relu, False)

    def _upload(self):
        sp = self.spec
        self.in_scale, self.in_zp = sp["in"]
        # ToTensor -> Normalize -> QuantStub per (channel, byte)
        self.qlut = Q.quantize_table(self.ntab.cpu(), self.in_scale, self.in_zp).to(self.device)
        self.stem = self._layer(sp["stem"], stem=True)
        self.blocks = []
        for e in sp["blocks"]:
            self.blocks.append({k: (self._layer(e[k]) if e.get(k) is not None else None)
                                for k in ("c1", "c2", "c3", "ds")})
        fc = sp["fc"]
        d = _DevLayer()
        w = np.asarray(fc["w"], np.int8)
        u, v, mult = Q.epilogue_constants(fc["s_x"], fc["s_w"], fc["s_y"], fc["b"])
        d.w = self._t(w)
        d.u, d.v, d.mult = self._t(u), self._t(v), self._t(mult)
        d.corr = self._t(((128 - int(fc["z_x"])) * w.astype(np.int64).sum(1)).astype(np.int32))
        d.z_x, d.z_y, d.s_y = int(fc["z_x"]), int(fc["z_y"]), F32(fc["s_y"])
        self.fc = d
        self.num_classes = w.shape[0]

    def _stem_fusable(self, x):
        """The one-launch stem (qcn_resnet_stem_fused) covers torchvision's
        7x7/2 pad-3 64-channel stem at 224x224 and 64x64 inputs (fp32 NCHW or
        u8 NHWC)."""
        e = self.spec["stem"]
        c, h, w = (x.shape[3], x.shape[1], x.shape[2]) if x.dtype == torch.uint8 else x.shape[1:]
        return (self.stem.cout == 64
                and tuple(np.asarray(e["w"]).shape[1:]) == (3, 7, 7)
                and tuple(e["stride"]) == (2, 2) and tuple(e["pad"]) == (3, 3)
                and c == 3 and h == w and h in (224, 64))

    def _input(self, x):
        """What the stem launches read, on the model's device: fp32 NCHW, or a
        raw u8 NHWC batch as it is — contiguous and on a 4-byte boundary (the
        fused stem loads its rows as dwords)."""
        if x.dtype != torch.uint8:
            return x.to(self.device, torch.float32)
        Q.check_u8_images(x)
        x = x.to(self.device).contiguous()
        return x.clone() if x.data_ptr() % 4 else x

    @staticmethod
    def _join_reduce_fusable(c3, c1n):
        """c3 (+ join) and the next block's c1 in one launch: the 64 -> 256 1x1
        expand and a 1x1 stride-1 256 -> 64 / 128 reduce (ResNet-50 layer 1 and
        the first reduce of layer 2)."""
        one = lambda d: (d.kh, d.kw, d.sy, d.sx, d.py, d.px) == (1, 1, 1, 1, 0, 0)
        return (one(c3) and one(c1n) and c3.cin == 64 and c3.cout == 256 and c1n.cin == 256
                and c1n.cout in (64, 128) and not c3.relu)

    def conv_layers(self):
        """Every conv launch in forward order (for MAC accounting)."""
        out = [self.stem]
        for b in self.blocks:
            out += ([b["ds"]] if b["ds"] is not None else []) + [b["c1"], b["c2"], b["c3"]]
        return out

    def run(self, x, keep=False, marks=None):
        """The whole int8 forward on the current stream of the model's device
        (no sync).  keep=True also returns the block outputs; keep="layers" is
        the inspection mode of the error report: the three-launch stem, every
        conv its own launch, conv3 without the join and then ops.add_relu —
        the same bits, with "stem.conv" (pre-pool), "block{i}.c1" / ".c2" /
        ".c3" (pre-add) / ".ds" and the u8 logits "fc.q" kept as well."""
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        with torch.cuda.device(self.device):
            return self._run(self._input(x), keep, marks)

    def _run(self, x, keep, marks):
        g = self._steps(x, keep, marks)
        while True:
            try:
                next(g)
            except StopIteration as e:
                return e.value

    def run_streams(self, x, nsplit=2):
        """The forward over `nsplit` slices of the batch, each on its own HIP
        stream, launches interleaved layer by layer: one slice's layer tail
        (its last, partly filled round of workgroups) runs beside the other
        slice's layer instead of leaving CUs idle.  Ordered after the current
        stream's prior work; the current stream waits for the result."""
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        with torch.cuda.device(self.device):
            x = self._input(x)
            main = torch.cuda.current_stream(self.device)
            if len(getattr(self, "_side", ())) < nsplit:
                self._side = [torch.cuda.Stream(device=self.device) for _ in range(nsplit)]
            streams = self._side[:nsplit]
            for s in streams:
                s.wait_stream(main)
            chunks = x.chunk(nsplit)
            # (u8: H * W * 3 bytes per image is a multiple of 4 at both fused sizes)
            assert not (x.dtype == torch.uint8 and self._stem_fusable(x)) or all(
                c.data_ptr() % 4 == 0 for c in chunks), "u8 slices off the 4-byte boundary"
            gens = [self._steps(c, False, None) for c in chunks]
            outs = [None] * len(gens)
            live = list(range(len(gens)))
            while live:
                for i in list(live):
                    with torch.cuda.stream(streams[i]):
                        try:
                            next(gens[i])
                        except StopIteration as e:
                            outs[i] = e.value
                            live.remove(i)
            for s in streams:
                main.wait_stream(s)
            for o, s in zip(outs, streams):
                o.record_stream(main)   # allocated on a side stream, read on main
            return torch.cat(outs)

    def _steps(self, x, keep, marks):
        """The forward as a generator: one yield after each launch."""
        inter = {}

        def mark(name):
            if marks is not None:
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append((name, ev))

        sp = self.spec
        mark("start")
        u8 = x.dtype == torch.uint8   # raw images: the QuantStub is a lookup in qlut
        layers = isinstance(keep, str) and keep == "layers"
        if keep not in (False, True) and not layers:
            raise ValueError(f"unknown keep {keep!r}")
        if self._stem_fusable(x) and not layers:   # quantize + conv + ReLU + max-pool in one launch
            if u8:
                q = ops.stem_fused_u8(x, self.qlut, self.in_zp, self.stem)
            else:
                q = ops.stem_fused(x, self.in_scale, self.in_zp, self.stem)
            mark("conv")   # carries the stem MACs (bench / resnet_layers accounting)
            yield
        else:
            if u8:
                q = ops.stem_pack_u8(x, self.qlut, self.in_zp)
            else:
                q = ops.stem_pack(x, self.in_scale, self.in_zp)
            mark("stem_pack")
            yield
            q = ops.conv(q, self.in_zp, self.stem)
            mark("conv")
            yield
            if layers:
                inter["stem.conv"] = q
            q = ops.maxpool3x3s2(q)
            mark("maxpool")
            yield
        if keep:
            inter["stem"] = q
        pending = None   # this block's c1 output, when the previous launch fused it
        for i, (b, e) in enumerate(zip(self.blocks, sp["blocks"])):
            zx = b["c1"].z_x
            if b["ds"] is not None:   # identity first, so conv3 can consume it
                idn = ops.conv(q, zx, b["ds"])
                mark("conv")
                yield
                si, zi = e["ds"]["s_y"], e["ds"]["z_y"]
            else:
                idn, si, zi = q, e["c1"]["s_x"], zx
            if pending is not None:
                y, pending = pending, None
            else:
                y = ops.conv(q, zx, b["c1"])
                mark("conv")
                yield
            y1 = y
            yh = self._conv3x3_halo(y, b["c2"])
            y = yh if yh is not None else ops.conv(y, b["c2"].z_x, b["c2"])
            mark("conv")
            yield
            so, zo = e["out"]
            # conv3 + residual join in one launch, with the next block's reduce
            # conv where the shapes allow (its input is this join's output)
            nb = self.blocks[i + 1] if i + 1 < len(self.blocks) else None
            fused = None
            if (not layers and self.fuse_reduce and nb is not None
                    and self._join_reduce_fusable(b["c3"], nb["c1"])):
                assert nb["c1"].z_x == int(zo), "the next reduce reads this join's output"
                fused = ops.conv_join_reduce(y, b["c3"].z_x, b["c3"], (idn, si, zi, so, zo), nb["c1"])
            if fused is not None:
                q, pending = fused
            elif layers:
                y3 = ops.conv(y, b["c3"].z_x, b["c3"])
                mark("conv")
                yield
                q = ops.add_relu(y3, e["c3"]["s_y"], e["c3"]["z_y"], idn, si, zi, so, zo)
                inter.update({f"block{i}.c1": y1, f"block{i}.c2": y, f"block{i}.c3": y3})
                if b["ds"] is not None:
                    inter[f"block{i}.ds"] = idn
            else:
                q = ops.conv(y, b["c3"].z_x, b["c3"], resid=(idn, si, zi, so, zo))
            mark("add_relu" if layers else "conv")
            yield
            if keep:
                inter[f"block{i}"] = q
        last = sp["blocks"][-1]["out"] if sp["blocks"] else (sp["stem"]["s_y"], sp["stem"]["z_y"])
        q = ops.avgpool(q, last[1])   # qparams kept: the fc reads `last`'s qparams
        mark("avgpool")
        yield
        if keep:
            inter["pool"] = q
        f = self.fc
        qy, logits = ops.linear_u8(q, f.z_x, f.w, f.u, f.v, f.mult, f.corr, f.z_y, False,
                                   y_scale=f.s_y, want_fp32=True)
        mark("fc")
        if layers:
            inter["fc.q"] = qy
        return (logits, inter) if keep else logits

    def capture_graph(self, x_static):
        n = x_static.shape[0]
        s = torch.cuda.Stream(device=self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self.run(x_static)
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
        # (raw uint8 images: the bytes are moved and read by the stem as they are)
        xd = self._input(x).contiguous()
        # two interleaved stream slices fill each layer's last workgroup round
        # (+6 % at batch 512, profiles/r02_diag_resnet_streams.txt)
        out = self.run_streams(xd, 2) if xd.shape[0] >= 128 else self.run(xd).clone()
        if host or self.host_io:
            return out.cpu()
        torch.cuda.current_stream(self.device).synchronize()
        return out

    __call__ = forward

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise RuntimeError("QuantizedResNet is inference-only")
        return self

    def to(self, device):
        self.host_io = torch.device(device).type == "cpu"   # compute stays on the GPU
        return self

    def cpu(self):
        self.host_io = True
        return self

    def cuda(self, device=None):
        self.host_io = False
        return self


# ============================================================ error report
def layer_names(qmodel):
    """The hand-offs layer_pairs scores, in forward order, under the
    observers' names (calibrate)."""
    names = ["x", "stem"]
    for i, b in enumerate(qmodel.blocks):
        names += [f"b{i}.c1", f"b{i}.c2", f"b{i}.c3"]
        names += ([f"b{i}.ds"] if b["ds"] is not None else []) + [f"b{i}.out"]
    return names + ["pool", "fc"]


def layer_pairs(qmodel, folded, images, batch=32):
    """Yield (name, x_fp32, q_u8, scale, zero_point, nhwc) for every hand-off
    of ``qmodel`` (a QuantizedResNet), batch by batch, in layer_names order
    within a batch.  ``folded``: fold_state_dict of the fp32 model it was built
    from; ``images``: fp32 NCHW, or raw uint8 NHWC (normalised with the model's
    mean / std), host or device.

    Per batch, on the model's device and current stream: ``qmodel.run(x,
    keep="layers")`` and the walk of calibrate() through torch ops (fp32 convs
    with a deterministic algorithm), one layer's reference at a time:
      "x":        the input against ops.quantize of it;
      "stem":     post-ReLU against the pre-pool stem conv;
      b{i}.c1/c2: post-ReLU; b{i}.c3 / .ds: raw (pre-add); b{i}.out: after
                  add + ReLU, against the join's output;
      "pool":     mean((2, 3)) against the u8 average pool (the last block's
                  qparams); "fc": the logits against the u8 logits.
    No sync."""
    from .qerror import _conv_deterministic
    if batch < 1:
        raise ValueError("layer_pairs: batch must be positive")
    dev = qmodel.device
    sp = qmodel.spec
    with torch.cuda.device(dev), torch.no_grad():
        def t(a):
            return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        stem = [t(a) for a in folded["stem"]]
        blocks = [{k: (t(v[0]), t(v[1]), v[2], v[3]) for k, v in b.items()} for b in folded["blocks"]]
        fc = [t(a) for a in folded["fc"]]
        for a in range(0, images.shape[0], batch):
            xb = images[a:a + batch].to(dev)
            x = normalized_input(xb, dev, qmodel.ntab).contiguous()
            _, q = qmodel.run(xb.contiguous() if xb.dtype == torch.uint8 else x, keep="layers")
            yield ("x", x, ops.quantize(x, qmodel.in_scale, qmodel.in_zp), qmodel.in_scale,
                   qmodel.in_zp, True)
            x = F.relu(_conv_deterministic(x, stem[0], stem[1], 2, 3))
            yield "stem", x, q["stem.conv"], sp["stem"]["s_y"], sp["stem"]["z_y"], True
            x = F.max_pool2d(x, 3, 2, 1)
            for i, (b, e) in enumerate(zip(blocks, sp["blocks"])):
                def cv(inp, k):
                    w, bb, s, p = b[k]
                    return _conv_deterministic(inp, w, bb, s, p)
                y = F.relu(cv(x, "c1"))
                yield f"b{i}.c1", y, q[f"block{i}.c1"], e["c1"]["s_y"], e["c1"]["z_y"], True
                y = F.relu(cv(y, "c2"))
                yield f"b{i}.c2", y, q[f"block{i}.c2"], e["c2"]["s_y"], e["c2"]["z_y"], True
                y = cv(y, "c3")
                yield f"b{i}.c3", y, q[f"block{i}.c3"], e["c3"]["s_y"], e["c3"]["z_y"], True
                idn = x
                if "ds" in b:
                    idn = cv(x, "ds")
                    yield f"b{i}.ds", idn, q[f"block{i}.ds"], e["ds"]["s_y"], e["ds"]["z_y"], True
                x = F.relu(y + idn)
                del y, idn
                yield f"b{i}.out", x, q[f"block{i}"], e["out"][0], e["out"][1], True
            last = sp["blocks"][-1]["out"] if sp["blocks"] else (sp["stem"]["s_y"], sp["stem"]["z_y"])
            x = x.mean((2, 3))
            yield "pool", x, q["pool"], last[0], last[1], True
            x = F.linear(x, fc[0], fc[1])
            yield "fc", x, q["fc.q"], sp["fc"]["s_y"], sp["fc"]["z_y"], True


def layer_report(qmodel, folded, images, batch=32):
    """{name: QuantErrorStats.result()} in layer_names order for ``images``
    run through ``qmodel`` and its fp32 original (layer_pairs); one stats
    object per name, one synchronisation, at the end."""
    from .qerror import score_pairs
    return score_pairs(layer_pairs(qmodel, folded, images, batch), qmodel.device)
