"""ResNet bottleneck network in the reference's own semantics — SURVEY §8(f)2,
BASELINE config 5, ``CustomQuantizedResNet50(mode="reference")``.

Reference: ``CustomQuantizedBottleneck`` / ``CustomQuantizedResNet50``
(/root/reference/models/custom_quantization_model.py:34-45, 60-143).  Every
conv (stem, conv1-3, downsample) and the fc is wrapped QuantStub -> op ->
DeQuantStub; BN, ReLU, the stem's max-pool, the float-domain residual add
(:95-101) and the average pool run in fp32 BETWEEN the int8 ops.  Nothing is
folded.  As shipped the reference never converts those stubs (its model
stays fp32); here they are live, as torch.ao eager prepare/convert makes them:
each stub's MinMax observer sees the fp32 network's activations during
calibration, each int8 conv requantizes to its own output observer's qparams
(no ReLU in the int8 op), per-channel symmetric s8 weights.  The outer
QuantStub / DeQuantStub pair (:107-108) stays an identity — converted, it
would feed conv1's own QuantStub a quantized tensor, which torch rejects.
The oracle is ``oracle.qref.resnet_qdq_forward``, pinned to torch.ao by
tests/golden/net_resnet_qdq.npz (oracle/make_golden.py gen_resnet_qdq_net).

Device pipeline per forward (every launch a hand-written HIP kernel):
  stem_pack (stem QuantStub + 7-tap rows) -> conv 7x1 -> dq_bn_relu_maxpool
  (fp32 block input + its u8 quantize) -> per block [conv1 -> dq_bn_q ->
  conv2 -> dq_bn_q -> conv3 (, downsample conv) -> qdq_join (fp32 block
  output + next block's u8 input)] -> avgpool_f32 -> fc QuantStub -> int8 fc
  -> DeQuantStub.  Activations between blocks are fp32 NHWC (the identity
  path of the next block reads them), every conv input is u8 NHWC.
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


def _np(v):
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def unfolded_state(sd):
    """torchvision-layout ResNet state_dict -> {"stem": conv, "blocks": [{c1, c2,
    c3[, ds]}], "fc": (w, b)}, conv = (w, stride, pad, bn), bn = (mean, var,
    gamma, beta, eps) — nothing folded (the reference keeps BN in fp32)."""
    g = {k: _np(v) for k, v in sd.items()}

    def bn(p):
        return (g[p + ".running_mean"], g[p + ".running_var"], g[p + ".weight"], g[p + ".bias"], 1e-5)

    out = {"stem": (np.asarray(g["conv1.weight"], F32), 2, 3, bn("bn1")), "blocks": []}
    keys = sorted({(int(m.group(1)), int(m.group(2)))
                   for k in g for m in [re.match(r"layer(\d)\.(\d+)\.conv1\.weight$", k)] if m})
    for li, bi in keys:
        p = f"layer{li}.{bi}."
        s = 2 if (bi == 0 and li > 1) else 1
        blk = {}
        for j, (st, pad) in enumerate(((1, 0), (s, 1), (1, 0)), start=1):
            blk[f"c{j}"] = (np.asarray(g[p + f"conv{j}.weight"], F32), st, pad, bn(p + f"bn{j}"))
        if p + "downsample.0.weight" in g:
            blk["ds"] = (np.asarray(g[p + "downsample.0.weight"], F32), s, 0, bn(p + "downsample.1"))
        out["blocks"].append(blk)
    out["fc"] = (np.asarray(g["fc.weight"], F32), np.asarray(g["fc.bias"], F32))
    return out


def calibrate(net, batches, device="cpu", mean=IMAGENET_MEAN, std=IMAGENET_STD,
              observer="minmax"):
    """The observers of the live-stub model: fp32 forward of the unfolded net
    (torch's own conv / batch_norm / pooling ops, as torch.ao's prepared model
    runs during calibration) recording, per int8 op, its QuantStub's input
    range ("<name>.in") and its output range ("<name>.out").  Batches:
    normalised fp32 NCHW, or raw uint8 NHWC images normalised here with
    ``mean`` / ``std``.  observer="histogram": torch.ao's default
    HistogramObserver (reduce_range=False) at the same points, the range its
    searched clipping range (qmodel.calibrate); on device="cuda" it is
    ops.HistogramObserver (qcn_histc_f32)."""
    if observer not in _OBSERVERS:
        raise ValueError(f"unknown observer {observer!r} (expected one of {sorted(_OBSERVERS)})")
    make = _OBSERVERS[observer]
    dev = torch.device(device)
    ntab = Q.normalize_table(mean, std).to(dev)

    def t(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    rng = {}

    def obs(key, x):
        if key not in rng:
            rng[key] = make(dev)
        rng[key](x)

    def qconv(name, x, layer):
        w, st, pad, (m, v, g, b, eps) = layer
        obs(name + ".in", x)
        y = F.conv2d(x, t(w), None, stride=st, padding=pad)
        obs(name + ".out", y)
        return F.batch_norm(y, t(m), t(v), t(g), t(b), False, 0.0, eps)

    with torch.no_grad():
        for xb in batches:
            x = normalized_input(xb, dev, ntab)
            x = F.max_pool2d(F.relu(qconv("stem", x, net["stem"])), 3, 2, 1)
            for i, blk in enumerate(net["blocks"]):
                out = F.relu(qconv(f"b{i}.c1", x, blk["c1"]))
                out = F.relu(qconv(f"b{i}.c2", out, blk["c2"]))
                out = qconv(f"b{i}.c3", out, blk["c3"])
                idn = qconv(f"b{i}.ds", x, blk["ds"]) if "ds" in blk else x
                x = F.relu(out + idn)
            x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
            obs("fc.in", x)
            obs("fc.out", F.linear(x, t(net["fc"][0]), t(net["fc"][1])))
    return {k: r.values() for k, r in rng.items()}


def build_spec(net, ranges, per_channel=True):
    """Host description of the live-stub int8 net (numpy) — the format
    oracle.qref.resnet_qdq_forward reads."""
    def conv(name, layer):
        w, st, pad, (m, v, g, b, eps) = layer
        s_w = _weight_scale(w, per_channel)
        s_x, z_x = Q.qparams_affine(*ranges[name + ".in"])
        s_y, z_y = Q.qparams_affine(*ranges[name + ".out"])
        return dict(w=Q.quantize_weight(w, s_w), b=np.zeros(w.shape[0], F32), s_w=s_w, s_x=s_x,
                    z_x=z_x, s_y=s_y, z_y=z_y, stride=(st, st), pad=(pad, pad),
                    bn=Q.bn_eval_affine(m, v, g, b, eps))

    spec = {"per_channel": bool(per_channel), "stem": conv("stem", net["stem"]), "blocks": []}
    for i, blk in enumerate(net["blocks"]):
        e = {k: conv(f"b{i}.{k}", blk[k]) for k in ("c1", "c2", "c3")}
        e["ds"] = conv(f"b{i}.ds", blk["ds"]) if "ds" in blk else None
        spec["blocks"].append(e)
    w, b = net["fc"]
    s_w = _weight_scale(w, per_channel)
    s_x, z_x = Q.qparams_affine(*ranges["fc.in"])
    s_y, z_y = Q.qparams_affine(*ranges["fc.out"])
    spec["fc"] = dict(w=Q.quantize_weight(w, s_w), b=np.asarray(b, F32), s_w=s_w, s_x=s_x, z_x=z_x,
                      s_y=s_y, z_y=z_y)
    return spec


def quantize_resnet_reference(model, calib_batches, device="cuda", per_channel=True,
                              calibration_device="cpu", mean=IMAGENET_MEAN, std=IMAGENET_STD,
                              observer="minmax"):
    """fp32 ResNet (torchvision layout) -> QuantizedResNetQDQ on `device`.
    ``mean`` / ``std`` normalise raw uint8 images (calibration and inference);
    ``observer``: "minmax" or "histogram" (calibrate)."""
    net = unfolded_state(model.state_dict())
    ranges = calibrate(net, calib_batches, calibration_device, mean, std, observer)
    return QuantizedResNetQDQ(build_spec(net, ranges, per_channel), device, mean, std)


class QuantizedResNetQDQ:
    """Duck-typed live-stub int8 ResNet (eval / cpu / to / __call__): fp32
    [N,3,H,W] in, fp32 [N,num_classes] logits out.  Raw uint8 NHWC images
    [N,H,W,3] go to the stem's row pack as they are: ToTensor -> Normalize
    (``mean`` / ``std``) -> the stem's QuantStub is the 3 x 256 byte table
    ``qlut``."""

    def __init__(self, spec, device="cuda", mean=IMAGENET_MEAN, std=IMAGENET_STD):
        self.spec = spec
        self.device = cuda_device(device)
        self.ntab = Q.normalize_table(mean, std).to(self.device)
        self.quantized = True
        self.host_io = False
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
        d.z_x, d.s_x, d.z_y, d.s_y, d.relu = int(e["z_x"]), F32(e["s_x"]), int(e["z_y"]), F32(e["s_y"]), False
        d.alpha, d.beta = (self._t(np.asarray(a, F32)) for a in e["bn"])
        return d

    def _upload(self):
        sp = self.spec
        self.stem = self._layer(sp["stem"], stem=True)
        # ToTensor -> Normalize -> the stem's QuantStub per (channel, byte)
        self.qlut = Q.quantize_table(self.ntab.cpu(), self.stem.s_x, self.stem.z_x).to(self.device)
        self.blocks = []
        for e in sp["blocks"]:
            b = {k: (self._layer(e[k]) if e.get(k) is not None else None) for k in ("c1", "c2", "c3", "ds")}
            if b["ds"] is not None and (b["ds"].s_x, b["ds"].z_x) != (b["c1"].s_x, b["c1"].z_x):
                raise ValueError("conv1's and the downsample's QuantStubs observe the same tensor "
                                 "and must agree on their qparams")
            self.blocks.append(b)
        fc = sp["fc"]
        d = _DevLayer()
        w = np.asarray(fc["w"], np.int8)
        u, v, mult = Q.epilogue_constants(fc["s_x"], fc["s_w"], fc["s_y"], fc["b"])
        d.w = self._t(w)
        d.u, d.v, d.mult = self._t(u), self._t(v), self._t(mult)
        d.corr = self._t(((128 - int(fc["z_x"])) * w.astype(np.int64).sum(1)).astype(np.int32))
        d.s_x, d.z_x, d.z_y, d.s_y = F32(fc["s_x"]), int(fc["z_x"]), int(fc["z_y"]), F32(fc["s_y"])
        self.fc = d
        self.num_classes = w.shape[0]

    def _input(self, x):
        """What the stem pack reads, on the model's device: fp32 NCHW, or a raw
        u8 NHWC batch as it is (contiguous; any byte alignment)."""
        if x.dtype != torch.uint8:
            return x.to(self.device, torch.float32)
        Q.check_u8_images(x)
        return x.to(self.device).contiguous()

    def run(self, x, keep=False):
        if x.device != self.device:
            raise ValueError(f"input on {x.device}, model on {self.device}")
        with torch.cuda.device(self.device):
            return self._run(self._input(x), keep)

    def _run(self, x, keep):
        inter = {}
        st = self.stem
        first = self.blocks[0]["c1"] if self.blocks else None
        if x.dtype == torch.uint8:   # raw images: the QuantStub is a lookup in qlut
            rows = ops.stem_pack_u8(x, self.qlut, st.z_x)
        else:
            rows = ops.stem_pack(x, st.s_x, st.z_x)
        y = ops.conv(rows, st.z_x, st)
        xf, xq = ops.dq_bn_relu_maxpool(y, st.s_y, st.z_y, st.alpha, st.beta,
                                        first.s_x if first else None, first.z_x if first else 0)
        if keep:
            inter["stem.q"], inter["stem"] = y, xf
        for i, b in enumerate(self.blocks):
            c1, c2, c3, ds = b["c1"], b["c2"], b["c3"], b["ds"]
            y1 = ops.conv(xq, c1.z_x, c1)
            y2 = ops.conv(ops.dq_bn_q(y1, c1.s_y, c1.z_y, c1.alpha, c1.beta, True, c2.s_x, c2.z_x), c2.z_x, c2)
            y3 = ops.conv(ops.dq_bn_q(y2, c2.s_y, c2.z_y, c2.alpha, c2.beta, True, c3.s_x, c3.z_x), c3.z_x, c3)
            if ds is not None:
                yd = ops.conv(xq, ds.z_x, ds)
                ident = (yd, ds.s_y, ds.z_y, ds.alpha, ds.beta)
            else:
                ident = xf
            nxt = self.blocks[i + 1]["c1"] if i + 1 < len(self.blocks) else None
            xf, xq = ops.qdq_join(y3, c3.s_y, c3.z_y, c3.alpha, c3.beta, ident,
                                  nxt.s_x if nxt else None, nxt.z_x if nxt else 0)
            if keep:
                inter.update({f"block{i}.c1": y1, f"block{i}.c2": y2, f"block{i}.c3": y3, f"block{i}": xf})
                if ds is not None:
                    inter[f"block{i}.ds"] = yd
        p = ops.avgpool_f32(xf)
        f = self.fc
        q = ops.quantize(p.view(p.shape[0], p.shape[1], 1, 1), f.s_x, f.z_x, nhwc=False).view(p.shape)
        qy, logits = ops.linear_u8(q, f.z_x, f.w, f.u, f.v, f.mult, f.corr, f.z_y, False,
                                   y_scale=f.s_y, want_fp32=True)
        if keep:
            inter["pool"], inter["fc.q"] = p, qy
            return logits, inter
        return logits

    @torch.no_grad()
    def forward(self, x):
        host = not x.is_cuda
        xd = self._input(x).contiguous()
        out = self.run(xd).clone()
        if host or self.host_io:
            return out.cpu()
        torch.cuda.current_stream(self.device).synchronize()
        return out

    __call__ = forward

    def eval(self):
        return self

    def train(self, mode=True):
        if mode:
            raise RuntimeError("QuantizedResNetQDQ is inference-only")
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
    """The hand-offs layer_pairs scores, in forward order."""
    names = ["stem", "stem.pool"]
    for i, b in enumerate(qmodel.blocks):
        names += [f"b{i}.c1", f"b{i}.c2", f"b{i}.c3"]
        names += ([f"b{i}.ds"] if b["ds"] is not None else []) + [f"b{i}"]
    return names + ["pool", "fc"]


def layer_pairs(qmodel, net, images, batch=32):
    """Yield (name, x_fp32, y, scale, zero_point, nhwc) for every hand-off of
    ``qmodel`` (a QuantizedResNetQDQ), batch by batch, in layer_names order
    within a batch.  ``net``: unfolded_state of the fp32 model it was built
    from; ``images``: fp32 NCHW, or raw uint8 NHWC (normalised with the model's
    mean / std), host or device.

    Per batch, on the model's device and current stream: ``qmodel.run(x,
    keep=True)`` and the walk of calibrate() through torch ops (fp32 convs with
    a deterministic algorithm), one layer's reference at a time.  ``y`` is u8
    (scored with scale, zero_point) or fp32 NHWC (scale and zero_point None):
      "stem", b{i}.c1|c2|c3|ds: the pre-BN conv output against the int8 conv's
                   u8 output, with its own output qparams;
      "stem.pool": fp32, after BN, ReLU and the max-pool, against the fp32
                   block input; "b{i}": fp32, after the float-domain add and
                   ReLU, against the fp32 block output; "pool": fp32 [N, C];
      "fc":        the logits against the u8 logits.
    No sync."""
    from .qerror import _conv_deterministic
    if batch < 1:
        raise ValueError("layer_pairs: batch must be positive")
    dev = qmodel.device
    sp = qmodel.spec
    with torch.cuda.device(dev), torch.no_grad():
        def t(a):
            return torch.from_numpy(np.ascontiguousarray(a, F32)).to(dev)

        def up(layer):
            w, st, pad, (m, v, g, b, eps) = layer
            return t(w), st, pad, (t(m), t(v), t(g), t(b), eps)

        stem = up(net["stem"])
        blocks = [{k: up(v) for k, v in b.items()} for b in net["blocks"]]
        fc = [t(a) for a in net["fc"]]

        def conv(x, layer):
            return _conv_deterministic(x, layer[0], None, layer[1], layer[2])

        def bn(y, layer):
            m, v, g, b, eps = layer[3]
            return F.batch_norm(y, m, v, g, b, False, 0.0, eps)

        for a in range(0, images.shape[0], batch):
            xb = images[a:a + batch].to(dev)
            x = normalized_input(xb, dev, qmodel.ntab).contiguous()
            _, q = qmodel.run(xb.contiguous() if xb.dtype == torch.uint8 else x, keep=True)
            y = conv(x, stem)
            yield "stem", y, q["stem.q"], sp["stem"]["s_y"], sp["stem"]["z_y"], True
            x = F.max_pool2d(F.relu(bn(y, stem)), 3, 2, 1).contiguous()
            yield "stem.pool", x, q["stem"], None, None, True
            for i, (b, e) in enumerate(zip(blocks, sp["blocks"])):
                y = x
                for k in ("c1", "c2", "c3"):
                    y = conv(y, b[k])
                    yield f"b{i}.{k}", y, q[f"block{i}.{k}"], e[k]["s_y"], e[k]["z_y"], True
                    y = bn(y, b[k])
                    if k != "c3":
                        y = F.relu(y)
                idn = x
                if "ds" in b:
                    idn = conv(x, b["ds"])
                    yield f"b{i}.ds", idn, q[f"block{i}.ds"], e["ds"]["s_y"], e["ds"]["z_y"], True
                    idn = bn(idn, b["ds"])
                x = F.relu(y + idn).contiguous()
                del y, idn
                yield f"b{i}", x, q[f"block{i}"], None, None, True
            x = torch.flatten(F.adaptive_avg_pool2d(x, 1), 1).contiguous()
            yield "pool", x, q["pool"], None, None, True
            x = F.linear(x, fc[0], fc[1])
            yield "fc", x, q["fc.q"], sp["fc"]["s_y"], sp["fc"]["z_y"], True


def layer_report(qmodel, net, images, batch=32):
    """{name: result} in layer_names order for ``images`` run through
    ``qmodel`` and its fp32 original (layer_pairs): QuantErrorStats.result()
    for the u8 hand-offs, FloatErrorStats.result() for the fp32 ones; one
    stats object per name, one synchronisation, at the end."""
    from .qerror import score_pairs
    return score_pairs(layer_pairs(qmodel, net, images, batch), qmodel.device)
