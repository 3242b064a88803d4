"""DynamicPTQModel — drop-in for /root/reference/models/dynamic_ptq_model.py:218-317.

Reference behaviour: duck-typed model (load_state_dict, eval, cpu, to, forward,
__call__ :234-279); quantize() folds conv_i+bn_i and fc1+bn7 (:289-299) then
``quantize_dynamic({Linear, Conv2d}, qint8)`` (:302-306).  torch has no dynamic
mapping for Conv2d, so the effect is BN-folded fp32 convs + dynamic int8
fc1/fc2.

MI355X version: fc1 and fc2 run ``quantized::linear_dynamic`` semantics in the
HIP kernel (device-side min/max -> ChooseQuantizationParams with reduce_range
-> LEGACY quantize -> u8 x s8 MFMA GEMM -> y = fmaf(acc, s_x*s_w, b)), bit-exact
with FBGEMM for the same fp32 input.  The six fp32 convolutions are the
reference's fp32 ops: through torch (MIOpen) on the same device by default
(``body="torch"``), or through the deterministic HIP kernel of
csrc/conv_f32.hip (``body="hip"``), which makes the features, and
with ``granularity="sample"`` the logits, independent of the batch.
``body="int8"`` goes past the reference: the six convolutions are
dynamically quantized too, every image by its own range, on the int8 MFMA
(csrc/conv_dyn.hip); nothing is calibrated and the batch independence holds
by integer arithmetic.  ``body="bf16"`` keeps the
reference's operation at reduced operand precision: activations and weights are
rounded to bf16, the sums are fp32 in a fixed order on the bf16 MFMA
(csrc/conv_bf16.hip), and the layers hand their activations on as bf16.  The
ResNet-50
``CustomDynamicQuantization`` of :13-216 needs torchvision and a weight
download and is out of scope.
"""
from __future__ import annotations

import io

import numpy as np
import torch
import torch.nn.functional as F

from models.baseline_model import CONV_TABLE, SimpleConvNet, load_checkpoint_state
from qconvnet import ops
from qconvnet import quant as Q
from qconvnet.data import CIFAR_MEAN, CIFAR_STD
from qconvnet.qmodel import cuda_device, fold_state_dict, normalized_input

F32 = np.float32
GRANULARITIES = ("batch", "sample")
BODIES = ("torch", "hip", "int8", "bf16")


def check_granularity(granularity):
    if granularity not in GRANULARITIES:
        raise ValueError(f"unknown granularity {granularity!r} (expected one of {GRANULARITIES})")
    return granularity


def check_body(body):
    if body not in BODIES:
        raise ValueError(f"unknown body {body!r} (expected one of {BODIES})")
    return body


def check_pairs(pairs, body):
    if not (isinstance(pairs, bool) or pairs == "all"):
        raise ValueError(f'unknown pairs {pairs!r} (expected False, True or "all")')
    if pairs and body != "int8":
        raise ValueError(f'pairs={pairs!r} needs body="int8" (got body="{body}"): only the dynamic int8 '
                         "convs have a pair kernel")
    return pairs


class DynamicQuantConvNet:
    """fp32 convs (+ optional BN fold) and dynamic-int8 fc1/fc2 on the GPU.
    Raw uint8 NHWC images are normalised with ``mean`` / ``std`` on the device
    (ops.normalize_u8).

    ``granularity``: whose min/max gives a dynamic Linear's activation qparams.
    "batch" (default) is torch's quantize_dynamic: one range per call, so an
    image's logits depend on the other images of its batch, and a batch split
    over ranks needs the all-reduce of ``_range`` to stay batch-exact.
    "sample": every row is quantized with its own range
    (ops.linear_dynamic_rows): ``classify`` gives each row the result it
    would get alone, at any batch size and in any shard, so no collective is
    needed and ``sharded`` is not consulted.

    ``body``: who runs the six fp32 convolutions of ``features``.  "torch"
    (default) is F.conv2d, i.e. MIOpen, whose algorithm and summation order may
    differ per batch size.  "hip" is ops.conv3x3_f32, six launches with BN,
    ReLU and the pools in their epilogues and a summation order fixed by the
    kernel: an image's features are the same bits in any batch, so with
    granularity="sample" the logits are too, images in to logits out.
    "int8" is ops.conv3x3_dyn: the conv weights are quantized once (symmetric
    s8, per output channel unless ``conv_per_channel=False``), every layer
    quantizes each image's activations with the qparams of that image's own
    min/max (full 8 bits: ``reduce_range`` applies to the Linears only) and
    accumulates in int32, so the same invariance holds and the convolutions are
    no longer the reference's fp32 ops.
    "bf16" is ops.conv3x3_bf16: six launches like "hip", the operands rounded
    to bf16 (8 bits of relative precision, fp32's range, nothing calibrated),
    the sums and the epilogues in fp32 in an order fixed by the kernel, conv1
    to conv5 writing bf16 NHWC, the bits the next layer would round to anyway:
    the same invariance at half the activation bytes.

    ``pairs`` (body="int8" only, default False): a layer without a pool and
    its successor run as one ops.conv3x3_dyn_pair launch wherever
    ops.conv3x3_dyn_pair_supported serves the shape (conv3 + conv4 and
    conv5 + conv6), the activation between them handed over as u8
    in LDS.  ``pairs="all"`` also takes ops.conv3x3_dyn_pair32 where the first
    kernel does not serve the shape and that one does (conv1 + conv2; DESIGN
    §26): features() is then min/max and three pair launches.  The bits are
    those of ``pairs=False``."""

    def __init__(self, state_dict, fold=True, device="cuda", reduce_range=True, mean=CIFAR_MEAN,
                 std=CIFAR_STD, granularity="batch", body="torch", conv_per_channel=True, pairs=False):
        self.granularity = check_granularity(granularity)
        self.body = check_body(body)
        self.pairs = check_pairs(pairs, body)
        self.device = cuda_device(device)
        self.ntab = Q.normalize_table(mean, std).to(self.device)
        self.reduce_range = reduce_range
        self.sharded = False   # True: batch-exact across ranks (see _range)
        self.quantized = True
        self.host_io = False
        g = {k: v.detach().cpu().numpy() for k, v in state_dict.items() if torch.is_tensor(v)}
        if fold:
            f = fold_state_dict(state_dict)
            convs = [(f[f"conv{i}.w"], f[f"conv{i}.b"], None) for i in range(1, 7)]
            fc1w, fc1b, self.bn7 = f["fc1.w"], f["fc1.b"], None
        else:
            convs = [(g[f"conv{i}.weight"], g[f"conv{i}.bias"],
                      tuple(g[f"bn{i}.{k}"] for k in ("running_mean", "running_var", "weight", "bias")))
                     for i in range(1, 7)]
            fc1w, fc1b = g["fc1.weight"], g["fc1.bias"]
            # bn7 in ATen's CPU op order (fma(x, alpha, beta')), so the dynamic
            # fc2 sees bit-identical input to the reference's CPU model
            self.bn7 = tuple(self._t(a) for a in Q.bn_eval_affine(
                *(g[f"bn7.{k}"] for k in ("running_mean", "running_var", "weight", "bias"))))
        self.convs = [(self._t(w), self._t(b), tuple(self._t(a) for a in bn) if bn else None)
                      for w, b, bn in convs]
        self.packed = None
        if self.body == "hip":
            # (packed weights, bias, BN as fma(x, alpha, beta) or None) per conv
            self.packed = [(self._t(ops.pack_conv3x3_f32(w)), self._t(b),
                            tuple(self._t(a) for a in Q.bn_eval_affine(*bn)) if bn else None)
                           for w, b, bn in convs]
        self.bconvs = None
        if self.body == "bf16":
            # (packed bf16 weights, bias, BN as fma(x, alpha, beta) or None) per conv
            self.bconvs = [(self._t(ops.pack_conv3x3_bf16(w)), self._t(b),
                            tuple(self._t(a) for a in Q.bn_eval_affine(*bn)) if bn else None)
                           for w, b, bn in convs]
        self.qconvs = None
        if self.body == "int8":
            # (packed s8 weights, wsum, s_w, bias, BN as fma(x, alpha, beta) or None) per conv
            self.qconvs = []
            for w, b, bn in convs:
                flat = w.reshape(w.shape[0], -1)
                s_w = (Q.qparams_symmetric(flat.min(1), flat.max(1)) if conv_per_channel
                       else np.atleast_1d(Q.qparams_symmetric(w.min(), w.max())))
                wp, wsum = ops.pack_conv3x3_dyn(Q.quantize_weight(w, s_w))
                self.qconvs.append((self._t(wp), self._t(wsum), self._t(s_w), self._t(b),
                                    tuple(self._t(a) for a in Q.bn_eval_affine(*bn)) if bn else None))
        self.fc = []
        for w, b in ((fc1w, fc1b), (g["fc2.weight"], g["fc2.bias"])):
            s_w = Q.qparams_symmetric(w.min(), w.max())     # default_weight_observer
            wq = Q.quantize_weight(w, s_w)
            self.fc.append((self._t(wq), self._t(np.atleast_1d(s_w)),
                            self._t(wq.astype(np.int64).sum(1).astype(np.int32)), self._t(b)))

    def _t(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.device)

    def _range(self, x):
        """None (each call uses its own batch range, quantize_dynamic's
        semantics) unless ``sharded`` is set — this process runs one shard of a
        batch split over the ranks (qconvnet.dist.sharded_forward): then the
        range is all-reduced so every shard quantizes exactly as the whole
        batch would (one 2-float RCCL all-reduce per dynamic Linear; every rank
        must make the same calls)."""
        import torch.distributed as dist
        if not self.sharded or not (dist.is_available() and dist.is_initialized()) \
                or dist.get_world_size() == 1:
            return None
        from qconvnet.dist import global_minmax
        return global_minmax(ops.minmax_range(x))

    @torch.no_grad()
    def __call__(self, x):
        with torch.cuda.device(self.device):   # ops launch on this device's current stream
            return self._forward(x)

    def features(self, x):
        """fp32 convs (+BN, ReLU, pools) -> the [N, 4096] NCHW-flatten fc1 input."""
        if self.body == "hip":
            return self._features_hip(x)
        if self.body == "int8":
            return self._features_int8(x)
        if self.body == "bf16":
            return self._features_bf16(x)
        for i, (w, b, bn) in enumerate(self.convs):
            x = F.conv2d(x, w, b, padding=1)
            if bn is not None:
                x = F.batch_norm(x, bn[0], bn[1], bn[2], bn[3], False, 0.0, 1e-5)
            x = F.relu(x)
            if CONV_TABLE[i][2]:
                x = F.max_pool2d(x, 2, 2)
        return x.reshape(x.shape[0], -1).contiguous()

    def _features_hip(self, x):
        """NCHW in at conv1, NHWC between the layers, NCHW-flatten out of conv6."""
        x = x.contiguous()
        last = len(self.packed) - 1
        for i, (wp, b, affine) in enumerate(self.packed):
            x = ops.conv3x3_f32(x, wp, CONV_TABLE[i][1], bias=b, affine=affine, relu=True,
                                pool=bool(CONV_TABLE[i][2]), x_nchw=i == 0, y_nchw=i == last)
        return x.reshape(x.shape[0], -1)

    def _features_bf16(self, x):
        """fp32 NCHW in at conv1, bf16 NHWC between the layers, fp32
        NCHW-flatten out of conv6."""
        x = x.contiguous()
        last = len(self.bconvs) - 1
        for i, (wp, b, affine) in enumerate(self.bconvs):
            x = ops.conv3x3_bf16(x, wp, CONV_TABLE[i][1], bias=b, affine=affine, relu=True,
                                 pool=bool(CONV_TABLE[i][2]), x_nchw=i == 0, y_nchw=i == last,
                                 y_bf16=i != last)
        return x.reshape(x.shape[0], -1)

    def _features_int8(self, x):
        """One per-image min/max launch, then six dynamic int8 convs, each
        handing its output's per-image range to the next (layouts as
        _features_hip).  With ``pairs``, a layer without a pool and the next
        one are one launch where a pair kernel serves the shape (the 32 x 32
        one with ``pairs="all"`` only)."""
        x = x.contiguous()
        stats = ops.image_minmax(x)
        last = len(self.qconvs) - 1
        h, w = x.shape[2:]
        i = 0
        while i <= last:
            (wp, wsum, s_w, b, affine), (cin, cout, pool) = self.qconvs[i], CONV_TABLE[i]
            pair = None
            if self.pairs and i < last and not pool:
                shape = (h, w, cin, cout, CONV_TABLE[i + 1][1])
                if ops.conv3x3_dyn_pair_supported(*shape):
                    pair = ops.conv3x3_dyn_pair
                elif self.pairs == "all" and ops.conv3x3_dyn_pair32_supported(*shape):
                    pair = ops.conv3x3_dyn_pair32
            if pair is not None:
                layers = [ops.DynLayer(q[0], q[1], q[2], CONV_TABLE[j][1], bias=q[3], affine=q[4], relu=True)
                          for j, q in ((i, self.qconvs[i]), (i + 1, self.qconvs[i + 1]))]
                i, pool = i + 1, CONV_TABLE[i + 1][2]
                x, stats = pair(x, stats, layers[0], layers[1], pool=bool(pool),
                                x_nchw=i == 1, y_nchw=i == last, want_stats=i != last)
            else:
                x, stats = ops.conv3x3_dyn(x, stats, wp, wsum, s_w, cout, bias=b, affine=affine, relu=True,
                                           pool=bool(pool), x_nchw=i == 0, y_nchw=i == last,
                                           want_stats=i != last)
            if pool:
                h, w = h // 2, w // 2
            i += 1
        return x.reshape(x.shape[0], -1)

    def _linear(self, x, fc):
        w, s, ws, b = fc
        if self.granularity == "sample":
            return ops.linear_dynamic_rows(x, w, s, ws, b, self.reduce_range)
        return ops.linear_dynamic(x, w, s, ws, b, self.reduce_range, minmax=self._range(x))

    @torch.no_grad()
    def classify(self, feats):
        """dynamic-int8 fc1 -> [bn7] -> ReLU -> dynamic-int8 fc2 on [N, 4096]
        fp32 features (device tensor in, device logits out, no sync)."""
        with torch.cuda.device(self.device):
            x = self._linear(feats, self.fc[0])
            if self.bn7 is not None:
                x = ops.channel_affine(x, self.bn7[0], self.bn7[1], relu=True)
            else:
                x = F.relu(x).contiguous()
            return self._linear(x, self.fc[1])

    def _forward(self, x):
        host = not x.is_cuda
        x = normalized_input(x, self.device, self.ntab)
        y = self.classify(self.features(x))
        if host or self.host_io:
            return y.cpu()
        torch.cuda.current_stream(self.device).synchronize()
        return y

    forward = __call__

    def eval(self):
        return self

    def to(self, device):
        self.host_io = torch.device(device).type == "cpu"   # compute stays on the GPU
        return self

    def cpu(self):
        self.host_io = True
        return self


class DynamicPTQModel:
    def __init__(self, device="cuda"):
        self.fp32_model = SimpleConvNet()
        self.quantized_model = None
        self.device = device

    def load_state_dict(self, state_dict):
        self.fp32_model.load_state_dict(load_checkpoint_state(state_dict))

    def eval(self):
        (self.quantized_model or self.fp32_model).eval()
        return self

    def cpu(self):
        if self.quantized_model is not None:
            self.quantized_model.cpu()
        else:
            self.fp32_model = self.fp32_model.cpu()
        return self

    def to(self, device):
        if self.quantized_model is not None:
            self.quantized_model.to(device)
        else:
            self.fp32_model = self.fp32_model.to(device)
        return self

    def forward(self, x):
        if self.quantized_model is not None:
            return self.quantized_model(x)
        return self.fp32_model(x)

    def __call__(self, x):
        return self.forward(x)

    def quantize(self, mean=CIFAR_MEAN, std=CIFAR_STD, granularity="batch", body="torch", pairs=False):
        """``mean`` / ``std``: the Normalize constants applied to raw uint8
        NHWC images.  ``granularity``: "batch" (quantize_dynamic's per-call
        activation range) or "sample" (one range per image).  ``body``:
        "torch" (MIOpen convolutions), "hip" (ops.conv3x3_f32), "int8"
        (ops.conv3x3_dyn, the convolutions dynamically quantized per image as
        well) or "bf16" (ops.conv3x3_bf16, bf16 operands and hand-offs, fp32
        sums); with "sample" and "hip", "int8" or "bf16" an image's logits are
        bit-identical whatever batch it arrives in (see DynamicQuantConvNet).
        ``pairs``: with "int8", conv3 + conv4 and conv5 + conv6 as one launch
        each (ops.conv3x3_dyn_pair), with "all" conv1 + conv2 too
        (ops.conv3x3_dyn_pair32), the same bits."""
        check_granularity(granularity)
        check_pairs(pairs, check_body(body))
        self.fp32_model = self.fp32_model.cpu().eval()
        self.quantized_model = DynamicQuantConvNet(self.fp32_model.state_dict(), fold=True,
                                                   device=self.device, mean=mean, std=std,
                                                   granularity=granularity, body=body, pairs=pairs)
        return self.quantized_model

    def get_model_size(self):
        buf = io.BytesIO()
        q = self.quantized_model
        torch.save([t for fc in q.fc for t in fc] + [t for c in q.qconvs or () for t in c[:4]] +
                   [c[0] for c in q.bconvs or ()], buf)
        return buf.tell() / (1024 * 1024)
