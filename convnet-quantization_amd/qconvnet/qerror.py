"""Per-layer quantization error, scored where the activations are.

``QuantErrorStats`` accumulates, per channel, the signal and error sums, the
clipping counts and the largest error of batches of a u8 activation against
its fp32 reference with qcn_qerror_u8_f32 (ops.qerror): nothing synchronises
until ``result()``, which makes ONE device-to-host copy.  ``layer_report()``
walks a QuantizedConvNet and the BN-folded fp32 net it was built from side by
side and scores every hand-off of the int8 path that way.

Fields (include/qconvnet.h), per channel and under "tensor" for
the channels combined (sums summed, the max of the max):
  count, below (x under the lowest representable value), above (x over the
  highest), differ (q is not quantize(x): the error arrived from upstream, not
  from this hand-off's rounding), max_abs_err, sum_x2, sum_e2, sum_abs_e;
  sqnr_db = 10 log10(sum_x2 / sum_e2) (torch.ao.ns.fx.utils.compute_sqnr),
  mse, mean_abs_err, below_frac, above_frac, differ_frac.

``FloatErrorStats`` is the twin for an fp32 activation against its fp32
reference (qcn_qerror_f32_f32): count, differ (x != y),
max_abs_err, sum_x2, sum_e2, sum_abs_e, sum_e (signed); sqnr_db, mse,
mean_abs_err, mean_err, differ_frac.  The ResNet executors' reports
(qconvnet.resnet / qconvnet.resnet_qdq: layer_names, layer_pairs,
layer_report) are built on the two.

Not covered: the dynamic models, and a reduction over ranks (max_abs_err is
not a sum).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import ops

RAW = ("count", "below", "above", "differ", "max_abs_err", "sum_x2", "sum_e2", "sum_abs_e")
DERIVED = ("sqnr_db", "mse", "mean_abs_err", "below_frac", "above_frac", "differ_frac")


def _sqnr_db(sum_x2, sum_e2):
    x2 = np.asarray(sum_x2, np.float64)
    e2 = np.asarray(sum_e2, np.float64)
    out = np.full(x2.shape, np.nan)
    both = (x2 > 0) & (e2 > 0)
    out[both] = 10.0 * np.log10(x2[both] / e2[both])
    out[(e2 == 0) & (x2 > 0)] = np.inf
    out[(x2 == 0) & (e2 > 0)] = -np.inf
    return out


def _derive(r):
    n = np.maximum(r["count"], 1).astype(np.float64)
    r["sqnr_db"] = _sqnr_db(r["sum_x2"], r["sum_e2"])
    r["mse"] = r["sum_e2"] / n
    r["mean_abs_err"] = r["sum_abs_e"] / n
    for k in ("below", "above", "differ"):
        r[k + "_frac"] = r[k] / n
    return r


def summarize(counts, sums):
    """Host only: the report of int64 ``counts`` [c, 5] and float64 ``sums``
    [c, 3] as qcn_qerror_u8_f32 leaves them — a dict of numpy arrays [c] (RAW
    and DERIVED fields) plus "tensor", the same fields as scalars for the
    channels combined."""
    counts = np.ascontiguousarray(counts, np.int64).reshape(-1, 5)
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 3)
    if counts.shape[0] != sums.shape[0]:
        raise ValueError("summarize: counts [c, 5] and sums [c, 3] of the same c")
    r = {"count": counts[:, 0].copy(), "below": counts[:, 1].copy(), "above": counts[:, 2].copy(),
         "differ": counts[:, 3].copy(),
         "max_abs_err": counts[:, 4].astype(np.uint32).view(np.float32).copy(),
         "sum_x2": sums[:, 0].copy(), "sum_e2": sums[:, 1].copy(), "sum_abs_e": sums[:, 2].copy()}
    t = {k: r[k].sum() for k in RAW if k != "max_abs_err"}
    t["max_abs_err"] = r["max_abs_err"].max() if len(r["max_abs_err"]) else np.float32(0)
    r = _derive(r)
    r["tensor"] = {k: v[()] for k, v in _derive({k: np.asarray(v) for k, v in t.items()}).items()}
    return r


class QuantErrorStats:
    """Running error statistics of one activation with ``channels`` channels."""

    def __init__(self, channels, device="cuda"):
        from .qmodel import cuda_device
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError("QuantErrorStats: expected at least one channel")
        self.device = cuda_device(device)
        c = self.channels
        # counts and sums share one buffer so one copy brings both
        self._buf = torch.zeros(8 * c, dtype=torch.int64, device=self.device)
        self.counts = self._buf[:5 * c].view(c, 5)
        self.sums = self._buf[5 * c:].view(torch.float64).view(c, 3)
        self._ws = None

    def update(self, x, q, scale, zero_point, nhwc=True):
        """Add one batch: ``x`` device fp32 [n, channels, h, w] or [rows,
        channels]; ``q`` the u8 activation (NHWC when ``nhwc``).  Launches on
        the current stream of the device; no sync.  Calls on concurrent streams
        need one QuantErrorStats each."""
        if not (x.is_cuda and q.is_cuda):
            raise ValueError("QuantErrorStats.update: expected device tensors")
        if x.dim() not in (2, 4) or x.shape[1] != self.channels:
            raise ValueError(f"QuantErrorStats.update: expected {self.channels} channels")
        with torch.cuda.device(self.device):
            h, w = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, 1)
            need = ops.qerror_workspace_size(x.shape[0], self.channels, h, w)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
            ops.qerror(x.contiguous(), q.contiguous(), scale, zero_point, self.counts, self.sums,
                       nhwc=nhwc, workspace=self._ws)
        return self

    def result(self):
        """ONE device-to-host copy (it waits for the current stream);
        summarize() of the counts and sums."""
        with torch.cuda.device(self.device):
            raw = self._buf.cpu().numpy()
        c = self.channels
        return summarize(raw[:5 * c], raw[5 * c:].view(np.float64))

    def reset(self):
        self._buf.zero_()
        return self


RAW_F32 = ("count", "differ", "max_abs_err", "sum_x2", "sum_e2", "sum_abs_e", "sum_e")
DERIVED_F32 = ("sqnr_db", "mse", "mean_abs_err", "mean_err", "differ_frac")


def _derive_f32(r):
    n = np.maximum(r["count"], 1).astype(np.float64)
    r["sqnr_db"] = _sqnr_db(r["sum_x2"], r["sum_e2"])
    r["mse"] = r["sum_e2"] / n
    r["mean_abs_err"] = r["sum_abs_e"] / n
    r["mean_err"] = r["sum_e"] / n
    r["differ_frac"] = r["differ"] / n
    return r


def summarize_f32(counts, sums):
    """Host only: the report of int64 ``counts`` [c, 3] and float64 ``sums``
    [c, 4] as qcn_qerror_f32_f32 leaves them — a dict of numpy arrays [c]
    (RAW_F32 and DERIVED_F32 fields; differ counts x != y, mean_err is the
    signed mean of x - y) plus "tensor", the same fields as scalars for the
    channels combined.  sqnr_db follows summarize()'s +-inf / nan rules."""
    counts = np.ascontiguousarray(counts, np.int64).reshape(-1, 3)
    sums = np.ascontiguousarray(sums, np.float64).reshape(-1, 4)
    if counts.shape[0] != sums.shape[0]:
        raise ValueError("summarize_f32: counts [c, 3] and sums [c, 4] of the same c")
    r = {"count": counts[:, 0].copy(), "differ": counts[:, 1].copy(),
         "max_abs_err": counts[:, 2].astype(np.uint32).view(np.float32).copy(),
         "sum_x2": sums[:, 0].copy(), "sum_e2": sums[:, 1].copy(), "sum_abs_e": sums[:, 2].copy(),
         "sum_e": sums[:, 3].copy()}
    t = {k: r[k].sum() for k in RAW_F32 if k != "max_abs_err"}
    t["max_abs_err"] = r["max_abs_err"].max() if len(r["max_abs_err"]) else np.float32(0)
    r = _derive_f32(r)
    r["tensor"] = {k: v[()] for k, v in _derive_f32({k: np.asarray(v) for k, v in t.items()}).items()}
    return r


class FloatErrorStats:
    """QuantErrorStats' twin for an fp32 activation against its fp32
    reference (qcn_qerror_f32_f32, ops.qerror_f32): one buffer, no sync until
    ``result()``, one copy there."""

    def __init__(self, channels, device="cuda"):
        from .qmodel import cuda_device
        self.channels = int(channels)
        if self.channels < 1:
            raise ValueError("FloatErrorStats: expected at least one channel")
        self.device = cuda_device(device)
        c = self.channels
        self._buf = torch.zeros(7 * c, dtype=torch.int64, device=self.device)
        self.counts = self._buf[:3 * c].view(c, 3)
        self.sums = self._buf[3 * c:].view(torch.float64).view(c, 4)
        self._ws = None

    def update(self, x, y, nhwc=True):
        """Add one batch: ``x`` device fp32 [n, channels, h, w] or [rows,
        channels]; ``y`` the fp32 activation (NHWC when ``nhwc``).  Launches on
        the current stream of the device; no sync."""
        if not (x.is_cuda and y.is_cuda):
            raise ValueError("FloatErrorStats.update: expected device tensors")
        if x.dim() not in (2, 4) or x.shape[1] != self.channels:
            raise ValueError(f"FloatErrorStats.update: expected {self.channels} channels")
        with torch.cuda.device(self.device):
            h, w = (x.shape[2], x.shape[3]) if x.dim() == 4 else (1, 1)
            need = ops.qerror_f32_workspace_size(x.shape[0], self.channels, h, w)
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(max(need, 8), dtype=torch.uint8, device=self.device)
            ops.qerror_f32(x.contiguous(), y.contiguous(), self.counts, self.sums, nhwc=nhwc,
                           workspace=self._ws)
        return self

    def result(self):
        """ONE device-to-host copy (it waits for the current stream);
        summarize_f32() of the counts and sums."""
        with torch.cuda.device(self.device):
            raw = self._buf.cpu().numpy()
        c = self.channels
        return summarize_f32(raw[:3 * c], raw[3 * c:].view(np.float64))

    def reset(self):
        self._buf.zero_()
        return self


def _conv_deterministic(x, w, b, stride=1, padding=1):
    """F.conv2d with a deterministic algorithm (the default choice for the
    8x8 layers at small batches adds in a varying order)."""
    prev = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        return F.conv2d(x, w, b, stride=stride, padding=padding)
    finally:
        torch.backends.cudnn.deterministic = prev


def score_pairs(pairs, device):
    """{name: result} in first-seen order for an iterable of (name, x_fp32,
    y, scale, zero_point, nhwc): a u8 ``y`` is scored by a QuantErrorStats
    with (scale, zero_point), an fp32 ``y`` by a FloatErrorStats; one stats
    object per name, one synchronisation, at the end."""
    stats = {}
    for name, x, y, scale, zp, nhwc in pairs:
        st = stats.get(name)
        if y.dtype == torch.uint8:
            if st is None:
                st = stats[name] = QuantErrorStats(x.shape[1], device)
            st.update(x, y, scale, zp, nhwc)
        else:
            if st is None:
                st = stats[name] = FloatErrorStats(x.shape[1], device)
            st.update(x, y, nhwc)
    if not stats:
        raise ValueError("layer_report: no images")
    return {name: st.result() for name, st in stats.items()}


def layer_names(mode):
    convs = ["x"] + [f"conv{i}" for i in range(1, 7)] + ["fc1"]
    return convs + ["fc2"] if mode == "static" else convs


def layer_pairs(qmodel, folded, images, batch=256):
    """Yield (name, x_fp32, q_u8, scale, zero_point, nhwc) for every hand-off
    of ``qmodel`` (a QuantizedConvNet), batch by batch, in layer_names(mode)
    order within a batch.  ``folded``: the BN-folded fp32 weights the model was
    built from (qmodel.fold_state_dict); ``images``: fp32 NCHW, or raw uint8
    NHWC (normalised with the model's mean / std), host or device.

    Per batch, on the model's device and current stream: the fp32 net through
    torch ops (the walk of qmodel.calibrate) and ``qmodel.run(x, keep=True)``
    with conv1 as its own launch, so a1 exists.
      "x":     the input against ops.quantize of it (input qparams);
      conv i:  the fp32 output after ReLU (and the pool) against a_i — with
               the layer's (s_y, z_y) in static mode, the hand-off's (the next
               layer's (s_x, z_x)) in qdq mode;
      fc1:     static: after ReLU against f1; qdq: before ReLU against f1;
      fc2:     static only: the fp32 logits against q.
    The u8 tensors are the model's reused buffers: use them before taking the
    next item of the next batch.  No sync."""
    from .qmodel import CONV_TABLE, normalized_input
    if batch < 1:
        raise ValueError("layer_pairs: batch must be positive")
    dev = qmodel.device
    static = qmodel.mode == "static"
    sp = qmodel.spec
    fuse12 = qmodel.fuse12
    with torch.cuda.device(dev), torch.no_grad():
        t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in folded.items()}
        for a in range(0, images.shape[0], batch):
            xb = images[a:a + batch].to(dev)
            x = normalized_input(xb, dev, qmodel.ntab).contiguous()
            qmodel.fuse12 = False
            try:
                _, b = qmodel.run(xb.contiguous() if xb.dtype == torch.uint8 else x, keep=True)
            finally:
                qmodel.fuse12 = fuse12
            yield ("x", x, ops.quantize(x, qmodel.in_scale, qmodel.in_zp), qmodel.in_scale,
                   qmodel.in_zp, True)
            for i, (_, _, pool) in enumerate(CONV_TABLE, start=1):
                # a deterministic algorithm: two walks over the same images give
                # the same fp32 reference, so two reports can be compared
                x = _conv_deterministic(x, t[f"conv{i}.w"], t[f"conv{i}.b"])
                x = F.relu(x)
                if pool:
                    x = F.max_pool2d(x, 2, 2)
                x = x.contiguous()
                e = sp[f"conv{i}"]
                s, z = (e["s_y"], e["z_y"]) if static else e["next"]
                yield f"conv{i}", x, b[f"a{i}"], s, z, True
            x = F.linear(x.reshape(x.shape[0], -1), t["fc1.w"], t["fc1.b"])
            e = sp["fc1"]
            if static:
                x = F.relu(x)
            yield "fc1", x.contiguous(), b["f1"], e["s_y"], e["z_y"], True
            if static:
                x = F.linear(x, t["fc2.w"], t["fc2.b"])
                e = sp["fc2"]
                yield "fc2", x.contiguous(), b["q"], e["s_y"], e["z_y"], True


def layer_report(qmodel, folded, images, batch=256):
    """{layer: QuantErrorStats.result()} in layer order for ``images`` run
    through ``qmodel`` and its fp32 original (layer_pairs), one
    QuantErrorStats per layer; one synchronisation, at the end."""
    stats = {}
    for name, x, q, scale, zp, nhwc in layer_pairs(qmodel, folded, images, batch):
        st = stats.get(name)
        if st is None:
            st = stats[name] = QuantErrorStats(x.shape[1], qmodel.device)
        st.update(x, q, scale, zp, nhwc)
    if not stats:
        raise ValueError("layer_report: no images")
    return {name: st.result() for name, st in stats.items()}
