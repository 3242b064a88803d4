"""Accuracy scoring that stays on the device.

``EvalCounts`` accumulates top-1 / top-k hits, per-class totals and correct
counts and (optionally) the confusion matrix of batches of logits with
qcn_eval_topk_f32 (ops.eval_topk): nothing synchronises until ``result()``,
which makes ONE device-to-host copy.  ``evaluate()`` scores a whole test set
that way, chunk by chunk over a few streams, with one sync at the end.

The order and the tie rule (include/qconvnet.h): NaN above
everything, -0.0 == +0.0, and a label hits top-k iff fewer than k columns beat
it, where an equal value at a lower index beats it — a stable descending sort.
The sums are integers, so results do not depend on how chunks interleave.
"""
from __future__ import annotations

import inspect

import torch

from . import dist, ops


class EvalCounts:
    """Running evaluation counts for ``num_classes`` classes on ``device``."""

    def __init__(self, num_classes, device="cuda", k=5, confusion=False):
        from .qmodel import cuda_device
        self.num_classes = int(num_classes)
        self.k = int(k)
        self.device = cuda_device(device)
        if self.num_classes < 1 or self.k < 1:
            raise ValueError("EvalCounts: expected num_classes >= 1 and k >= 1")
        c = self.num_classes
        n = ops.eval_counters_len(c)
        # counters and confusion share one buffer so one copy brings both
        self._buf = torch.zeros(n + (c * c if confusion else 0), dtype=torch.int64,
                                device=self.device)
        self.counters = self._buf[:n]
        self.confusion = self._buf[n:].view(c, c) if confusion else None

    def update(self, logits, labels, pred=None):
        """Add one batch: ``logits`` device fp32 [rows, num_classes];
        ``labels`` [rows] integers on the device or the host (they go up
        non_blocking).  ``pred`` (device int64 [rows]) receives the arg-max.
        Launches on the current stream of the device; no sync."""
        if not logits.is_cuda:
            raise ValueError("EvalCounts.update: the logits must be a device tensor")
        if logits.dim() != 2 or logits.shape[1] != self.num_classes:
            raise ValueError(f"EvalCounts.update: expected [rows, {self.num_classes}] logits")
        with torch.cuda.device(self.device):
            labels = labels.to(self.device, torch.int64, non_blocking=True).contiguous()
            ops.eval_topk(logits.contiguous(), labels, self.k, self.counters, self.confusion, pred)
        return self

    def all_reduce(self):
        """Sum the counts over the ranks (dist.sum_counts; no-op at world 1)."""
        with torch.cuda.device(self.device):
            dist.sum_counts(self._buf)
        return self

    def result(self):
        """ONE device-to-host copy (it waits for the current stream): python
        ints rows / top1 / topk / bad_labels, numpy int64 class_total /
        class_correct [num_classes] and confusion [num_classes, num_classes]
        (None when not kept)."""
        with torch.cuda.device(self.device):
            raw = self._buf.cpu().numpy()
        c = self.num_classes
        return {"rows": int(raw[0]), "top1": int(raw[1]), "topk": int(raw[2]),
                "bad_labels": int(raw[3]), "class_total": raw[4:4 + c].copy(),
                "class_correct": raw[4 + c:4 + 2 * c].copy(),
                "confusion": raw[4 + 2 * c:].reshape(c, c).copy() if self.confusion is not None
                else None}

    def reset(self):
        self._buf.zero_()
        return self


def _takes_slot(model):
    run = getattr(model, "run", None)
    if run is None:
        return False
    try:
        return "slot" in inspect.signature(run).parameters
    except (TypeError, ValueError):
        return False


def evaluate(model, images, labels, batch=1024, k=5, streams=2, confusion=False):
    """Score a whole test set with one sync at the end; returns
    EvalCounts.result().

    ``images``: the full set, on the host (pin it and the uploads overlap the
    forwards) or on the device; raw uint8 [N,H,W,3] or fp32 NCHW.  ``labels``:
    [N] integers, host or device.  ``streams``: how many streams (or the
    streams themselves).

    A model with ``run(x, slot=)`` (QuantizedConvNet) gets chunk j on
    streams[j % S], in this order on that stream: the chunk's host-to-device
    copy, ``run(x, slot=j % S)``, ``EvalCounts.update`` — so chunk j+1's upload
    overlaps chunk j's forward.  The counters are shared by the streams
    (integer atomics).  The last chunk is ragged.  Any other model is called
    as ``model(x)`` and must return a device tensor."""
    from .qmodel import cuda_device
    n = images.shape[0]
    if labels.shape[0] != n:
        raise ValueError("evaluate: one label per image")
    if batch < 1:
        raise ValueError("evaluate: batch must be positive")
    dev = getattr(model, "device", None)
    if dev is None or torch.device(dev).type != "cuda":
        dev = images.device if images.is_cuda else "cuda"
    dev = cuda_device(dev)
    slotted = _takes_slot(model)
    if isinstance(streams, int):
        if streams < 1:
            raise ValueError("evaluate: at least one stream")
        streams = [torch.cuda.Stream(device=dev) for _ in range(streams)]
    S = len(streams)
    counts = None
    with torch.cuda.device(dev), torch.no_grad():
        cur = torch.cuda.current_stream(dev)
        labels_d = labels.to(dev, torch.int64, non_blocking=True)
        for s in streams:
            s.wait_stream(cur)
        for j, a in enumerate(range(0, n, batch)):
            with torch.cuda.stream(streams[j % S]):
                x = images[a:a + batch].to(dev, non_blocking=True)
                out = model.run(x, slot=j % S) if slotted else model(x)
                if not (torch.is_tensor(out) and out.is_cuda):
                    raise ValueError("evaluate: the model must return a device tensor")
                if counts is None:
                    # the class count is known once the first forward is
                    # queued; the zeroing goes on the caller's stream (idle
                    # but for the labels' upload) and every stream waits for it
                    with torch.cuda.stream(cur):
                        counts = EvalCounts(out.shape[1], dev, k, confusion)
                    for s in streams:
                        s.wait_stream(cur)
                counts.update(out, labels_d[a:a + batch])
        for s in streams:
            cur.wait_stream(s)
        if counts is None:
            raise ValueError("evaluate: no images")
        return counts.result()
