"""ModelEvaluator — drop-in for /root/reference/utils/model_evaluator.py:10-204.

* ``evaluate_accuracy`` (:15-55): top-1/top-5 with ``topk(5, 1, True, True)``.
  torch's ``topk`` leaves the order of tied values unspecified (on rows with
  few distinct values its index set differs from a stable descending sort),
  so on quantized logits the host path's top-5 is whatever that call picks;
* ``evaluate_class_accuracy`` (:57-119): per-class top-1 (``torch.max``
  argmax), sorted by accuracy, descending;
* ``compare_models`` (:121-204): overall and per-class accuracy per model.

The reference moves every quantized model to the CPU (:20, :78-81, :139-142).
Here ``model.cpu()`` on our int8 models switches only their I/O to host
tensors — the HIP kernels still do the compute — so the reference's calling
pattern runs unchanged; with ``device="cuda"`` inputs go to the GPU and no
host round trip is made (the GPU counterpart of SURVEY §8(f) row 4).
Messages are in English; the tqdm progress bars are dropped.

``counts="device"`` (opt-in, needs a cuda ``device``) keeps the scoring on the
GPU: every batch's logits go through ``qconvnet.evaluate.EvalCounts``
(qcn_eval_topk_f32) with no ``.cpu()`` per batch and one copy at the end.  Its
tie rule is defined: a label is a top-k hit iff fewer than k columns beat it,
an equal value at a lower index counting as beating it (a stable descending
sort; NaN above everything, -0.0 == +0.0).  On tie-free logits both paths
return the same floats.  ``evaluate_all`` answers top-1, top-5 and per-class
accuracy from ONE pass over the loader."""
from __future__ import annotations

import torch


def _model_type(model):
    if hasattr(model, "quantized"):
        return ("custom quantized model" if getattr(model, "is_custom_quantized", False)
                else "quantized model")
    return "FP32 model"


class ModelEvaluator:
    def __init__(self, test_loader, device="cpu", counts="host"):
        if counts not in ("host", "device"):
            raise ValueError(f"unknown counts {counts!r}: 'host' or 'device'")
        if counts == "device" and torch.device(device).type != "cuda":
            raise ValueError("counts='device' scores on the GPU: pass a cuda device")
        self.test_loader = test_loader
        self.device = device
        self.counts = counts

    def _place(self, model):
        """(model, input device): every model goes to self.device.  The reference
        forces quantized models to the CPU (:78-84) because fbgemm runs there;
        our int8 models compute on the GPU, and with self.device == "cpu" they
        take host tensors and keep their compute on the GPU (model.cpu())."""
        model.eval()
        if str(self.device) == "cpu":
            return model.cpu(), torch.device("cpu")
        model.to(self.device)
        return model, torch.device(self.device)

    def _predict(self, model, device):
        with torch.no_grad():
            for images, labels in self.test_loader:
                out = model(images.to(device))
                yield out.cpu(), labels.cpu()

    def _logits(self, model, device):
        """counts="device": (device logits, labels as the loader gives them)."""
        with torch.no_grad():
            for images, labels in self.test_loader:
                out = model(images.to(device, non_blocking=True))
                if not (torch.is_tensor(out) and out.is_cuda):
                    raise ValueError("counts='device' needs a model that returns device tensors")
                yield out, labels

    def _device_result(self, model, device):
        """One pass over the loader through EvalCounts (k = 5); one copy."""
        from qconvnet.evaluate import EvalCounts
        counts = None
        for out, labels in self._logits(model, device):
            if counts is None:
                counts = EvalCounts(out.shape[1], out.device, 5)
            counts.update(out, labels)
        if counts is None:
            raise ValueError("the test loader is empty")
        return counts.result()

    @staticmethod
    def _fit(a, n):
        """Per-class counts over the model's classes as float64 [n] (the host
        path's bincount(...)[:n] with minlength n)."""
        out = torch.zeros(n, dtype=torch.float64)
        m = min(n, a.shape[0])
        out[:m] = torch.from_numpy(a[:m].copy()).double()
        return out

    def evaluate_accuracy(self, model, verbose=True):
        model, device = self._place(model)
        if self.counts == "device":
            r = self._device_result(model, device)
            top1, top5 = 100.0 * r["top1"] / r["rows"], 100.0 * r["topk"] / r["rows"]
            if verbose:
                print(f"Top-1 Accuracy: {top1:.2f}%\nTop-5 Accuracy: {top5:.2f}%")
            return top1, top5
        c1 = c5 = total = 0
        for out, labels in self._predict(model, device):
            _, pred = out.topk(5, 1, True, True)
            pred = pred.t()
            correct = pred.eq(labels.view(1, -1).expand_as(pred))
            c1 += correct[0].sum().item()
            c5 += correct.sum().item()
            total += labels.size(0)
        top1, top5 = 100.0 * c1 / total, 100.0 * c5 / total
        if verbose:
            print(f"Top-1 Accuracy: {top1:.2f}%\nTop-5 Accuracy: {top5:.2f}%")
        return top1, top5

    def _class_counts(self, model, device, n_classes):
        if self.counts == "device":
            r = self._device_result(model, device)
            return self._fit(r["class_correct"], n_classes), self._fit(r["class_total"], n_classes)
        correct = torch.zeros(n_classes, dtype=torch.float64)
        total = torch.zeros(n_classes, dtype=torch.float64)
        for out, target in self._predict(model, device):
            _, predicted = torch.max(out, 1)
            total += torch.bincount(target, minlength=n_classes)[:n_classes].double()
            hit = target[predicted == target]
            correct += torch.bincount(hit, minlength=n_classes)[:n_classes].double()
        return correct, total

    @staticmethod
    def _sorted_class_acc(classes, correct, total):
        acc = {classes[i]: 100.0 * correct[i].item() / total[i].item()
               for i in range(len(classes)) if total[i] > 0}
        return dict(sorted(acc.items(), key=lambda kv: kv[1], reverse=True))

    def evaluate_class_accuracy(self, model, classes, verbose=True):
        kind = _model_type(model)
        model, device = self._place(model)
        correct, total = self._class_counts(model, device, len(classes))
        res = self._sorted_class_acc(classes, correct, total)
        if verbose:
            print(f"\n[{kind}] per-class accuracy (top 20 classes):")
            for i, (name, a) in enumerate(res.items()):
                if i >= 20:
                    break
                print(f"{name}: {a:.2f}%")
        return res

    def evaluate_all(self, model, classes, verbose=True):
        """(top-1 %, top-5 %, per-class accuracy sorted descending) from ONE
        pass over the loader: what evaluate_accuracy and
        evaluate_class_accuracy return, which walk it once each."""
        model, device = self._place(model)
        n = len(classes)
        if self.counts == "device":
            r = self._device_result(model, device)
            c1, c5, rows = r["top1"], r["topk"], r["rows"]
            correct, total = self._fit(r["class_correct"], n), self._fit(r["class_total"], n)
        else:
            c1 = c5 = rows = 0
            correct = torch.zeros(n, dtype=torch.float64)
            total = torch.zeros(n, dtype=torch.float64)
            for out, labels in self._predict(model, device):
                _, pred = out.topk(5, 1, True, True)
                hit = pred.t().eq(labels.view(1, -1).expand(5, -1))
                c1 += hit[0].sum().item()
                c5 += hit.sum().item()
                rows += labels.size(0)
                _, predicted = torch.max(out, 1)
                total += torch.bincount(labels, minlength=n)[:n].double()
                correct += torch.bincount(labels[predicted == labels], minlength=n)[:n].double()
        top1, top5 = 100.0 * c1 / rows, 100.0 * c5 / rows
        res = self._sorted_class_acc(classes, correct, total)
        if verbose:
            print(f"Top-1 Accuracy: {top1:.2f}%\nTop-5 Accuracy: {top5:.2f}%")
        return top1, top5, res

    def compare_models(self, models_dict, classes):
        results = {}
        print("\n=== Model accuracy comparison ===")
        for name, model in models_dict.items():
            kind = _model_type(model)
            m, device = self._place(model)
            correct, total = self._class_counts(m, device, len(classes))
            accuracy = 100.0 * correct.sum().item() / total.sum().item()
            results[name] = {"accuracy": accuracy,
                             "class_accuracies": self._sorted_class_acc(classes, correct, total)}
            print(f"[{kind}] {name} accuracy: {accuracy:.2f}%")
        print("\n=== Summary ===")
        for name, r in results.items():
            print(f"[{_model_type(models_dict[name])}] {name}: {r['accuracy']:.2f}%")
        return results

    def agreement(self, model_a, model_b):
        """Share of inputs where the two models' argmax agree (%)."""
        if self.counts == "device":
            return self._agreement_device(model_a, model_b)
        same = total = 0
        with torch.no_grad():
            for images, _ in self.test_loader:
                a = model_a(images).cpu().argmax(1)
                b = model_b(images).cpu().argmax(1)
                same += (a == b).sum().item()
                total += images.shape[0]
        return 100.0 * same / total

    def _agreement_device(self, model_a, model_b):
        """agreement() with the arg-max taken on the device (the ``pred``
        output of qcn_eval_topk_f32, torch.argmax's order) and the matches
        summed there: one copy at the end."""
        from qconvnet import ops
        dev = torch.device(self.device)
        same = scratch = None
        total = 0
        with torch.no_grad():
            for images, _ in self.test_loader:
                x = images.to(dev, non_blocking=True)
                preds = []
                for model in (model_a, model_b):
                    out = model(x)
                    if not (torch.is_tensor(out) and out.is_cuda):
                        raise ValueError("counts='device' needs a model that returns device tensors")
                    pred = torch.empty(out.shape[0], dtype=torch.int64, device=out.device)
                    with torch.cuda.device(out.device):   # only pred is wanted: any label does
                        scratch = ops.eval_topk(out.contiguous(), torch.zeros_like(pred), 1,
                                                scratch, pred=pred)
                    preds.append(pred)
                hits = (preds[0] == preds[1]).sum()
                same = hits if same is None else same + hits
                total += images.shape[0]
        return 100.0 * int(same.item()) / total
