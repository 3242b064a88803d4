"""StaticPTQModel — drop-in for /root/reference/models/static_ptq_model.py:7-43.

Reference behaviour: a plain wrapper holding ``fp32_model`` / ``quantized_model``;
``quantize(calibration_data_loader=None)`` returns the quantized model and
``get_model_size(model)`` reports MB.  The reference's quantize() actually calls
``quantize_dynamic`` (only fc1/fc2 become int8).  Here
``quantize`` does what the class name and BASELINE config 3 promise: true
static PTQ of the whole net — BN folded, MinMax-calibrated activations, every
conv and linear int8 on the MI355X (``QuantizedConvNet``, static mode), with
torch.ao/fbgemm numerics bit for bit.  The calibration loader is used (the
reference ignores it); with none, 512 synthetic CIFAR images are used.
"""
from __future__ import annotations

import io

import torch

from models.baseline_model import SimpleConvNet, load_checkpoint_state
from qconvnet import data
from qconvnet.qmodel import QuantizedConvNet, build_qspec, calibrate, fold_state_dict


class StaticPTQModel:
    """mode="static" (default): full static int8 on the MI355X.
    mode="reference": the reference's actual semantics — quantize_dynamic on the
    unfolded net (fp32 convs + BN, dynamic int8 fc1/fc2; the dynamic Linear on
    the HIP kernel)."""

    def __init__(self, device="cuda", mode="static"):
        if mode not in ("static", "reference"):
            raise ValueError(f"unknown mode {mode!r}")
        self.fp32_model = SimpleConvNet()
        self.quantized_model = None
        self.device = device
        self.mode = mode

    def load_state_dict(self, state_dict):
        self.fp32_model.load_state_dict(load_checkpoint_state(state_dict))

    def quantize(self, calibration_data_loader=None, per_channel=False, calibration_device="cpu",
                 max_batches=None, observer="minmax", mean=data.CIFAR_MEAN, std=data.CIFAR_STD,
                 granularity="batch"):
        """Calibrate (fp32, BN folded — the reference quantizes on the CPU, so
        does the default here) and build the int8 GPU model.  observer:
        "minmax" (default) or "histogram", torch.ao's default
        HistogramObserver (get_default_qconfig('fbgemm') activations,
        reduce_range=False).  ``mean`` / ``std``: the Normalize constants
        applied to raw uint8 NHWC images (calibration batches and inference
        inputs may be either those or normalised fp32 NCHW).  ``granularity``
        ("batch" or "sample") belongs to mode="reference": whose range gives
        the dynamic fc1/fc2 their activation qparams (DynamicQuantConvNet);
        the static net has no dynamic layer, so "sample" is an error there."""
        from models.dynamic_ptq_model import DynamicQuantConvNet, check_granularity
        check_granularity(granularity)
        if self.mode == "static" and granularity != "batch":
            raise ValueError('granularity="sample" needs mode="reference": the static net has no '
                             "dynamic layer")
        self.fp32_model.eval()
        if self.mode == "reference":
            self.quantized_model = DynamicQuantConvNet(self.fp32_model.state_dict(), fold=False,
                                                       device=self.device, mean=mean, std=std,
                                                       granularity=granularity)
            return self.quantized_model
        folded = fold_state_dict(self.fp32_model.state_dict())
        batches = data.calibration_batches(calibration_data_loader, max_batches)
        ranges = calibrate(folded, batches, calibration_device, observer=observer, mode="static",
                           mean=mean, std=std)
        spec = build_qspec(folded, ranges, "static", per_channel)
        self.quantized_model = QuantizedConvNet(spec, self.device, mean=mean, std=std)
        return self.quantized_model

    def quantization_report(self, images, batch=256):
        """Per-layer quantization error of ``images`` (fp32 NCHW or raw uint8
        NHWC): {layer: per-channel and whole-tensor SQNR, clipping and rounding
        statistics} — qconvnet.qerror.layer_report of the int8 model against
        the BN-folded ``fp32_model``.  The reference prints one
        torch.abs(fp32_output - int8_output).mean() (static_ptq_model.py:93-95)."""
        if not isinstance(self.quantized_model, QuantizedConvNet):
            raise RuntimeError("quantization_report: call quantize() first (mode='static')")
        from qconvnet.qerror import layer_report
        self.fp32_model.eval()
        folded = fold_state_dict(self.fp32_model.state_dict())
        return layer_report(self.quantized_model, folded, images, batch)

    def get_model_size(self, model):
        """MB of the serialized parameters (the reference writes temp_model.pth
        into the CWD, static_ptq_model.py:36-43; this uses an in-memory buffer)."""
        buf = io.BytesIO()
        if isinstance(model, QuantizedConvNet):
            torch.save({k: v for k, v in model.spec.items()}, buf)
        else:
            torch.save(model.state_dict(), buf)
        return buf.tell() / (1024 * 1024)
