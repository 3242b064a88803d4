"""Host-side quantization arithmetic of the product (one-time, at quantize()):
observer qparams, BN folding, weight quantization, and the fp32 epilogue
constants the HIP kernels consume.

Every function reproduces torch.ao / FBGEMM bit for bit (the committed golden
vectors in tests/golden/ pin it; tests/test_host_quant.py checks it):

* qparams_affine / qparams_symmetric — MinMaxObserver._calculate_qparams
  (torch/ao/quantization/observer.py:349-427);
* fold_bn — torch.nn.utils.fusion.fuse_conv_bn_weights / fuse_linear_bn_weights
  (torch/nn/utils/fusion.py:56-101, 156-186), called by the reference at
  /root/reference/models/custom_quantization_model.py:180-190 and
  /root/reference/models/dynamic_ptq_model.py:289-299;
* quantize_weight — the weight quantization done by from_float;
* epilogue_constants — FBGEMM ReQuantizeOutput's fp32 constants
  (torch/include/fbgemm/OutputProcessing-inl.h:76-127, vector form);
* normalize_table / quantize_table / expand_u8 — ToTensor + Normalize (+
  aten quantize_per_tensor) of a raw uint8 image as 3 x 256 tables
  (tests/test_u8_input_cpu.py checks them against torch);
* hist_combine / hist_upscale / hist_param_search / hist_quantization_error and
  HistogramState — HistogramObserver's host half (torch/ao/quantization/
  observer.py:1076-1370).  These are built from torch CPU ops in torch's own
  order: its fp32 sum, cumsum, linspace, bucketize and bincount fix the
  rounding, which a numpy re-derivation would not reproduce.
"""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32
EPS = F32(np.finfo(np.float32).eps)


def qparams_affine(min_val, max_val, qmin=0, qmax=255):
    """quint8 per_tensor_affine: scale = (max+ - min-)/(qmax-qmin) (fp32, >= eps),
    zp = clamp(qmin - rne(min- / scale))."""
    mn = min(F32(min_val), F32(0.0))
    mx = max(F32(max_val), F32(0.0))
    scale = max(F32(F32(mx - mn) / F32(qmax - qmin)), EPS)
    zp = qmin - int(np.rint(F32(mn / scale)))
    return F32(scale), int(min(max(zp, qmin), qmax))


def qparams_symmetric(min_val, max_val):
    """qint8 per_tensor/per_channel_symmetric: scale = max(|min-|, max+)/127.5, zp = 0."""
    mn = np.minimum(np.asarray(min_val, F32), F32(0.0))
    mx = np.maximum(np.asarray(max_val, F32), F32(0.0))
    amax = np.maximum(-mn, mx)
    return np.maximum((amax / F32(127.5)).astype(F32), EPS).astype(F32)


def fold_bn(w, b, mean, var, gamma, beta, eps=1e-5):
    """w' = w * (gamma * rsqrt(var + eps)); b' = (b - mean) * rsqrt * gamma + beta."""
    w = np.asarray(w, F32)
    b = np.zeros(w.shape[0], F32) if b is None else np.asarray(b, F32)
    rsq = (F32(1.0) / np.sqrt((np.asarray(var, F32) + F32(eps)).astype(F32))).astype(F32)
    s = (np.asarray(gamma, F32) * rsq).astype(F32)
    wf = (w * s.reshape((-1,) + (1,) * (w.ndim - 1))).astype(F32)
    bf = ((((b - np.asarray(mean, F32)).astype(F32) * rsq).astype(F32) * np.asarray(gamma, F32)).astype(F32)
          + np.asarray(beta, F32)).astype(F32)
    return wf, bf


def fold_linear_bn(w, b, mean, var, gamma, beta, eps=1e-5):
    """fuse_linear_bn_weights (fusion.py:156-186) — note the different bias order:
    s = gamma * rsqrt(var + eps); w' = w * s; b' = (b - mean) * s + beta."""
    w = np.asarray(w, F32)
    b = np.zeros(w.shape[0], F32) if b is None else np.asarray(b, F32)
    rsq = (F32(1.0) / np.sqrt((np.asarray(var, F32) + F32(eps)).astype(F32))).astype(F32)
    s = (np.asarray(gamma, F32) * rsq).astype(F32)
    wf = (w * s.reshape(-1, 1)).astype(F32)
    bf = (((b - np.asarray(mean, F32)).astype(F32) * s).astype(F32) + np.asarray(beta, F32)).astype(F32)
    return wf, bf


def bn_eval_affine(mean, var, gamma, beta, eps=1e-5):
    """Per-channel (alpha, beta') of an inference BatchNorm in ATen's CPU op
    order (torch 2.10 batch_norm with training=False, probed bit-exact on the
    host): invstd = fp32(1 / sqrt(fp32(var + eps))), alpha = fp32(invstd *
    gamma), beta' = fma(-mean, alpha, beta); then y = fma(x, alpha, beta')."""
    f32 = np.float32
    mean, var = np.asarray(mean, f32), np.asarray(var, f32)
    gamma, beta = np.asarray(gamma, f32), np.asarray(beta, f32)
    invstd = (f32(1.0) / np.sqrt(var + f32(eps))).astype(f32)
    alpha = (invstd * gamma).astype(f32)
    return alpha, fmaf_host(-mean, alpha, beta)


def fmaf_host(a, b, c):
    """fl32(a*b + c) with one rounding, vectorised on the host: a*b is exact
    in float64, the sum rounds once to float64, and when that double lands
    exactly on an fp32 midpoint the TwoSum error term decides the direction
    (the one case where double rounding would differ)."""
    a64 = np.asarray(a, F32).astype(np.float64)
    b64 = np.asarray(b, F32).astype(np.float64)
    c64 = np.asarray(c, F32).astype(np.float64)
    p = a64 * b64
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(F32)
    r64 = r.astype(np.float64)
    diff = s - r64
    nxt = np.nextafter(r, np.where(diff > 0, np.inf, -np.inf).astype(F32))
    mid = (diff != 0) & (s == (r64 + nxt.astype(np.float64)) * 0.5)
    fix = mid & (e != 0) & (np.sign(e) == np.sign(diff))
    return np.where(fix, nxt, r).astype(F32)


def quantize_weight(w, scale):
    """q = clamp(rne(w * fp32(1/s)), -128, 127), per tensor (scalar scale) or per
    output channel (vector scale)."""
    w = np.asarray(w, F32)
    scale = np.asarray(scale, F32)
    if scale.ndim == 0 or scale.size == 1:
        inv = (F32(1.0) / F32(scale.reshape(-1)[0]))
        return np.clip(np.rint((w * inv).astype(F32)), -128, 127).astype(np.int8)
    inv = (F32(1.0) / scale).astype(F32).reshape((-1,) + (1,) * (w.ndim - 1))
    return np.clip(np.rint((w * inv).astype(F32)), -128, 127).astype(np.int8)


def epilogue_constants(s_x, s_w, s_y, bias):
    """(u, v, mult) per output channel for  t = fmaf(u, v, fp32(acc)); ab = t * mult.

    FBGEMM's compiled vector epilogue (requantizeOutputProcessingAvx2 in the torch
    wheel) FMA-contracts the per-tensor bias term with rcp = fp32(1.0f / aws), and
    divides per channel: per-tensor -> (b, rcp); per-channel -> (fp32(b/aws), 1)."""
    s_w = np.atleast_1d(np.asarray(s_w, F32))
    bias = np.asarray(bias, F32)
    aws = (F32(s_x) * s_w).astype(F32)
    mult = (aws / F32(s_y)).astype(F32)
    if aws.size == 1:
        rcp = F32(F32(1.0) / aws[0])
        return bias.copy(), np.full(bias.shape, rcp, F32), np.full(bias.shape, mult[0], F32)
    return (bias / aws).astype(F32), np.ones(bias.shape, F32), mult


def nhwc_flatten_perm(c=256, h=4, w=4):
    """perm such that W_nhwc = W_nchw[:, perm]: fc1 consumes the NHWC-flattened
    pooled tensor while keeping baseline_model.py:78's NCHW flatten semantics."""
    idx = np.arange(c * h * w).reshape(c, h, w)
    return np.ascontiguousarray(np.transpose(idx, (1, 2, 0))).reshape(-1)


# ------------------------------------------------------ raw u8 image input
# ToTensor -> Normalize -> QuantStub of a u8 HWC image is a function of
# (channel, byte): two 3 x 256 tables replace the per-pixel arithmetic, exact
# by construction (tests/test_u8_input_cpu.py checks both against torch).
U8_LAYOUT = "uint8 images are expected as NHWC [N, H, W, 3]"


def normalize_table(mean, std):
    """float32 [3, 256]: tab[c][p] = (fp32(p) / 255 - mean_c) / std_c, with
    torch's fp32 ops in the order ToTensor (div 255) then Normalize (sub, div)."""
    mean = torch.as_tensor(mean, dtype=torch.float32).reshape(3, 1)
    std = torch.as_tensor(std, dtype=torch.float32).reshape(3, 1)
    p = torch.arange(256, dtype=torch.float32).reshape(1, 256).div(255)
    return p.sub(mean).div(std).contiguous()


def quantize_table(tab, scale, zp):
    """uint8 [3, 256]: aten quantize_per_tensor of the normalised table,
    clamp(zp + rint(x * fp32(1 / scale)), 0, 255)."""
    x = np.asarray(tab, F32)
    inv = F32(F32(1.0) / F32(scale))
    q = np.rint((x * inv).astype(F32)).astype(np.int64) + int(zp)
    return torch.from_numpy(np.clip(q, 0, 255).astype(np.uint8))


def check_u8_images(x, hw=None):
    """Raise unless x is a uint8 NHWC image batch [N, H, W, 3] (H = W = hw when
    given).  An NCHW u8 batch is rejected, not guessed at."""
    shape = tuple(x.shape)
    ok = x.dtype == torch.uint8 and len(shape) == 4 and shape[3] == 3
    if ok and hw is not None:
        ok = shape[1:3] == (hw, hw)
    if not ok:
        want = f"[N, {hw}, {hw}, 3]" if hw is not None else "[N, H, W, 3]"
        raise ValueError(f"{U8_LAYOUT}; expected {want}, got {x.dtype} {list(shape)}")


def expand_u8(x, ntab):
    """Host form of the normalize kernel: u8 NHWC [N, H, W, 3] -> fp32 NCHW
    [N, 3, H, W] by indexing ntab (normalize_table); equals ToTensor +
    Normalize of the same bytes bit for bit."""
    check_u8_images(x)
    idx = x.permute(0, 3, 1, 2).long()
    tab = torch.as_tensor(ntab, dtype=torch.float32, device=x.device)
    return torch.stack([tab[c][idx[:, c]] for c in range(3)], dim=1).contiguous()


# ------------------------------------------------------ HistogramObserver (host)
HIST_BINS = 2048        # HistogramObserver's default
HIST_UPSAMPLE = 16      # observer.py:1056-1058
HIST_DST_NBINS = 256    # 2 ** bits of quint8, reduce_range=False (observer.py:1055)


def hist_upscale(histogram, orig_min, orig_max, update_min, update_max, bins=HIST_BINS):
    """_upscale_histogram (observer.py:1194-1233): the old histogram, split
    16-fold, re-binned by its sub-bin midpoints into the new range's bins."""
    histogram = histogram.repeat_interleave(HIST_UPSAMPLE) / HIST_UPSAMPLE
    bin_size = (orig_max - orig_min) / (bins * HIST_UPSAMPLE)
    mid_points = torch.linspace(orig_min, orig_max, bins * HIST_UPSAMPLE + 1)[:-1] + 0.5 * bin_size
    boundaries = torch.linspace(update_min, update_max, bins + 1)
    bucket = torch.bucketize(mid_points, boundaries, right=True) - 1
    bucket[bucket >= bins] = bins - 1
    bucket[bucket < 0] = 0
    return torch.bincount(bucket, weights=histogram, minlength=bins)


def hist_combine(orig_hist, orig_min, orig_max, update_hist, update_min, update_max,
                 bins=HIST_BINS):
    """_combine_histograms (observer.py:1235-1274).  update_hist is already
    binned over [update_min, update_max], which contains [orig_min, orig_max]."""
    if update_min == orig_min and update_max == orig_max:
        return orig_hist + update_hist
    if orig_min == orig_max:   # the old histogram holds one value
        bin_value = torch.sum(orig_hist)
        moved = torch.histc(orig_min, bins=bins, min=update_min, max=update_max) * bin_value
        return moved + update_hist
    if update_min > orig_min or update_max < orig_max:
        raise AssertionError("the updated range must contain the old one")
    return update_hist + hist_upscale(orig_hist, orig_min, orig_max, update_min, update_max, bins)


def _hist_norm(delta_begin, delta_end, density):
    """_get_norm (observer.py:1060-1074): density * (end^3 - begin^3) / 3."""
    norm = (delta_end * delta_end * delta_end - delta_begin * delta_begin * delta_begin) / 3
    return density * norm


def hist_quantization_error(histogram, min_val, max_val, next_start_bin, next_end_bin,
                            bins=HIST_BINS, dst_nbins=HIST_DST_NBINS):
    """_compute_quantization_error (observer.py:1076-1128).  bin_width comes
    from .item() here, so it is a Python double (an fp32 tensor in the search
    below); torch does the same and the rounding depends on it."""
    bin_width = (max_val.item() - min_val.item()) / bins
    dst_bin_width = bin_width * (next_end_bin - next_start_bin + 1) / dst_nbins
    if dst_bin_width == 0.0:
        return 0.0
    src_bin = torch.arange(bins)
    src_bin_begin = (src_bin - next_start_bin) * bin_width
    src_bin_end = src_bin_begin + bin_width
    dst_bin_of_begin = torch.clamp(torch.div(src_bin_begin, dst_bin_width, rounding_mode="floor"),
                                   0, dst_nbins - 1)
    dst_bin_of_begin_center = (dst_bin_of_begin + 0.5) * dst_bin_width
    dst_bin_of_end = torch.clamp(torch.div(src_bin_end, dst_bin_width, rounding_mode="floor"),
                                 0, dst_nbins - 1)
    density = histogram / bin_width
    norm = torch.zeros(bins)
    delta_begin = src_bin_begin - dst_bin_of_begin_center
    delta_end = dst_bin_width / 2
    norm += _hist_norm(delta_begin, torch.ones(bins) * delta_end, density)
    norm += (dst_bin_of_end - dst_bin_of_begin - 1) * _hist_norm(
        torch.tensor(-dst_bin_width / 2), torch.tensor(dst_bin_width / 2), density)
    dst_bin_of_end_center = dst_bin_of_end * dst_bin_width + dst_bin_width / 2
    delta_begin = -dst_bin_width / 2
    delta_end = src_bin_end - dst_bin_of_end_center
    norm += _hist_norm(torch.tensor(delta_begin), delta_end, density)
    return norm.sum().item()


def hist_param_search(histogram, min_val, max_val, bins=HIST_BINS, dst_nbins=HIST_DST_NBINS):
    """_non_linear_param_search (observer.py:1130-1192): shrink the range from
    whichever end frees more bins per 1e-5 quantile step while the L2
    quantization error does not grow.  Returns (new_min, new_max) fp32 tensors."""
    bin_width = (max_val - min_val) / bins
    total = torch.sum(histogram).item()
    c_sum = torch.cumsum(histogram, dim=0)
    stepsize = 1e-5
    alpha, beta = 0.0, 1.0
    start_bin, end_bin = 0, bins - 1
    norm_min = float("inf")
    while alpha < beta:
        next_alpha = alpha + stepsize
        next_beta = beta - stepsize
        l, r = start_bin, end_bin
        while l < end_bin and c_sum[l] < next_alpha * total:
            l = l + 1
        while r > start_bin and c_sum[r] > next_beta * total:
            r = r - 1
        next_start_bin, next_end_bin = start_bin, end_bin
        if (l - start_bin) > (end_bin - r):
            next_start_bin = l
            alpha = next_alpha
        else:
            next_end_bin = r
            beta = next_beta
        if next_start_bin == start_bin and next_end_bin == end_bin:
            continue
        norm = hist_quantization_error(histogram, min_val, max_val, next_start_bin, next_end_bin,
                                       bins, dst_nbins)
        if norm > norm_min:
            break
        norm_min = norm
        start_bin, end_bin = next_start_bin, next_end_bin
    new_min = min_val + bin_width * start_bin
    new_max = min_val + bin_width * (end_bin + 1)
    return new_min, new_max


class HistogramState:
    """The running state of one HistogramObserver(reduce_range=False) on the
    host: fp32 ``histogram`` [bins], ``min_val``, ``max_val`` (0-dim fp32 CPU
    tensors), updated as HistogramObserver.forward does (observer.py:1289-1346)
    from a batch's histogram over the NEW running range.  Whoever owns the
    data (the HIP kernels, or torch.histc on the host) supplies that histogram;
    the running range is min(old, batch min) / max(old, batch max).  Inputs
    holding +-inf or NaN are outside the contract: torch filters inf before
    observing, this does not."""

    def __init__(self, bins=HIST_BINS):
        self.bins = int(bins)
        self.histogram = torch.zeros(self.bins)
        self.min_val = torch.tensor(float("inf"))
        self.max_val = torch.tensor(float("-inf"))

    def initialized(self):
        return not (self.min_val == float("inf") or self.max_val == float("-inf"))

    def update(self, new_min, new_max, update_hist):
        """new_min / new_max: the running range after this batch; update_hist:
        this batch's counts over it (fp32, or integers below 2^24)."""
        new_min = torch.as_tensor(new_min, dtype=torch.float32).reshape(())
        new_max = torch.as_tensor(new_max, dtype=torch.float32).reshape(())
        update_hist = torch.as_tensor(update_hist).to(torch.float32)
        if not self.initialized():                      # reset_histogram (:1276-1287)
            self.histogram = update_hist.clone()
        elif new_min == self.min_val and new_max == self.max_val:
            self.histogram = self.histogram + update_hist
        else:
            self.histogram = hist_combine(self.histogram, self.min_val, self.max_val, update_hist,
                                          new_min, new_max, self.bins)
        self.min_val, self.max_val = new_min.clone(), new_max.clone()

    def observe_host(self, x):
        """HistogramObserver.forward on a host tensor (aminmax + torch.histc)."""
        if x.numel() == 0:
            return
        x = x.detach().to(torch.float32)
        x_min, x_max = torch.aminmax(x)
        new_min, new_max = torch.min(self.min_val, x_min), torch.max(self.max_val, x_max)
        self.update(new_min, new_max, torch.histc(x, self.bins, min=new_min, max=new_max))

    def search(self):
        """(new_min, new_max) of calculate_qparams' search as two np.float32;
        qparams_affine(*search()) is calculate_qparams() (:1348-1370)."""
        if not self.initialized():
            raise ValueError("the observer has seen no data")
        lo, hi = hist_param_search(self.histogram, self.min_val, self.max_val, self.bins)
        return F32(lo.item()), F32(hi.item())
