/*
 * qconvnet.h — C ABI of the MI355X (gfx950) int8 ConvNet inference path.
 *
 * One shared library, libqconvnet.so, built from
 * the HIP sources in convnet-quantization_amd/csrc/.  Every compute entry point:
 *   - takes caller-owned DEVICE pointers (e.g. torch tensors' data_ptr()),
 *     explicit shapes and quantization parameters, and an explicit HIP
 *     stream (hipStream_t passed as void*; NULL = default stream);
 *   - allocates nothing and never synchronizes (safe inside hipGraph capture);
 *   - returns 0 (QCN_OK) or a negative status; no exceptions cross the ABI.
 * The qcn_pack_* functions work on HOST memory (one-time weight packing).
 *
 * The reference (his0si/ConvNet-Quantization) has no FFI: its hot path is the
 * torch.ao / FBGEMM arithmetic behind its duck-typed model objects.  Each entry
 * below names the reference interface it replaces (file:line in
 * /root/reference unless prefixed torch/, which is the torch 2.10 wheel).
 * Numerics are bit-exact with torch.ao's fbgemm engine on the integer path
 * (see oracle/qref.py and tests/golden/).
 */
#ifndef QCONVNET_H
#define QCONVNET_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QCN_OK 0
#define QCN_ERR_ARG (-1)          /* invalid argument / shape                     */
#define QCN_ERR_UNSUPPORTED (-2)  /* shape combination has no kernel              */
#define QCN_ERR_HIP (-3)          /* HIP launch / runtime error                   */

/* Per-layer QDQ hand-off (CustomQuantizedConv2d chain): after requantizing to
 * (scale s1, zero point z1), dequantize, ReLU, and quantize with the next
 * layer's input qparams (inv2 = fp32(1/scale2), z2).  Replaces the fp32
 * DeQuantStub -> F.relu -> [pool] -> QuantStub sequence of
 * models/custom_quantization_model.py:41-45, :237-252. */
typedef struct qcn_qdq_t {
  float s1;
  int32_t z1;
  float inv2;
  int32_t z2;
} qcn_qdq_t;

/* One conv of SimpleConvNet for qcn_convnet_convs_f32_nchw: packed weights
 * (qcn_pack_conv1_weight for conv1, qcn_pack_conv3x3_weight otherwise), the
 * requant constants, the input / output zero points, ReLU and the optional
 * QDQ hand-off into the next layer. */
typedef struct qcn_conv_layer_t {
  const int8_t* w;
  const float* u;
  const float* v;
  const float* mult;
  const int32_t* corr;
  int32_t x_zp;
  int32_t y_zp;
  int32_t relu;
  const qcn_qdq_t* qdq;
} qcn_conv_layer_t;

/* Library version (major*10000 + minor*100 + patch). */
int qcn_version(void);

/* A1 — aten::quantize_per_tensor (QuantStub once converted,
 * models/custom_quantization_model.py:42,55,234):
 *   q = clamp(zp + rne(x * fp32(1/scale)), 0, 255).
 * x is fp32 [n,c,h,w] NCHW; q is u8, NHWC when nhwc_out != 0 else NCHW. */
int qcn_quantize_f32_u8(const float* x, uint8_t* q, int n, int c, int h, int w, int nhwc_out,
                        float scale, int zero_point, void* stream);

/* A7 — aten::dequantize (DeQuantStub, custom_quantization_model.py:44,57,260):
 *   x = fp32(scale) * fp32(q - zp). */
int qcn_dequantize_u8_f32(const uint8_t* q, float* x, long long count, float scale,
                          int zero_point, void* stream);

/* A2 — MinMaxObserver.forward (torch/ao/quantization/observer.py:558-569):
 * running [min, max] of fp32 data, reduced on the device.  minmax points to 2
 * device floats; qcn_minmax_reset writes [+inf, -inf].  Subnormals are kept;
 * a zero result may carry either sign.  NaN input is outside the contract. */
int qcn_minmax_reset(float* minmax, void* stream);
int qcn_minmax_f32(const float* x, long long count, float* minmax, void* stream);

/* HistogramObserver.forward's histogram (torch/ao/quantization/observer.py:
 * 1289-1346; torch.ao's default activation observer, imported by the reference
 * at models/custom_quantization_model.py:5): ADDS the torch.histc(x, bins,
 * min, max) counts of x into hist[bins]; the caller zeroes hist.  minmax
 * points to 2 DEVICE floats, the running [min, max] qcn_minmax_f32 has just
 * updated, so no host round trip sits between the two launches.
 *   bin = min(int(((v - lo) / (hi - lo)) * bins), bins - 1)  for lo <= v <= hi,
 * every operation IEEE fp32 with a correctly rounded division; elements
 * outside the range (and NaN) are skipped; lo == hi counts over [lo - 1,
 * hi + 1]; the reset state [+inf, -inf] counts nothing.
 * Counts are exact integers.  torch.histc accumulates them in fp32 per thread,
 * so a torch bin above 2^24 saturates and depends on the thread count; the
 * two are equal while every bin stays below 2^24.  Inputs holding +-inf are
 * outside the contract (torch's observer filters them first; this does not).
 * bins: a power of two, 16 <= bins <= 4096 (else QCN_ERR_UNSUPPORTED);
 * 0 <= count < 2^32 (count == 0: no launch); x needs only 4-byte alignment. */
int qcn_histc_f32(const float* x, long long count, const float* minmax, int bins,
                  uint32_t* hist, void* stream);

/* A10 — nn.MaxPool2d(2, 2) on u8 NHWC (baseline_model.py:17,25,33). */
int qcn_maxpool2x2_u8_nhwc(const uint8_t* x, int n, int h, int w, int c, uint8_t* y,
                           void* stream);

/* A11 — argmax over the last axis, ties -> lowest index (torch.argmax /
 * topk(1), utils/model_evaluator.py:36,96,160).  +-inf compare as values;
 * NaN input is outside the contract. */
int qcn_argmax_f32(const float* x, int rows, int cols, long long* idx, void* stream);

/* The evaluator's scoring (utils/model_evaluator.py:36-46, 96-102, 160-168):
 * top-1 / top-k hits, per-class totals and correct counts, the confusion
 * matrix and the predictions of fp32 logits [rows, cols] against int64 labels,
 * without the logits leaving the device.
 * Order: NaN above everything and all NaNs equal, -0.0 == +0.0, otherwise the
 * usual order with +-inf as values (torch's for max / argmax / topk).  For a
 * row x with label l:
 *   rank = #{ j : x[j] > x[l]  or  (x[j] == x[l] and j < l) }
 *   top-k hit iff rank < k, top-1 hit iff rank == 0  (a stable descending sort
 *   on ties; torch.topk's tie order is unspecified);
 *   pred = the lowest j whose value is maximal (torch.argmax, NaN included).
 * A label outside [0, cols) makes the row a miss: it is counted in rows and
 * bad_labels and in no class bin or confusion cell.  k > cols is legal (every
 * in-range label hits).
 * int64 counters[qcn_eval_counters_len(cols) = 4 + 2*cols]:
 *   [0] rows seen  [1] top-1 hits  [2] top-k hits  [3] rows with a bad label
 *   [4 .. 4+cols)        per-class total   (indexed by label)
 *   [4+cols .. 4+2cols)  per-class top-1 correct
 * confusion (nullable): int64 [cols][cols], cell [label][pred];
 * pred (nullable): int64 [rows].
 * ADDS into counters and confusion with 64-bit integer atomics (the caller
 * zeroes them once; calls on several streams may share them).  logits need
 * 4-byte alignment only.  QCN_ERR_ARG for a null logits / labels / counters,
 * rows < 0, cols < 1 or k < 1; rows == 0 launches nothing. */
long long qcn_eval_counters_len(int cols);
int qcn_eval_topk_f32(const float* logits, int rows, int cols, const long long* labels, int k,
                      long long* counters, long long* confusion, long long* pred, void* stream);

/* Quantization error of a u8 activation against its fp32 reference, per
 * channel (the reference prints one torch.abs(fp32 - int8).mean() per model,
 * models/static_ptq_model.py:93-95; torch.ao.ns compute_sqnr per tensor).
 * x: fp32 NCHW [n,c,h,w] ([rows,c] is h = w = 1); q: u8 with qparams (scale,
 * zero_point), NHWC when nhwc_q != 0 else NCHW.  Per element, IEEE fp32 with
 * nothing contracted unless it says double:
 *   d = scale * float(int(q) - zp);  lo = scale * float(0 - zp);
 *   hi = scale * float(255 - zp);    e = double(x) - double(d);
 *   qref = clamp(zp + rne(x * fp32(1/scale)), 0, 255)   (qcn_quantize_f32_u8).
 * int64 counts[c][5]: elements, #(x < lo), #(x > hi), #(qref != q), and the
 * fp32 bit pattern of max fabsf(x - d), zero-extended (non-negative floats
 * order as their bits do).  double sums[c][3]: sum double(x)^2, sum e^2,
 * sum |e|.  NaN / +-inf in x are outside the contract.
 * ADDS into counts (64-bit integer atomics) and sums (no floating-point
 * atomics: per-workgroup partials in `workspace`, added in a fixed order by a
 * finishing launch, so the same calls on one stream give the same bits; the
 * caller zeroes counts and sums once; concurrent streams each need their own
 * sums and workspace).  workspace: device memory of
 * qcn_qerror_workspace_size(n,c,h,w) bytes, 8-byte aligned, no initialisation
 * needed; the size is host arithmetic (0 for n == 0, a negative status for a
 * bad shape).  x needs 4-byte alignment, q none (16-byte accesses where both
 * the pointer and the shape allow).  1 <= c <= 65536 and n*h*w < 2^31, else
 * QCN_ERR_UNSUPPORTED; QCN_ERR_ARG for a null pointer, n < 0, c / h / w < 1,
 * zero_point outside [0,255] or a scale that is not finite and positive —
 * checked before any device call; n == 0 launches nothing. */
long long qcn_qerror_workspace_size(int n, int c, int h, int w);
int qcn_qerror_u8_f32(const float* x, const uint8_t* q, int n, int c, int h, int w, int nhwc_q,
                      float scale, int zero_point, long long* counts, double* sums,
                      void* workspace, void* stream);

/* Error of an fp32 activation y against its fp32 reference x, per channel
 * (the fp32 hand-offs of the reference-semantics ResNet: block outputs after
 * the float-domain residual add, the pooled vector).
 * x: fp32 NCHW [n,c,h,w] ([rows,c] is h = w = 1); y: fp32, NHWC when
 * nhwc_y != 0 else NCHW.  Per element, IEEE with nothing contracted:
 *   e = double(x) - double(y).
 * int64 counts[c][3]: elements, #(x != y) (IEEE compare: -0.0 == +0.0), and
 * the fp32 bit pattern of max fabsf(x - y), zero-extended.  double sums[c][4]:
 * sum double(x)^2, sum e^2, sum |e|, sum e (signed: the channel's mean shift).
 * NaN / +-inf are outside the contract.
 * ADDS into counts and sums under qcn_qerror_u8_f32's rules: no floating-point
 * atomics, per-workgroup partials in `workspace`
 * (qcn_qerror_f32_workspace_size(n,c,h,w) bytes, 8-byte aligned, host
 * arithmetic) added in a fixed order by a finishing launch, 64-bit integer
 * atomics for counts; the same calls on one stream give the same bits;
 * concurrent streams each need their own sums and workspace.  x and y need
 * 4-byte alignment (16-byte loads where the pointer and the shape allow).
 * 1 <= c <= 65536 and n*h*w < 2^31, else QCN_ERR_UNSUPPORTED; QCN_ERR_ARG for
 * a null pointer, n < 0 or c / h / w < 1 — checked before any device call;
 * n == 0 launches nothing. */
long long qcn_qerror_f32_workspace_size(int n, int c, int h, int w);
int qcn_qerror_f32_f32(const float* x, const float* y, int n, int c, int h, int w, int nhwc_y,
                       long long* counts, double* sums, void* workspace, void* stream);

/* Resize(R) -> CenterCrop(C) of raw u8 images of mixed sizes (the ImageNet
 * transform, utils/dataset_manager.py:24-25), byte for byte what Pillow's
 * bilinear Image.resize followed by a crop gives.
 * src: one packed device buffer; image i is u8 HWC [h][w][3] at src + offset
 * and is resampled to (oh, ow), of which the window [top, top+ch) x
 * [left, left+cw) is written to y[i] (u8 HWC [ch][cw][3]); only that window
 * is computed.  src, y and the offsets may have any byte alignment.
 * Per axis, `in` samples become `out` samples (IEEE double, nothing
 * contracted; (int) truncates):
 *   scale = in / out;  fs = max(scale, 1.0);  support = 1.0 * fs;  ss = 1.0 / fs
 *   center = (xx + 0.5) * scale
 *   xmin = max((int)(center - support + 0.5), 0)
 *   xmax = min((int)(center + support + 0.5), in)
 *   w[i] = max(0.0, 1.0 - fabs((i + xmin - center + 0.5) * ss)),  i < xmax - xmin
 *   ww = w[0] + w[1] + ...;  k[i] = (int)(0.5 + (w[i] / ww) * 4194304.0)
 *   y[xx] = clamp((sum_i x[xmin + i] * k[i] + (1 << 21)) >> 22, 0, 255)   (int32)
 * The horizontal pass runs first and rounds to u8; the vertical pass reads
 * that u8 image.  Three launches: the tables (computed on the device, in
 * double), the horizontal pass, the vertical pass.
 * desc_host / desc_dev: the same nimg descriptors in host and in device memory
 * (the caller uploads them; desc_dev 8-byte aligned).  The entry reads
 * desc_host only, before any device call: QCN_ERR_ARG for a null pointer,
 * nimg < 0, a non-positive size, a negative offset, a window outside
 * (oh, ow), an image that runs past src_bytes or a workspace that is not
 * 16-byte aligned; QCN_ERR_UNSUPPORTED when ceil(in / out) > 32 on either axis
 * (more than 65 taps).  nimg == 0 launches nothing.
 * workspace: qcn_resize_crop_workspace_size(...) bytes of device memory (host
 * arithmetic; a negative status for a bad descriptor), no initialisation
 * needed; concurrent streams need their own.  It starts with the tables: with
 * S = qcn_resize_crop_tap_stride(...), the int32 record of column j of image
 * i is at index (i * (cw + ch) + j) * S and that of row r at
 * (i * (cw + ch) + cw + r) * S; a record is xmin, the tap count n, then
 * k[0 .. n).  The u8 intermediate image follows the tables. */
typedef struct qcn_resize_img_t {
  long long offset;
  int32_t h, w, oh, ow, top, left;
} qcn_resize_img_t;
long long qcn_resize_crop_workspace_size(const qcn_resize_img_t* desc_host, int nimg, int ch, int cw);
int qcn_resize_crop_tap_stride(const qcn_resize_img_t* desc_host, int nimg, int ch, int cw);
int qcn_resize_crop_u8_hwc(const uint8_t* src, long long src_bytes,
                           const qcn_resize_img_t* desc_host, const qcn_resize_img_t* desc_dev,
                           int nimg, int ch, int cw, uint8_t* y, void* workspace, void* stream);

/* Inference BatchNorm1d (+ReLU) on fp32 [rows, cols] (bn7 of the reference's
 * StaticPTQModel between its dynamic fc1 and fc2, models/static_ptq_model.py:
 * 19-34 over baseline_model.py:80-82): y = fma(x, alpha[c], beta[c]), then
 * max(y, 0) when relu, in ATen's CPU op order (alpha / beta from the host,
 * qconvnet.quant.bn_eval_affine).  cols % 4 == 0, 16-B aligned pointers. */
int qcn_channel_affine_f32(const float* x, int rows, int cols, const float* alpha,
                           const float* beta, int relu, float* y, void* stream);

/* A5/A6 weight packing (host).  w_oihw is torch's s8 [cout][cin][3][3].
 * out receives qcn_conv3x3_packed_size(cin, cout) bytes; wsum[cout] receives
 * sum_k w (for the activation zero-point correction). */
int qcn_conv3x3_packed_size(int cin, int cout);
int qcn_pack_conv3x3_weight(const int8_t* w_oihw, int cout, int cin, int8_t* out, int32_t* wsum);
int qcn_pack_conv1_weight(const int8_t* w_oihw, int cout, int8_t* out, int32_t* wsum);

/* A5/A6/A10 — QuantizedConv2d / QuantizedConvReLU2d (fbgemm), 3x3, pad 1,
 * stride 1, optionally followed by a fused 2x2 max-pool and a per-layer QDQ
 * hand-off (qdq may be NULL).  Replaces the conv of CustomQuantizedConv2d
 * (custom_quantization_model.py:43) and the FX/eager full-int8 conv.
 *   x: u8 NHWC [nimg,h,w,cin] (zero point x_zp);  y: u8 NHWC.
 *   u, v, mult: fp32 [cout] epilogue constants (t = fmaf(u,v,acc); ab = t*mult)
 *   corr: int32 [cout] = (128 - x_zp) * wsum  (activations enter the MFMA as
 *   q - 128). */
int qcn_conv3x3_u8s8_nhwc(const uint8_t* x, int nimg, int h, int w, int cin, int x_zp,
                          const int8_t* w_packed, int cout, const float* u, const float* v,
                          const float* mult, const int32_t* corr, int y_zp, int relu, int pool,
                          const qcn_qdq_t* qdq, uint8_t* y, void* stream);

/* A1 + conv1 .. conv6 of SimpleConvNet (baseline_model.py:60-72; per-layer
 * QDQ form custom_quantization_model.py:233-255) in ONE persistent launch:
 * fp32 NCHW [nimg,3,32,32] in (quantized with in_scale / in_zp ==
 * layers[0].x_zp), conv6's pooled output into a6: chunk-major
 * ([128][nimg][32], the classifier head's input) when kmajor != 0, NHWC
 * [nimg,4,4,256] otherwise; a2 ([nimg,16,16,64]) and a4 ([nimg,8,8,128]) are
 * written on the way.  Each workgroup carries its own
 * images through all six convs, so the results are those of
 * qcn_conv12_fused_f32_nchw + two qcn_conv3x3_pair_u8s8 launches bit for
 * bit.  By batch, with C = the device's CUs:
 *   nimg <= C        one image per workgroup (convnet_convs_sm_kernel);
 *   C < nimg < 4 C   QCN_ERR_UNSUPPORTED (the caller launches the three kernels);
 *   nimg >= 4 C      one persistent workgroup per CU, when conv3..conv6 are all
 *                    on the FBGEMM fast epilogue or all on the one-fma QDQ form
 *                    (else QCN_ERR_UNSUPPORTED).
 * layers[i].x_zp must be conv i-1's output zero point (its QDQ hand-off's z2
 * when it has one): QCN_ERR_ARG otherwise. */
int qcn_convnet_convs_f32_nchw(const float* x, int nimg, float in_scale, int in_zp,
                               const qcn_conv_layer_t* layers, uint8_t* a2, uint8_t* a4, uint8_t* a6,
                               int kmajor, void* stream);

/* A5+A6+A10 x4 — conv3 .. conv6 of SimpleConvNet (baseline_model.py:20-33,
 * :64-75) in one persistent launch of 256-thread workgroups (one wave per
 * SIMD, 64-cout x 256-pixel wave tiles, r06): a2 u8 NHWC [nimg,16,16,64] in
 * (qcn_conv12_fused_f32_nchw's output), a4 ([nimg,8,8,128]) written on the
 * way, conv6's pooled output into a6 as qcn_convnet_convs_f32_nchw writes it
 * (chunk-major when kmajor).  layers: the four layers conv3 .. conv6
 * (layers[0].x_zp = conv2's output zero point).  Bit-exact with the pair
 * launches.  QCN_ERR_UNSUPPORTED unless conv3..conv6 are all on the FBGEMM
 * fast epilogue or all on the one-fma QDQ form. */
int qcn_convs36_u8s8(const uint8_t* a2, int nimg, const qcn_conv_layer_t* layers, uint8_t* a4, uint8_t* a6,
                     int kmajor, void* stream);

/* Host query (no launch): which form qcn_convnet_convs_f32_nchw takes for
 * these arguments on the current device — 1 one image per workgroup, 2 the
 * persistent form, or the error it would return (QCN_ERR_UNSUPPORTED,
 * QCN_ERR_ARG, QCN_ERR_HIP). */
int qcn_convnet_convs_form(int nimg, float in_scale, int in_zp, const qcn_conv_layer_t* layers, int kmajor);

/* A1+A5+A6 fused — QuantStub + conv1(+ReLU) of SimpleConvNet
 * (baseline_model.py:13, :60): fp32 NCHW [nimg,3,hw,hw] in, quantized with
 * (in_scale, in_zp), 3x3 conv to 64 channels, u8 NHWC out.  q_in (optional,
 * may be NULL) receives the quantized input, u8 NHWC. */
int qcn_conv1_f32_nchw(const float* x, int nimg, int hw, float in_scale, int in_zp,
                       const int8_t* w1_packed, const float* u, const float* v, const float* mult,
                       const int32_t* corr, int y_zp, int relu, const qcn_qdq_t* qdq, uint8_t* y,
                       uint8_t* q_in, void* stream);

/* A1+A5+A6+A10 fused — QuantStub + conv1(+ReLU) + conv2(+ReLU) + 2x2 max-pool
 * of SimpleConvNet's first block (baseline_model.py:13-18, :60-63): fp32 NCHW
 * [nimg,3,32,32] in, u8 NHWC [nimg,16,16,64] out; conv1's activation stays in
 * LDS.  Parameters as qcn_conv1_f32_nchw (conv1: z1 = its output zero point,
 * qdq1 its optional hand-off) and qcn_conv3x3_u8s8_nhwc (conv2: x2_zp = its
 * input zero point). */
int qcn_conv12_fused_f32_nchw(const float* x, int nimg, float in_scale, int in_zp,
                              const int8_t* w1_packed, const float* u1, const float* v1,
                              const float* mult1, const int32_t* corr1, int z1, int relu1,
                              const qcn_qdq_t* qdq1, int x2_zp, const int8_t* w2_packed,
                              const float* u2, const float* v2, const float* mult2,
                              const int32_t* corr2, int y_zp, int relu2, const qcn_qdq_t* qdq2,
                              uint8_t* y, void* stream);

/* ---- raw u8 image input ------------------------------------------------
 * ToTensor -> Normalize(mean, std) -> QuantStub is a function of (channel,
 * byte), so a u8 HWC image needs two tables of [3][256] entries (built on the
 * host, qconvnet/quant.py normalize_table / quantize_table; device memory
 * here): ntab, the normalised fp32 value of byte p in channel c, and qlut, its
 * quantize_per_tensor(in_scale, in_zp).  Exact by construction.
 *
 * General fallback: u8 NHWC [n,h,w,3] -> fp32 NCHW [n,3,h,w],
 * x = ntab[c][img].  Any h, w and any byte alignment of img. */
int qcn_u8img_normalize_f32_nchw(const uint8_t* img, int n, int h, int w, const float* ntab,
                                 float* x, void* stream);

/* qcn_conv12_fused_f32_nchw on raw images: img u8 NHWC [nimg,32,32,3] (4-byte
 * aligned, QCN_ERR_ARG otherwise), the QuantStub by lookups in qlut while the
 * window is staged.  The remaining arguments and the result are those of
 * qcn_conv12_fused_f32_nchw fed with ntab[c][img]. */
int qcn_conv12_fused_u8_nhwc(const uint8_t* img, int nimg, const uint8_t* qlut, int in_zp,
                             const int8_t* w1_packed, const float* u1, const float* v1,
                             const float* mult1, const int32_t* corr1, int z1, int relu1,
                             const qcn_qdq_t* qdq1, int x2_zp, const int8_t* w2_packed,
                             const float* u2, const float* v2, const float* mult2,
                             const int32_t* corr2, int y_zp, int relu2, const qcn_qdq_t* qdq2,
                             uint8_t* y, void* stream);

/* qcn_convnet_convs_f32_nchw on raw images (img, qlut as above; in_zp ==
 * layers[0].x_zp): the same forms by batch, the same planning
 * (qcn_convnet_convs_form answers for both input kinds) and the same bytes in
 * a2, a4 and a6. */
int qcn_convnet_convs_u8_nhwc(const uint8_t* img, int nimg, const uint8_t* qlut, int in_zp,
                              const qcn_conv_layer_t* layers, uint8_t* a2, uint8_t* a4, uint8_t* a6,
                              int kmajor, void* stream);

/* qcn_resnet_stem_fused on raw images: img u8 NHWC [nimg,h,w,3] and qlut (both
 * 4-byte aligned, QCN_ERR_ARG otherwise); the QuantStub is a byte-wise lookup
 * of each image row while the band is staged, so the data loader's ToTensor ->
 * Normalize (dataset_manager.py:41-44) and the QuantStub ahead of conv1
 * (custom_quantization_model.py:127) cost no launch and no fp32 copy of the
 * batch; replaces qcn_u8img_normalize_f32_nchw + qcn_resnet_stem_fused.
 * The remaining arguments, the envelope (h == w in {224, 64}, cout == 64, else
 * QCN_ERR_UNSUPPORTED) and the result are those of qcn_resnet_stem_fused fed
 * with ntab[c][img]. */
int qcn_resnet_stem_fused_u8_nhwc(const uint8_t* img, int nimg, int h, int w, const uint8_t* qlut,
                                  int in_zp, const int8_t* w_packed, int cout, const float* u,
                                  const float* v, const float* mult, const int32_t* corr,
                                  int y_zp, int relu, uint8_t* y, void* stream);

/* qcn_stem_pack_f32_nchw on raw images (the general stem fallback): QuantStub
 * + row im2col, y[n][h][ow][32] byte 3*s+ch = qlut[ch][img[n][iy][2*ox-3+s][ch]],
 * zp outside the image and in bytes 21..31; ow = (w-1)/2 + 1.  Any h, w and
 * any byte alignment of img; y 16-byte aligned.  The bytes are those of
 * qcn_stem_pack_f32_nchw fed with ntab[c][img]. */
int qcn_stem_pack_u8_nhwc(const uint8_t* img, int nimg, int h, int w, const uint8_t* qlut, int zp,
                          uint8_t* y, void* stream);

/* Two convolutions of one SimpleConvNet block in one launch: conv A
 * (cin -> cmid, no pool) then conv B (cmid -> cout, fused 2x2 max-pool).  A's
 * output never leaves LDS; the results are those of two qcn_conv3x3_u8s8_nhwc
 * calls (A's u8 output zero point zmid is B's input zero point, or qdqa->z2 in
 * QDQ mode; qdqa / qdqb may be NULL).  y: u8 NHWC [nimg, hw/2, hw/2, cout], or chunk-major like
 * qcn_conv3x3_u8s8_kmajor when kmajor != 0.  Supported: (hw 16, 64 -> 128 ->
 * 128) and (hw 8, 128 -> 256 -> 256) — SimpleConvNet conv3+conv4 and
 * conv5+conv6; QCN_ERR_UNSUPPORTED otherwise. */
int qcn_conv3x3_pair_u8s8(const uint8_t* x, int nimg, int hw, int cin, int x_zp,
                          const int8_t* wa_packed, int cmid, const float* ua, const float* va,
                          const float* multa, const int32_t* corra, int zmid, int relua,
                          const qcn_qdq_t* qdqa, const int8_t* wb_packed, int cout, const float* ub,
                          const float* vb, const float* multb, const int32_t* corrb, int y_zp,
                          int relub, const qcn_qdq_t* qdqb, int kmajor, uint8_t* y, void* stream);

/* A5/A6 as above, but y is written chunk-major for the classifier head:
 * y[f / 32][nimg][32] with f the NHWC flatten index of one image's output
 * (oh * ow * cout bytes).  Supported: the 8x8 layers with cout == 256
 * (SimpleConvNet conv5/conv6), QCN_ERR_UNSUPPORTED otherwise. */
int qcn_conv3x3_u8s8_kmajor(const uint8_t* x, int nimg, int h, int w, int cin, int x_zp,
                            const int8_t* w_packed, int cout, const float* u, const float* v,
                            const float* mult, const int32_t* corr, int y_zp, int relu, int pool,
                            uint8_t* y, void* stream);

/* A9 — quantized Linear / LinearReLU (fbgemm), static qparams:
 * fc1/fc2 of SimpleConvNet (baseline_model.py:38,40).
 *   x: u8 [m,k] (zero point x_zp); w: s8 [n,k] row-major; y: u8 [m,n].
 *   y_deq (optional) receives fp32 (y - y_zp) * y_scale  (DeQuantStub). */
int qcn_linear_u8s8(const uint8_t* x, int m, int k, int x_zp, const int8_t* w, int n,
                    const float* u, const float* v, const float* mult, const int32_t* corr,
                    int y_zp, int relu, uint8_t* y, float* y_deq, float y_scale, void* stream);

/* A9 x 2 + A7 — the static classifier head in two launches: fc1 (+ReLU)
 * u8 x s8 -> u8 [m, n1] as a split-K GEMM (2 partial planes from 1024 rows
 * up, 4 below) into an int32 workspace, then
 * one wave per row finishes fc1 (requant) and computes fc2 (n2 <= 16) and its
 * DeQuantStub.  Same results as qcn_linear_u8s8(fc1) followed by
 * qcn_linear_u8s8(fc2, y_deq) — fc2's input zero point is y1_zp, fc2's
 * correction is applied exactly in the finisher (no corr2 argument).
 * x and w1 are CHUNK-MAJOR: x[k/32][m][32] (qcn_conv3x3_u8s8_kmajor writes
 * conv6's output that way), w1[k/32][n1][32] (qcn_pack_fc_kmajor).
 * corr1 = (128 - x_zp) * sum_k w1[f][k].  Supported: m % 128 == 0, n1 == 512,
 * k % 1024 == 0, n2 <= 16 (QCN_ERR_UNSUPPORTED otherwise).  workspace: device
 * memory of qcn_classifier_workspace_size(m, n1) bytes (the int32 split-K
 * partials; no initialisation needed); one workspace per stream the head runs
 * on concurrently. */
long long qcn_classifier_workspace_size(int m, int n1);
/* Host: s8 [n][k] row-major -> [k/32][n][32] (k % 32 == 0). */
int qcn_pack_fc_kmajor(const int8_t* w, int n, int k, int8_t* out);
/* Host: the QDQ hand-off (qcn_qdq_t) after a requant to (y_zp, lo) in its
 * one-fma form.  With r = rint(ab) of the requant, the layer output is
 * q1 = clamp(r + y_zp, lo, 255) and the next stub's input g(q1); on success
 * (returns 1) out[4] = {qa, qb, glo, ghi} with
 *   g(clamp(r + y_zp, lo, 255)) == rne_sat_u8(med3(fma(r, qa, qb), glo, ghi))
 * for every integer r (checked in fp32 over all r with q1 in [lo, 255]);
 * returns 0 when no exact form was found (the conv epilogues then run the
 * general requant + qdq sequence).  The conv launchers apply it themselves;
 * exported for the host tests (no device work). */
int qcn_qdq_affine(const qcn_qdq_t* q, int y_zp, int lo, float* out);
/* Host: the fused residual join of the ResNet bottleneck (out zero point 0,
 * custom_quantization_model.py:94-101) in its one form: on success (returns
 * 1) out[3] = {a, b, c} with
 *   sat(rne(((y - y_zp) y_scale + (r - r_zp) r_scale) * fp32(1/out_scale)))
 *     == sat(rne(fma(y, a, fma(r, b, c))))
 * for all 256 x 256 byte pairs (y, r) in the kernel's fp32 op order; 0 when
 * no exact form was found (the streaming kernel then keeps the sequence).
 * Applied by qcn_conv_gemm_u8s8_nhwc itself; exported for the host tests. */
int qcn_join_affine(float y_scale, int y_zp, float r_scale, int r_zp, float out_scale, float* out);
int qcn_classifier_u8s8(const uint8_t* x, int m, int k, const int8_t* w1, int n1, const float* u1,
                        const float* v1, const float* mult1, const int32_t* corr1, int y1_zp,
                        int relu1, const int8_t* w2, int n2, const float* u2, const float* v2,
                        const float* mult2, int y2_zp, int relu2, float y2_scale, void* workspace,
                        uint8_t* y1, uint8_t* y2, float* y2_deq, void* stream);

/* QDQ classifier head (CustomQuantizedSimpleConvNet, BASELINE config 2;
 * custom_quantization_model.py:218-219, 256-258): fc1's QuantStub -> int8
 * Linear -> requant to (y1_scale, y1_zp) (no ReLU in the int8 op) ->
 * DeQuantStub -> F.relu (fp32) -> fc2 as an fp32 nn.Linear (w2 fp32 [n2][n1],
 * b2 fp32 [n2] or NULL) -> y2 fp32 [m][n2].  y1 (optional) receives fc1's u8
 * output.  Same split-K first launch, layouts, envelope and workspace as
 * qcn_classifier_u8s8; fc2's fp32 sums run in a different order from a CPU
 * sgemm (the QDQ tests bound the difference). */
int qcn_classifier_qdq_u8s8(const uint8_t* x, int m, int k, const int8_t* w1, int n1,
                            const float* u1, const float* v1, const float* mult1,
                            const int32_t* corr1, int y1_zp, float y1_scale, const float* w2,
                            int n2, const float* b2, void* workspace, uint8_t* y1, float* y2,
                            void* stream);

/* A8 — quantized::linear_dynamic (DynamicQuantizedLinear of
 * models/static_ptq_model.py:28-32 and models/dynamic_ptq_model.py:302-306):
 * per-call activation qparams from the batch min/max (ChooseQuantizationParams,
 * qrange [0,127] when reduce_range), quantize, u8 x s8 GEMM,
 * y = fmaf(fp32(acc), fp32(s_x * s_w), bias).  w_scale holds 1 (per-tensor) or
 * n (per-channel) floats; bias may be NULL.  workspace: >= 64 bytes of device
 * memory + m*k bytes (quantized activations). */
long long qcn_linear_dynamic_workspace_size(int m, int k);
int qcn_linear_dynamic_f32(const float* x, int m, int k, const int8_t* w, int n,
                           const float* w_scale, int per_channel, const int32_t* wsum,
                           const float* bias, int reduce_range, float* y, void* workspace,
                           void* stream);

/* A8 with the activation range supplied by the caller: minmax points to 2
 * device floats [min, max] — e.g. the all-reduced range of every rank's shard,
 * which makes a sharded dynamic Linear batch-exact.  Otherwise
 * identical to qcn_linear_dynamic_f32. */
int qcn_linear_dynamic_range_f32(const float* x, int m, int k, const int8_t* w, int n,
                                 const float* w_scale, int per_channel, const int32_t* wsum,
                                 const float* bias, int reduce_range, const float* minmax,
                                 float* y, void* workspace, void* stream);

/* A8 with per-sample activation qparams: every row of x is quantized with the
 * ChooseQuantizationParams of its own min/max, so row i of y is bit for bit
 * qcn_linear_dynamic_f32 applied to x[i] alone ([1][k]) — an image's result
 * does not depend on its batch, and a sharded batch needs no collective.
 * Two launches (row min/max + qparams + quantize; GEMM with a per-row
 * epilogue).  Other arguments as qcn_linear_dynamic_f32.  workspace: device
 * memory, 16-byte aligned, qcn_linear_dynamic_rows_workspace_size(m, k) =
 * roundup64(16 * m) + m * k bytes, laid out as
 *   [0, 16 * m)                 one record per row: float scale, float 1/scale,
 *                               float zero_point, int32 zero_point;
 *   [roundup64(16 * m), + m*k)  the u8 activations, row-major;
 * after the call a caller can read each row's scale and zero point there.
 * NULL x, w, w_scale, wsum, y or workspace, or m, k or n <= 0: QCN_ERR_ARG,
 * nothing launched. */
long long qcn_linear_dynamic_rows_workspace_size(int m, int k);
int qcn_linear_dynamic_rows_f32(const float* x, int m, int k, const int8_t* w, int n,
                                const float* w_scale, int per_channel, const int32_t* wsum,
                                const float* bias, int reduce_range, float* y, void* workspace,
                                void* stream);

/* fp32 Linear (fc2 of CustomQuantizedSimpleConvNet stays fp32,
 * custom_quantization_model.py:219): y = x @ w^T + b, with optional ReLU on x
 * (relu_in) applied on load. */
int qcn_linear_f32(const float* x, int m, int k, const float* w, int n, const float* b,
                   int relu_in, float* y, void* stream);

/* ---- ResNet-style bottleneck blocks (config 5) ----------
 * CustomQuantizedBottleneck / CustomQuantizedResNet50
 * (models/custom_quantization_model.py:60-148): 1x1, 3x3 (strided) and 1x1
 * downsample convs, the fp32-domain residual add + ReLU (:94-101), the stem
 * conv + maxpool, the global average pool and the fc classifier. */

/* Host: s8 OIHW [cout][cin][kh][kw] -> chunk-major [kh*kw*cin/32][cout][32]
 * (K ordered (r, s, c)); wsum[cout] = sum of each filter.  cin % 32 == 0. */
int qcn_pack_conv_weight_kmajor(const int8_t* w_oihw, int cout, int cin, int kh, int kw,
                                int8_t* out, int32_t* wsum);
/* Quantized Conv2d(+ReLU) (QuantizedConv2d / QuantizedConvReLU2d with
 * per-channel or per-tensor weights) on u8 NHWC, any kernel / stride /
 * padding; requant as qcn_conv3x3_u8s8_nhwc (A6).  cin % 32 == 0,
 * cout % 64 == 0; corr = (128 - x_zp) * wsum.  Output [n][oh][ow][cout]. */
int qcn_conv_u8s8_nhwc(const uint8_t* x, int nimg, int h, int w, int cin, int x_zp,
                       const int8_t* w_packed, int cout, int kh, int kw, int stride_h,
                       int stride_w, int pad_h, int pad_w, const float* u, const float* v,
                       const float* mult, const int32_t* corr, int y_zp, int relu, uint8_t* y,
                       void* stream);
/* Same conv as qcn_conv_u8s8_nhwc on the LDS-tiled implicit-GEMM kernel
 * (256-pixel x 128/64-channel tiles, LDS-DMA im2col).  With resid != NULL the
 * residual join is fused into the epilogue (the conv must have relu == 0):
 * y3 = requant(acc) with (y_scale, y_zp), then
 * y = quantize(relu(y_scale*(y3-y_zp) + r_scale*(resid-r_zp)), out_scale, out_zp)
 * — bit-identical to qcn_conv_u8s8_nhwc followed by qcn_add_relu_u8. */
int qcn_conv_gemm_u8s8_nhwc(const uint8_t* x, int nimg, int h, int w, int cin, int x_zp,
                            const int8_t* w_packed, int cout, int kh, int kw, int stride_h,
                            int stride_w, int pad_h, int pad_w, const float* u, const float* v,
                            const float* mult, const int32_t* corr, int y_zp, int relu,
                            const uint8_t* resid, float y_scale, float r_scale, int r_zp,
                            float out_scale, int out_zp, uint8_t* y, void* stream);
/* The bottleneck's expand + residual join (qcn_conv_gemm_u8s8_nhwc with
 * resid, 1x1, cin 64 -> cout 256) with the NEXT block's reduce conv (1x1,
 * stride 1, 256 -> cout2 in {64, 128}, input zero point out_zp) fused: y is
 * the joined block output (u8 NHWC [n][h][w][256], the next identity), y2 the
 * reduce's output [n][h][w][cout2] (FBGEMM requant with u2/v2/mult2/corr2,
 * y2_zp, relu2).  Bit-identical to the two separate launches; replaces
 * custom_quantization_model.py:89-101 of block i followed by :81-83 (conv1,
 * bn1, relu) of block i + 1.  QCN_ERR_UNSUPPORTED for other shapes. */
int qcn_conv1x1_join_reduce_u8s8_nhwc(const uint8_t* x, int nimg, int h, int w, int cin, int x_zp,
                                      const int8_t* w_packed, int cout, const float* u, const float* v,
                                      const float* mult, const int32_t* corr, int y_zp, const uint8_t* resid,
                                      float y_scale, float r_scale, int r_zp, float out_scale, int out_zp,
                                      uint8_t* y, const int8_t* w2_packed, int cout2, const float* u2,
                                      const float* v2, const float* mult2, const int32_t* corr2, int y2_zp,
                                      int relu2, uint8_t* y2, void* stream);
/* What qcn_conv_gemm_u8s8_nhwc / qcn_conv1x1_join_reduce_u8s8_nhwc launch for
 * a set of arguments (qcn_conv_gemm_form, qcn_conv1x1_join_reduce_form). */
#define QCN_CONV_STREAM 1       /* conv1x1_stream_kernel, stride 1                */
#define QCN_CONV_STREAM_S2 2    /* conv1x1_stream_kernel, the stride-2 downsample */
#define QCN_CONV_JOIN_REDUCE 3  /* conv1x1_stream_kernel with the fused reduce    */
#define QCN_CONV_IMG 4          /* conv3x3_img_kernel (whole image per workgroup) */
#define QCN_CONV_TILED 5        /* conv_gemm_kernel (256-pixel tiles)             */
typedef struct qcn_conv_form_t {
  int32_t family; /* QCN_CONV_*                                                    */
  int32_t bn;     /* tiled: output channels per workgroup (64 / 128 / 256), else 0 */
  int32_t nw;     /* waves per workgroup                                           */
  int32_t rq;     /* requant form: 0 z_y == 0 and no ReLU floor (the saturating
                     pack alone), 1 no ReLU floor (rint + z_y, saturating pack),
                     2 the general clamp; the tiled kernel's three branches in the
                     same order (0 also with ReLU: the floor is 0 there); the
                     whole-image kernel has the general clamp only                 */
  int32_t zo;     /* join form: 0 out_zp != 0, 1 out_zp == 0, 2 out_zp == 0 in the
                     one-fma form (qcn_join_affine; streaming families only);
                     -1 without a join                                             */
  int32_t k;      /* streaming families: the compiled-in K, else 0                 */
  int32_t p;      /* streaming families: prefetch ring depth in strips, else 0     */
  int32_t bl;     /* streaming families: 1 activations through the LDS ring        */
  int32_t cr;     /* fused reduce: its output channels, else 0                     */
  int32_t nstrip; /* streaming families: 32-pixel strips, else 0                   */
  int32_t nchunk; /* streaming families: chunks (workgroups per channel group) and */
  int32_t per;    /*   strips per chunk; both -1 when asked without the device     */
} qcn_conv_form_t;
/* Host query (no launch, no tensors): the form qcn_conv_gemm_u8s8_nhwc takes
 * for these shape and quantization arguments (has_resid: whether resid would
 * be non-NULL).  It runs the launch's own argument checks and dispatch with
 * the launchers recording instead of launching, so it returns what the launch
 * would return before any device work (QCN_OK and *form filled, or
 * QCN_ERR_ARG / QCN_ERR_UNSUPPORTED).  use_device == 0: no HIP call is made
 * and nchunk / per, which depend on the device's CU count and the kernel's
 * occupancy, are -1; otherwise they are those of the current device
 * (QCN_ERR_HIP without one). */
int qcn_conv_gemm_form(int nimg, int h, int w, int cin, int x_zp, int cout, int kh, int kw, int stride_h,
                       int stride_w, int pad_h, int pad_w, int y_zp, int relu, int has_resid, float y_scale,
                       float r_scale, int r_zp, float out_scale, int out_zp, int use_device,
                       qcn_conv_form_t* form);
/* The same for qcn_conv1x1_join_reduce_u8s8_nhwc. */
int qcn_conv1x1_join_reduce_form(int nimg, int h, int w, int cin, int x_zp, int cout, int y_zp, float y_scale,
                                 float r_scale, int r_zp, float out_scale, int out_zp, int cout2, int y2_zp,
                                 int relu2, int use_device, qcn_conv_form_t* form);
/* Residual join (custom_quantization_model.py:94-101 then the next stage's
 * QuantStub): y = quantize(relu?(fp32(sa*(a-za)) + fp32(sb*(b-zb))), s_out, z_out).
 * Any byte alignment: 16-byte accesses when a, b and y are all 16-byte
 * aligned, an element-wise path otherwise (same results). */
int qcn_add_relu_u8(const uint8_t* a, float sa, int za, const uint8_t* b, float sb, int zb,
                    long long count, float s_out, int z_out, int relu, uint8_t* y, void* stream);
/* nn.MaxPool2d(3, 2, padding=1) on u8 NHWC (c % 16 == 0, else
 * QCN_ERR_UNSUPPORTED).  Any byte alignment: 16-byte accesses when x and y
 * are 16-byte aligned, a byte-wise kernel otherwise (same results). */
int qcn_maxpool3x3s2_u8_nhwc(const uint8_t* x, int nimg, int h, int w, int c, uint8_t* y,
                             void* stream);
/* QuantStub on fp32 NCHW [n][3][h][w] fused with the row im2col of the 7x7 /
 * stride-2 / pad-3 stem: y[n][h][ow][32], byte 3*s+ch = q(x[n][ch][iy][2*ox-3+s]),
 * zero point outside the image and in bytes 21..31.  ow = (w-1)/2 + 1. */
int qcn_stem_pack_f32_nchw(const float* x, int nimg, int h, int w, float scale, int zp, uint8_t* y,
                           void* stream);
/* The whole ResNet stem in one launch: QuantStub (scale, zp) on fp32 NCHW
 * [n][3][h][w] -> 7x7/2 pad-3 conv 3->64 (w_packed = stem_weight_rows packed
 * k-major, [7][64][32]; u/v/mult/corr and y_zp/relu as qcn_conv_gemm_u8s8_nhwc)
 * -> MaxPool2d(3, 2, padding=1) -> u8 NHWC [n][h/4][w/4][64].  Bit-identical
 * to qcn_stem_pack_f32_nchw + qcn_conv_gemm_u8s8_nhwc (7x1, strides (2,1), pad
 * (3,0)) + qcn_maxpool3x3s2_u8_nhwc; replaces the reference's
 * conv1/bn1/relu/maxpool of custom_quantization_model.py:117-141 after its
 * QuantStub.  h == w in {224, 64}, cout == 64, else QCN_ERR_UNSUPPORTED. */
int qcn_resnet_stem_fused(const float* x, int nimg, int h, int w, float scale, int zp,
                          const int8_t* w_packed, int cout, const float* u, const float* v,
                          const float* mult, const int32_t* corr, int y_zp, int relu, uint8_t* y,
                          void* stream);
/* AdaptiveAvgPool2d(1) on u8 NHWC [nimg][hw][c] -> [nimg][c], quantization
 * parameters kept (torch's quantized adaptive_avg_pool2d, the avgpool of a
 * static-int8 ResNet ahead of its fc): y = clamp(x_zp + rne(fp32(sum_q -
 * hw*x_zp) * fp32(1/hw)), 0, 255).  c % 4 == 0. */
int qcn_avgpool_u8_nhwc(const uint8_t* x, int nimg, int hw, int c, int x_zp, uint8_t* y,
                        void* stream);

/* ---- SURVEY §8(f)2 in the reference's own semantics ----------------------
 * CustomQuantizedBottleneck / CustomQuantizedResNet50 with live per-layer
 * stubs (models/custom_quantization_model.py:34-45, 60-143): fp32 BN / ReLU /
 * max-pool / residual add / avg-pool between int8 convs
 * (qcn_conv_gemm_u8s8_nhwc, requant to each conv's own output qparams, no
 * ReLU).  All maps NHWC, C % 4 == 0; alpha / beta are BN's eval constants
 * (ATen: alpha = fp32(fp32(1/sqrt(var+eps)) * gamma), beta = fmaf(-mean,
 * alpha, bias); the map is fmaf(x, alpha, beta)); every quantize is
 * zp + rint(x * fp32(1/s)) clamped to [0, 255]; ReLU keeps -0.0 (torch.relu).
 * Pointers: u8 4-B aligned, fp32 maps and alpha / beta 16-B aligned. */
/* conv -> DeQuantStub -> BN -> [ReLU] -> next conv's QuantStub (u8 -> u8). */
int qcn_dq_bn_q_u8(const uint8_t* y, long long count, int c, float s, int z, const float* alpha,
                   const float* beta, int relu, float s_next, int z_next, uint8_t* out,
                   void* stream);
/* Stem: conv -> DeQuantStub -> BN -> ReLU -> MaxPool2d(3, 2, 1): fp32
 * [n][(h-1)/2+1][(w-1)/2+1][c] (the first block's input and identity), plus,
 * when out_q is not NULL, that map quantized for block 0's QuantStubs. */
int qcn_dq_bn_relu_maxpool_f32(const uint8_t* y, int n, int h, int w, int c, float s, int z,
                               const float* alpha, const float* beta, float* out, float s_next,
                               int z_next, uint8_t* out_q, void* stream);
/* Residual join (:92-101): out = relu(bn3(dq(y3)) + identity), identity =
 * bn_d(dq(yd)) (downsample conv, yd != NULL) or the fp32 block input idf;
 * fp32 out, plus out_q (optional) quantized for the next block's stubs. */
int qcn_qdq_join_f32(const uint8_t* y3, float s3, int z3, const float* a3, const float* b3,
                     const uint8_t* yd, float sd, int zd, const float* ad, const float* bd,
                     const float* idf, long long count, int c, float* out, float s_next, int z_next,
                     uint8_t* out_q, void* stream);
/* AdaptiveAvgPool2d(1) on fp32 NHWC -> [n][c]: the fp32 sum over the window
 * in the order of ATen's CPU sum kernel (mean over H, W of a channels-last
 * map: row-major, 16 pixels at a time into the lowest of four cascade
 * levels, 2^(ceil_log2(h*w)/4) at a time once that exceeds 16; the plain
 * sequential sum up to 16 pixels), then / (h*w).  Bit-equal to torch on the CPU where ATen
 * reduces whole 4-vector column blocks (c % 64 == 0 covers AVX2 and AVX-512);
 * narrower column remainders take an interleaved order there that depends on
 * the host's vector width and is not reproduced. */
int qcn_avgpool_f32_nhwc(const float* x, int n, int h, int w, int c, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* QCONVNET_H */
