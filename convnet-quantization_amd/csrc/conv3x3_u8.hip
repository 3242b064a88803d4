// Raw u8 NHWC image input for the conv1+conv2 phase: the u8 twins of
// conv12p_kernel and of the one-launch conv1..conv6 kernels, in a translation
// unit of their own (conv3x3.hip's compile time stays where it was and its
// fp32 kernels are built from the same text as before).
//
// ToTensor -> Normalize -> quantize_per_tensor is a function of (channel,
// byte): the host builds its 3 x 256 table (qconvnet/quant.py quantize_table)
// and conv12p_body<uint8_t> stages the input window by lookups in a copy of it
// in LDS (conv3x3.hip, 'Window staging').  Everything after the window — conv1,
// conv2, the pair phases — is the fp32-input code, so the outputs equal those
// of the fp32 entries fed with the table-expanded image bit for bit.
#define QCN_CONV_U8_TU 1
#define QCN_NO_ABI 1
#include "conv3x3.hip"

namespace qcn {

// the conv12 phase also holds the QuantStub table
constexpr int kConvnet16LdsU8 = cmax(Conv12P::LDS_U8, kConvnet16Lds);
constexpr int kConvnetSmLdsU8 = cmax(Conv12P::LDS_U8, kConvnetSmLds);

__global__ __launch_bounds__(512, 1)
void conv12p_u8_kernel(const uint8_t* __restrict__ img, int nimg, const uint8_t* __restrict__ qlut,
                       int in_zp, const int8_t* __restrict__ w1, ConvEpi ep1, int x2_zp,
                       const int8_t* __restrict__ w2, ConvEpi ep2, uint8_t* __restrict__ y) {
  const int T = (int)blockIdx.x < nimg ? 2 * ((nimg - 1 - (int)blockIdx.x) / (int)gridDim.x + 1) : 0;
  conv12p_body((int)blockIdx.x, (int)gridDim.x, T, img, nimg, 0.0f, in_zp, w1, ep1, x2_zp, w2, ep2, y,
               qlut);
}

// convnet_convs16_kernel with the u8 conv12 phase (the pair phases read a2 /
// a4 as before)
template <int EM, bool KMAJOR>
__global__ __launch_bounds__(512, 1)
void convnet_convs16_u8_kernel(const uint8_t* __restrict__ img, int nimg,
                               const uint8_t* __restrict__ qlut, QCN_C16_PARAMS,
                               uint8_t* __restrict__ a2, uint8_t* __restrict__ a4,
                               uint8_t* __restrict__ a6) {
  static_assert(PairWs16<W16A3, W16B4>::SEGS == 1, "conv3+4 tile k of workgroup b is image b + kG");
  const int b = (int)blockIdx.x, G = (int)gridDim.x;
  const int T = b < nimg ? 2 * ((nimg - 1 - b) / G + 1) : 0;
  conv12p_body(b, G, T, img, nimg, 0.0f, z0, w0, e0, z1, w1, e1, a2, qlut);
  phase_boundary();
  convpair_ws16_body<W16A3, W16B4, EM, EM, false>(b, G, a2, nimg, z2, w2, e2, z3, w3, e3, a4);
  phase_boundary();
  convpair_ws16_body<W16A5, W16B6, EM, EM, KMAJOR, true>(b, G, a4, nimg, z4, w4, e4, z5, w5, e5, a6);
}

// convnet_convs_sm_kernel with the u8 conv12 phase
__global__ __launch_bounds__(512, 1)
void convnet_convs_sm_u8_kernel(const uint8_t* __restrict__ img, int nimg,
                                const uint8_t* __restrict__ qlut, QCN_C16_PARAMS,
                                uint8_t* __restrict__ a2, uint8_t* __restrict__ a4,
                                uint8_t* __restrict__ a6) {
  const int b = (int)blockIdx.x;
  conv12p_body(b, (int)gridDim.x, 2, img, nimg, 0.0f, z0, w0, e0, z1, w1, e1, a2, qlut);
  phase_boundary();
  convpair_body<SmA3, SmB4>(b, a2, nimg, z2, w2, e2, z3, w3, e3, a4);
  phase_boundary();
  convpair_ga_body<SmA5, SmB6, kSm56D>(b, a4, nimg, z4, w4, e4, z5, w5, e5, a6);
}

// the one-launch kernels of the raw-u8 input (convnet_convs)
struct ConvsU8 {
  static constexpr auto sm = convnet_convs_sm_u8_kernel;
  template <int EM, bool KMAJOR>
  static constexpr auto k16 = convnet_convs16_u8_kernel<EM, KMAJOR>;
  static constexpr int kLdsSm = kConvnetSmLdsU8, kLds16 = kConvnet16LdsU8;
};

}  // namespace qcn

extern "C" {

int qcn_conv12_fused_u8_nhwc(const uint8_t* img, int nimg, const uint8_t* qlut, int in_zp,
                             const int8_t* w1_packed, const float* u1, const float* v1,
                             const float* mult1, const int32_t* corr1, int z1, int relu1,
                             const qcn_qdq_t* qdq1, int x2_zp, const int8_t* w2_packed,
                             const float* u2, const float* v2, const float* mult2,
                             const int32_t* corr2, int y_zp, int relu2, const qcn_qdq_t* qdq2,
                             uint8_t* y, void* stream) {
  // the window rows are dword loads
  if (!qlut || (reinterpret_cast<uintptr_t>(img) & 3)) return QCN_ERR_ARG;
  return qcn::conv12_fused<qcn::conv12p_u8_kernel, qcn::Conv12P::LDS_U8>(
      img, nimg, qlut, {w1_packed, u1, v1, mult1, corr1, in_zp, z1, relu1, qdq1},
      {w2_packed, u2, v2, mult2, corr2, x2_zp, y_zp, relu2, qdq2}, y, stream);
}

int qcn_convnet_convs_u8_nhwc(const uint8_t* img, int nimg, const uint8_t* qlut, int in_zp,
                              const qcn_conv_layer_t* layers, uint8_t* a2, uint8_t* a4, uint8_t* a6,
                              int kmajor, void* stream) {
  if (!qlut || (reinterpret_cast<uintptr_t>(img) & 3)) return QCN_ERR_ARG;   // dword window loads
  // the plan does not depend on the input scale (the table carries it)
  return qcn::convnet_convs<qcn::ConvsU8>(img, nimg, qlut, 1.0f, in_zp, layers, a2, a4, a6, kmajor, stream);
}

}  // extern "C"
