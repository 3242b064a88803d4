// Geometry shared by the dynamic int8 3x3 conv kernels (conv_dyn.hip,
// conv_dyn_pair.hip): the K chunking, the LDS band strides and the MFMA step
// count that qcn_pack_conv3x3_weight_dyn's format is built on.
#pragma once

namespace qcn {

constexpr int CD_CK = 256;       // channels per LDS chunk (16 K units per tap)
constexpr int CD_ROWS = 8;       // output rows of a block
constexpr int CD_MAX_CIN = 7310; // 9 * cin * 255 * 128 <= 2^31 - 1

// LDS strides in bytes for chunks of ncg 16-channel groups and lcols columns
__host__ __device__ constexpr int cd_pixel_stride(int ncg) {
  return 16 * (ncg % 4 ? ncg + (ncg == 1) : (ncg % 8 ? ncg : ncg + 2));
}
__host__ __device__ constexpr int cd_row_stride(int ncg, int lcols) {
  return lcols * cd_pixel_stride(ncg) + (ncg % 4 ? (ncg == 1 ? 16 : 96) : (ncg % 8 ? 32 : 64));
}
// MFMA steps of all chunks of a layer
__host__ __device__ constexpr int cd_steps(int cin) {
  const int ncg = (cin + 15) / 16;
  return (ncg / 16) * 36 + (9 * (ncg % 16) + 3) / 4;
}

}  // namespace qcn
