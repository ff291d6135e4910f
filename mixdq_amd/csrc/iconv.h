// 3x3 / stride 1 / pad 1 INT8 convolution with the input HALO resident in LDS (csrc/iconv.hip).
#pragma once
#include "common.h"

namespace mixdq {

struct HaloConvArgs {
  const int8_t* X;        // [NI, H, W, C] int8 (NHWC)
  const int8_t* Wt;       // [K, 3, 3, C] int8, or [K, 3, 3, C / 2] packed signed 4-bit (halo_conv_launch w4)
  const float* scale;     // [K]
  const __half* bias;     // [K] or null
  const float* table;     // [81][K] tap-rectangle sums (mixdq_conv_border_table)
  const float* zp;        // device scalar: the activation zero point
  __half* D;              // [NI, H, W, K]
  const __half* res;      // residual or null: [NI, H, W, K] (res_div == 1) or [NI, K] (res_div == H * W)
  int64_t res_div;
  int NI, H, W, C, K;     // H, W: the conv's input (= output) size
  int unfused;
  int ups;                // 1: X is [NI, H / 2, W / 2, C] and the conv reads its nearest-neighbour 2x
                          //    upsampling (Upsample2D: conv(interpolate(x))) without materialising it
};

// The halo kernel's tiles: X(id, TH, TW, BN, CK, WNG) -- output pixels (rows, columns), output channels, channel
// chunk bytes, wave groups along the channels.  The only place they are written: halo_conv_launch's W8 and W4
// switches are generated from it, and mixdq_tile_config (family 5) reports it.
#define MIXDQ_HALO_TILES(X)   \
  X(90, 8, 16, 80, 128, 1)    \
  X(91, 8, 8, 80, 128, 1)     \
  X(92, 16, 16, 80, 64, 1)    \
  X(93, 16, 16, 160, 64, 2)

// Tile id the halo kernel would run this problem on (90: 8x16 pixels x 80 channels, 91: 8x8 x 80, 92: 16x16 x 80, 93: 16x16 x 160), or 0
// when the problem is outside its range (then the implicit-GEMM family of csrc/igemm.hip runs it).
// w4: for packed 4-bit weights (MIXDQ_FLAG_W4) -- the same range (what a forced tile id is checked against: ask
// with w4 = false) and the same rule but for one measured exception (csrc/iconv.hip).
int halo_conv_select(int NI, int H, int W, int C, int K, int R, int S, int stride, int pad, bool w4 = false);

// Launch; `tile` from halo_conv_select (or forced); w4: Wt is packed.  Returns a mixdq_status.
int halo_conv_launch(const HaloConvArgs& a, int tile, hipStream_t stream, bool w4 = false);

}  // namespace mixdq
