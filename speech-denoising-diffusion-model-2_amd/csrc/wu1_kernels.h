// Waveunet (the 12-level Wave-U-Net of config_waveunet.json) kernel argument structs and host
// launchers (implemented in waveunet1.hip).  The stem, the GroupNorm finalize and the head are
// Waveunet2's (wu2_kernels.h, wu_kernels.h): the first level of both networks is 24 channels wide.
#pragma once
#include "wu2_kernels.h"

namespace sddm {

// ---- the MFMA convolution of wu2_kernels.h for layers up to 288 -> 288 (FiLM output_conv: 264 ->
// 528).  A block no longer holds the whole Cout: blockIdx.z selects a group of `gco` output
// channels (a multiple of 16; the last group may be short), so a block's accumulators and weight
// image stay at the sizes Waveunet2's have.  launch_wu1_conv chooses gco (wu1_conv_group).
constexpr int kWu1MaxC = 288;             // the widest Cin and enc_dim
struct WU1ConvArgs : WU2ConvArgs {
  int gco;                                // set by launch_wu1_conv
};
// channels per group: the fewest groups of at most 96 (WU_CONV3: 144) channels, evened out to whole
// fragments -- 120 -> 64 + 56, 168 -> 96 + 72, 288 -> 96 x 3; WU_CONV3: 528 -> 144 x 3 + 96
inline int wu1_conv_group(int mode, int Cout) {
  const int cap = mode == WU_CONV3 ? 144 : 96;
  const int ng = (Cout + cap - 1) / cap;
  return ((Cout + ng - 1) / ng + 15) / 16 * 16;
}
// what both launchers refuse
inline hipError_t wu1_conv_check(const WU2ConvArgs& a) {
  if (a.mode < WU_CONV5 || a.mode > WU_UP4 || a.B < 1 || a.B > 65535 || a.Lin < 1 || a.Lout < 1) return hipErrorInvalidValue;
  if (!a.src || !a.w || !a.bias || !a.out) return hipErrorInvalidValue;
  if (a.Cin % 8 || a.Cin < 8 || a.Cin > kWu1MaxC || a.Cout % 8 || a.Cout < 8 || a.Cout > 2 * kWu1MaxC) return hipErrorInvalidValue;
  if (a.mode != WU_CONV3 && a.Cout > kWu1MaxC) return hipErrorInvalidValue;
  if (((a.mode == WU_CONV5 || a.mode == WU_CONV3) && a.Lout != a.Lin) || (a.mode == WU_DOWN4 && a.Lin != 2 * a.Lout) ||
      (a.mode == WU_UP4 && a.Lout != 2 * a.Lin))
    return hipErrorInvalidValue;
  if ((a.scale == nullptr) != (a.shift == nullptr) || (a.film && (!a.scale || a.mode != WU_CONV5))) return hipErrorInvalidValue;
  if (a.enc_dim && (a.enc_dim != a.Cout || a.enc_dim > kWu1MaxC || a.enc_dim % 2)) return hipErrorInvalidValue;
  if (a.enc_dim && !a.lv.levels && (!a.lv.t_dev || (!a.lv.time_step && !a.lv.table))) return hipErrorInvalidValue;
  return hipSuccess;
}
hipError_t launch_wu1_conv(int dtype, const WU2ConvArgs& a, hipStream_t s);

// ---- the same convolution for rows shorter than a tile (Lout < 128), the batch folded into the
// column dimension (waveunet1_fold.hip): a block owns wu1_fold_rows whole batch rows and its 128
// columns are their positions, so the rows share the weights the block stages.  No statistics
// partials: with gamma / beta the block writes the scale / shift of its rows' output itself
// (oscale / oshift [B][Cout], not the buffers `scale` / `shift` point to: the blocks of the other
// channel groups still read those); null: none (the FiLM convs).  enc_dim > 0 only without gamma.
constexpr int kWu1FoldRows = 16;          // batch rows per block at most
struct WU1FoldArgs : WU2ConvArgs {
  int gco;                                // set by launch_wu1_fold
  const float* gamma; const float* beta; float eps;
  float* oscale; float* oshift;
};
// batch rows per block; 0: the rows are too long
inline int wu1_fold_rows(int mode, int Lin, int Lout) {
  const int r = mode == WU_UP4 ? (kWuTile / 2) / Lin : kWuTile / Lout;
  return r < kWu1FoldRows ? r : kWu1FoldRows;
}
hipError_t launch_wu1_fold(int dtype, const WU1FoldArgs& a, hipStream_t s);

}  // namespace sddm
