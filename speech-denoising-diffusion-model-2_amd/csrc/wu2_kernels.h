// Kernel argument structs and host launchers of the two FiLM Wave-U-Nets: Waveunet2 (implemented in
// waveunet2.hip) and the 12-level Waveunet (its conv launcher: waveunet1.hip; the stem, the GroupNorm
// finalize and the head are Waveunet2's, the first level of both networks is 24 channels wide).
#pragma once
#include "wu_kernels.h"

namespace sddm {

// Activations are channels-last [B][L][C] in the compute dtype T at the true C (24 (i + 1): a
// multiple of 8, so 8 channels are one 16-byte vector in 16-bit).  A ConvLayer's raw conv output is
// what is stored; its GroupNorm + ReLU is applied by whoever reads it, from the scale / shift
// [B][C] that launch_wu_gn_finalize (wu_kernels.h) makes of the producer's statistics partials
// [B][nslots][C][2].  The noise level of a row is a WULevel, as for Waveunet3.

// ---- stem: raw = Conv1d(2, 24, 5, padding 2) of cat(cond, y_t) (no norm on the raw input): WUStemArgs
// (wu_kernels.h) with w [24][2][5], bias [24] and t_dev
constexpr int kWu2StemC = 24;
hipError_t launch_wu2_stem(int dtype, const WUStemArgs& a, hipStream_t s);

// ---- the MFMA implicit-GEMM convolution (modes: wu_kernels.h) for channel counts that are multiples of 8
// prologue: none (scale null), or ReLU(v * scale[b][c] + shift[b][c]), then with `film`
//   film[b][l][Cin + c] * v + film[b][l][c] (film = the FiLM output_conv's [B][Lin][2 Cin]: shift
//   first, scale second); the halo is zero after all of it.
// epilogue: + bias, then with enc_dim > 0 leaky_relu(0.2) + PositionalEncoding(level)[c]
//   (enc_dim == Cout), store, statistics partials (stats null: none).
struct WU2ConvArgs {
  int mode;
  const void* src; int Lin, Cin;          // [B][Lin][Cin] (T), Cin % 8 == 0
  const float* scale; const float* shift; // [B][Cin] or null
  const void* film;                       // [B][Lin][2 Cin] (T) or null
  const void* w; const float* bias;       // packed [Cout][taps][Cin] (T), [Cout] fp32
  int enc_dim; WULevel lv;
  void* out; int Lout, Cout;              // Cout % 8 == 0
  float* stats;                           // [B][4 ntiles][Cout][2] or null
  int B;
};
// what both conv launchers refuse: max_c bounds Cin and enc_dim, max_cout the Cout of every mode but
// WU_CONV3, max_cout3 WU_CONV3's (the FiLM output_conv is twice as wide as its level)
inline hipError_t wu2_conv_check(const WU2ConvArgs& a, int max_c, int max_cout, int max_cout3) {
  if (a.mode < WU_CONV5 || a.mode > WU_UP4 || a.B < 1 || a.B > 65535 || a.Lin < 1 || a.Lout < 1) return hipErrorInvalidValue;
  if (!a.src || !a.w || !a.bias || !a.out) return hipErrorInvalidValue;
  if (a.Cin % 8 || a.Cin < 8 || a.Cin > max_c || a.Cout % 8 || a.Cout < 8) return hipErrorInvalidValue;
  if (a.Cout > (a.mode == WU_CONV3 ? max_cout3 : max_cout)) return hipErrorInvalidValue;
  if (((a.mode == WU_CONV5 || a.mode == WU_CONV3) && a.Lout != a.Lin) || (a.mode == WU_DOWN4 && a.Lin != 2 * a.Lout) ||
      (a.mode == WU_UP4 && a.Lout != 2 * a.Lin))
    return hipErrorInvalidValue;
  if ((a.scale == nullptr) != (a.shift == nullptr) || (a.film && (!a.scale || a.mode != WU_CONV5))) return hipErrorInvalidValue;
  if (a.enc_dim && (a.enc_dim != a.Cout || a.enc_dim > max_c || a.enc_dim % 2)) return hipErrorInvalidValue;
  if (a.enc_dim && !a.lv.levels && (!a.lv.t_dev || (!a.lv.time_step && !a.lv.table))) return hipErrorInvalidValue;
  return hipSuccess;
}
// Waveunet2's launcher (waveunet2.hip): every block holds the whole Cout, Cin <= 96, Cout <= 144
hipError_t launch_wu2_conv(int dtype, const WU2ConvArgs& a, hipStream_t s);

// ---- the same convolution for the 12-level Waveunet (waveunet1.hip): layers up to 288 -> 288 (FiLM
// output_conv: 264 -> 528).  A block no longer holds the whole Cout: blockIdx.z selects a group of
// `gco` output channels (a multiple of 16; the last group may be short), so a block's accumulators
// and weight image stay at the sizes Waveunet2's have.  launch_wu1_conv chooses gco (wu1_conv_group).
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
hipError_t launch_wu1_conv(int dtype, const WU2ConvArgs& a, hipStream_t s);

// ---- head: eps = clamp(Conv1x1 24 -> 1 of ReLU(GN(raw)), -1, 1) as fp32 [B][L]
struct WU2HeadArgs {
  const void* src; const float* scale; const float* shift;   // [B][L][24] (T), [B][24]
  const float* w; const float* bias; float* out; int B, L;
};
hipError_t launch_wu2_head(int dtype, const WU2HeadArgs& a, hipStream_t s);

}  // namespace sddm
