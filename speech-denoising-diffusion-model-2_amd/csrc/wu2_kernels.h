// Waveunet2 kernel argument structs and host launchers (implemented in waveunet2.hip).
#pragma once
#include "wu_kernels.h"

namespace sddm {

// Activations are channels-last [B][L][C] in the compute dtype T at the true C (24 / 48 / 72 / 96: a
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
  const void* src; int Lin, Cin;          // [B][Lin][Cin] (T), Cin % 8 == 0, <= 96
  const float* scale; const float* shift; // [B][Cin] or null
  const void* film;                       // [B][Lin][2 Cin] (T) or null
  const void* w; const float* bias;       // packed [Cout][taps][Cin] (T), [Cout] fp32
  int enc_dim; WULevel lv;
  void* out; int Lout, Cout;              // Cout % 8 == 0, <= 144
  float* stats;                           // [B][4 ntiles][Cout][2] or null
  int B;
};
hipError_t launch_wu2_conv(int dtype, const WU2ConvArgs& a, hipStream_t s);

// ---- head: eps = clamp(Conv1x1 24 -> 1 of ReLU(GN(raw)), -1, 1) as fp32 [B][L]
struct WU2HeadArgs {
  const void* src; const float* scale; const float* shift;   // [B][L][24] (T), [B][24]
  const float* w; const float* bias; float* out; int B, L;
};
hipError_t launch_wu2_head(int dtype, const WU2HeadArgs& a, hipStream_t s);

}  // namespace sddm
