// Waveunet3 kernel argument structs and host launchers (implemented in waveunet.hip).
#pragma once
#include "sddm_common.h"

namespace sddm {

// Activations are channels-last [B][L][C] in the compute dtype T.  GroupNorm statistics travel as
// per-slot partials [B][nslots][C][2] (sum, sum of squares of the values as stored, fp32): a slot
// is the share of one wave (or one fixed group of threads) of a producer block, so the partials are
// written by plain stores and reduced in a fixed order by wu_gn_finalize -- no atomics anywhere.

// the noise level of a row: levels[b] (network forward), else the step's t ('time_step') or
// table[t] (sqrt_alpha_bar) with t read from the device step counter
struct WULevel { const float* levels; const float* table; int time_step; const int* t_dev; };

// ---- GroupNorm finalize: partials -> per-(row, channel) scale = gamma * rstd, shift = beta - mean * scale
struct WUGnArgs {
  const float* stats; int nslots, C, G; int64_t L;   // L positions per row behind the partials
  const float* gamma; const float* beta; float eps;
  float* scale; float* shift;                        // [B][C]
  int B;
};
hipError_t launch_wu_gn_finalize(const WUGnArgs& a, hipStream_t s);

// ---- statistics of the two raw input channels (GroupNorm(2, 2) of the first block: one group per
// channel) -> scale / shift [B][2]; channel 0 = condition, 1 = y_t (waveunet3.py:396).  Decrements
// the device step counter (the first launch of a reverse step)
struct WUInStatsArgs {
  const float* cond; const float* x; int B, L; const float* gamma; const float* beta; float eps;
  float* scale; float* shift; int* t_dev;
};
hipError_t launch_wu_in_stats(const WUInStatsArgs& a, hipStream_t s);

// ---- stem: Conv1d(2, C, 5, padding 2) of cat(cond, y_t) + bias, 2 -> C channels (VALU), with the
// statistics partials of what it stored.  One argument struct for both networks:
//   Waveunet3 (launch_wu_stem, C = 32): the sources go through SiLU(GN(2, 2)) from scale / shift, and
//     the block's noise constant nw * level + nb is added; t_dev is not used (wu_in_stats steps it)
//   Waveunet2 (launch_wu2_stem, wu2_kernels.h, C = 24): the raw sources; scale, shift, nw, nb and lv
//     are not used.  Decrements the device step counter t_dev (the first launch of a reverse step;
//     null in a forward)
constexpr int kWuStemTile = 256;          // positions per block; 8 statistics slots per block
struct WUStemArgs {
  const float* cond; const float* x; const float* scale; const float* shift;   // [B][L], [B][2]
  const float* w; const float* bias;      // [C][2][5], [C] fp32
  const float* nw; const float* nb;       // Waveunet3: Linear(1, C) of the block's noise_func
  WULevel lv;
  void* out; float* stats; int B, L;      // [B][L][C] (T), [B][8 ceil(L / 256)][C][2]
  int* t_dev;
};
hipError_t launch_wu_stem(int dtype, const WUStemArgs& a, hipStream_t s);

// ---- the MFMA implicit-GEMM convolution (one kernel for both networks, wu_conv_impl.h)
//   WU_CONV5: 5 taps, stride 1, padding 2               (Block / ConvLayer convs)
//   WU_CONV3: 3 taps, stride 1, padding 1               (Waveunet2 only: FiLM input_conv / output_conv)
//   WU_DOWN4: 4 taps, stride 2, padding 1, Lout = Lin/2 (DownsampleLayer)
//   WU_UP4:   ConvTranspose1d 4 taps, stride 2, padding 1, Lout = 2 Lin, as two output phases of
//             2 taps each (UpsampleLayer)
// prologue: GroupNorm + SiLU from scale / shift [B][Cin] (null: none); the halo is zero after it.
// epilogue: + bias [+ nw * level + nb] [+ residual] [+ shortcut], store, statistics partials.
// residual: 1 identity (res [B][Lout][Cout]), 2 the 1x1 res_conv as extra K steps over the block's
//   un-normalised input (res [B][Lout][RC], rw [Cout][RC]; its bias is folded into `bias`), 3 the
//   first block's 2 -> 32 res_conv on the raw fp32 inputs (rw2 [Cout][2], bias folded likewise)
// The above is Waveunet3's launch (no WU_CONV3); Waveunet2's is in wu2_kernels.h.
enum { WU_CONV5 = 0, WU_CONV3 = 1, WU_DOWN4 = 2, WU_UP4 = 3 };
constexpr int kWuTile = 128;              // output positions per block; 4 statistics slots per block
struct WUConvArgs {
  int mode;
  const void* src; int Lin, Cin;          // [B][Lin][Cin] (T), Cin % 32 == 0
  const float* scale; const float* shift;
  const void* w; const float* bias;       // packed [Cout][taps][Cin] (T), [Cout] fp32
  const float* nw; const float* nb; WULevel lv;
  int res_mode; const void* res; int RC; const void* rw;
  const float* cond; const float* x; const float* rw2;
  const void* shortcut;                   // [B][Lout][Cout] (T) or null
  void* out; int Lout, Cout;              // Cout 32 / 64 / 96 / 128 (resampling: not 32)
  float* stats;                           // [B][4 ntiles][Cout][2] or null
  int B;
};
hipError_t launch_wu_conv(int dtype, const WUConvArgs& a, hipStream_t s);
inline int wu_conv_slots(int Lout) { return 4 * ((Lout + kWuTile - 1) / kWuTile); }   // statistics slots of a launch

// ---- the ConvLayer's own norm: y = ReLU(GN(raw)) with the statistics partials of y
constexpr int kWuActTile = 64;            // positions per block; 1 statistics slot per block
struct WUActArgs {
  const void* src; const float* scale; const float* shift; void* out; float* stats; int B, L, C;
};
hipError_t launch_wu_act(int dtype, const WUActArgs& a, hipStream_t s);

// ---- head: eps = clamp(Conv1x1 32 -> 1, -1, 1) as fp32 [B][L]
struct WUHeadArgs { const void* src; const float* w; const float* bias; float* out; int B, L; };
hipError_t launch_wu_head(int dtype, const WUHeadArgs& a, hipStream_t s);

}  // namespace sddm
