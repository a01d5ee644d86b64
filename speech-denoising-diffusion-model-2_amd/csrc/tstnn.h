// TSTNN (reference model/tstnn.py:216-299) kernel arguments and host launchers (tstnn.hip).
// Activations are channels-last [B][Fr][W][64] in the compute dtype T (Fr frames of 512 samples
// every 256, W positions in the frame: 512, or 256 between the two resampling convs); the sampler
// state, the condition and eps are fp32 [B][N].  The Dual_Transformer is caunet.hip's
// (launch_cau_dual_transformer with CauDtArgs::prelu_first); the weights travel as caunet.h's MFMA
// A fragments.
#pragma once
#include "caunet.h"

namespace sddm {

constexpr int kTstnnF = 512;        // frame length F
constexpr int kTstnnStride = 256;   // frame stride
constexpr int kTstnnLayers = 4;     // Dual_Transformer(64, 64, num_layers=4) of the network

// ---- frames of (cond, y_t) -> inp_conv (1x1, 2 -> 64) -> LayerNorm(512) over the frame -> PReLU(64).
// One block per frame.  The row statistics come from the frame's own moments (the conv is linear in
// the two inputs): mean_c = w0 mean(u) + w1 mean(v) + b, and the centred value is
// w0 (u - mean u) + w1 (v - mean v); all fp32, the stored output is rounded to T.
// Decrements the device step counter t_dev (the first launch of a reverse step; null in a forward)
struct TstnnFirstArgs {
  const float* cond; const float* x;     // [B][N]
  const float* w;                        // [64][2] fp32; inp_conv's bias is constant over the frame, so the
                                         // LayerNorm removes it and the kernel never reads it
  const float* lnw; const float* lnb; const float* alpha;   // [512], [512], [64]
  void* out;                             // [B][Fr][512][64] (T)
  int B, F; int64_t N; int* t_dev;
};
hipError_t launch_tstnn_first(int dtype, const TstnnFirstArgs& a, hipStream_t s);

// ---- the wide-row convolution: caunet.h's implicit GEMM (MFMA 16x16x32, wave j owns output channels
// 16 j .. 16 j + 15, weights as fragments with k = ((s KH + kh) 3 + kw) 64 + ci) with one block per
// row of Wc = 256 or 512 conv positions, so the row's LayerNorm stays inside the block.  Modes and
// their meaning are CauConvArgs' (no affine):
//   CAU_DENSE  nsrc 1..4, dil >= 1, Wc 256 or 512
//   CAU_DOWN   nsrc 1, Wc 256 from Win 512
//   CAU_UP     nsrc 1, Wc 256 -> 512 outputs, the norm over the 512
// One (source, kh) slab of Win + 2 pixels x 72 channels is staged at a time: 72.3 KiB in the 16-bit
// types, 144.6 KiB in fp32 at Win 512; the launcher refuses what the device's LDS does not hold.
// Rounded to T: the weights, the inputs (they are stored as T) and the stored output.
struct TstnnConvArgs {
  int mode;
  const void* src[4]; int nsrc;          // [B][Fr][Win][64] (T), newest first
  int dil;
  const void* w;                         // fragments of W[64 NR][nsrc * KH * 3 * 64]
  const float* bias; const float* lnw; const float* lnb; const float* alpha;   // [64 NR], [Wout], [Wout], [64]
  void* out;                             // [B][Fr][Wout][64] (T)
  int B, F, Wc;
};
hipError_t launch_tstnn_conv(int dtype, const TstnnConvArgs& a, hipStream_t s);

// ---- the gated mask, per token (tstnn.py:287-291):
//   mask = ReLU(Wm (tanh(W1 y + b1) * sigmoid(W2 y + b2)) + bm),  out = x1 * mask
// Three 64 x 64 MFMA products per 16-token tile.  The gate leaves the first two products in the
// accumulator layout (lane (g, col) holds channels 16 nt + 4 g + i) and enters the third as a B
// fragment without moving: Wm's fragments are packed with their K index permuted to match
// (tstnn_gate_k below), which leaves every dot product unchanged.
// Rounded to T: W1, W2, Wm; y and x1 (stored as T by their producers); the gate
// tanh(.) * sigmoid(.) where it enters the third product; the stored output.  Biases, tanh, sigmoid,
// ReLU and the product with x1 are fp32.
struct TstnnGateArgs {
  const void* y; const void* x1;         // [tokens][64] (T)
  const void* w1; const void* w2; const void* wm;   // fragments of [64][64]
  const float* b1; const float* b2; const float* bm;
  void* out;                             // [tokens][64] (T)
  int64_t tokens;
};
// channel that sits in K slot kk (0..63) of the gate's B fragments
constexpr int tstnn_gate_k(int kk) { return (2 * (kk / 32) + ((kk % 8) >> 2)) * 16 + 4 * ((kk % 32) / 8) + (kk & 3); }
hipError_t launch_tstnn_gate(int dtype, const TstnnGateArgs& a, hipStream_t s);

// ---- out_conv (1x1, 64 -> 1) and overlap-add of the 512 / 256 frames -> eps [B][N] fp32; the frames
// are added in ascending order as overlapAdd does (tstnn.py:37-39)
struct TstnnFinalArgs { const void* src; const float* w; const float* bias; float* out; int B, F; int64_t N; };
hipError_t launch_tstnn_final(int dtype, const TstnnFinalArgs& a, hipStream_t s);

}  // namespace sddm
