// CAUNet (reference model/CAUNet.py:307-374) kernel arguments, packed weight layouts and host
// launchers (caunet.hip).  Activations are channels-last [B][F][W][64] in the compute dtype T
// (F frames, W positions in the frame); the sampler state, the condition and eps are fp32 [B][N].
#pragma once
#include "wu_kernels.h"

namespace sddm {

constexpr int kCauC = 64;        // inner_channel: every conv's output channels
constexpr int kCauD = 32;        // Dual_Transformer d_model = C / 2
constexpr int kCauHid = 64;      // GRU hidden size per direction (2 d_model)
constexpr int kCauHeads = 4;     // nn.MultiheadAttention(32, 4): head dimension 8
constexpr int kCauEmb = 64;      // PositionalEncoding(64)
constexpr int kCauMlpHid = 256;  // FeatureWiseAffine: Linear 64 -> 256 -> 64 (128 with use_affine_level)

// Every matrix W[N][K] travels as MFMA A fragments [N / 16][K / 32][64 lanes][8] in T: lane l of
// fragment (nt, kc) holds W[16 nt + (l & 15)][32 kc + 8 (l >> 4) + j], j = 0..7.
constexpr int cau_frag_elems(int N, int K) { return (N / 16) * (K / 32) * 512; }

// ---- first_conv: Conv2d(2, 64, 1x1) over the frames of (cond, y_t), no norm, no activation.
// Decrements the device step counter t_dev (the first launch of a reverse step; null in a forward)
struct CauFirstArgs {
  const float* cond; const float* x;     // [B][N]
  const float* w; const float* bias;     // [64][2], [64] fp32
  void* out;                             // [B][F][128][64] (T)
  int B, F; int64_t N; int* t_dev;
};
hipError_t launch_cau_first(int dtype, const CauFirstArgs& a, hipStream_t s);

// ---- the eight FeatureWiseAffine MLPs of one step: PositionalEncoding(64) of the row's level ->
// Linear 64 -> 256, PReLU(256), Linear 256 -> 64 (affine: 128 = gamma | beta).  Writes the
// per-(row, layer, channel) scale (1 + gamma, or 1) and shift (beta, or the MLP's output).
struct CauNoiseArgs {
  WULevel lv;
  const float* w1; const float* b1; const float* a1;   // [NL][256][64], [NL][256], [NL][256]
  const float* w2; const float* b2;                    // [NL][OUT][256], [NL][OUT]; OUT = 64 or 128
  int affine, B, NL;
  float* sc; float* sh;                                // [B][NL][64]
};
hipError_t launch_cau_noise(const CauNoiseArgs& a, hipStream_t s);

// ---- the MFMA implicit-GEMM convolution to 64 channels with LayerNorm over the output row and a
// per-channel PReLU in the epilogue.  A block owns 128 conv positions = 128 / Wc whole rows.
//   CAU_DENSE: (2,3) taps, frame dilation dil, causal (zero rows above), one zero column each side,
//              over nsrc concatenated 64-channel sources (newest first, DenseBlock CAUNet.py:241-249)
//   CAU_DOWN:  (1,3) taps, stride (1,2), padding (0,1): Win = 2 Wc
//   CAU_UP:    SPConvTranspose2d (CAUNet.py:204-219): (1,3) taps over two sources to 128 channels,
//              channel r * 64 + c stored at [c][h][2 w + r]; the norm is over the 2 Wc outputs
// The affine x * sc + sh of the layer's FeatureWiseAffine is applied to source aff_src as it is
// loaded, inside the image only (the padding stays zero).
enum { CAU_DENSE = 0, CAU_DOWN = 1, CAU_UP = 2 };
struct CauConvArgs {
  int mode;
  const void* src[3]; int nsrc;          // [B][F][Win][64] (T)
  int dil, aff_src;                      // aff_src -1: no affine
  const float* sc; const float* sh; int aff_ld;   // row b, channel c at [b * aff_ld + c]
  const void* w;                         // fragments of W[64 NR][nsrc * KH * 3 * 64], k = ((s KH + kh) 3 + kw) 64 + ci
  const float* bias; const float* lnw; const float* lnb; const float* alpha;   // [64 NR], [Wout], [Wout], [64]
  void* out;                             // [B][F][Wout][64] (T)
  int B, F, Wc;                          // Wc: conv output width, a power of two in [8, 128]
};
hipError_t launch_cau_conv(int dtype, const CauConvArgs& a, hipStream_t s);

// ---- final_conv (1x1, 64 -> 1) and overlap-add of the 128 / 64 frames -> eps [B][N] fp32
struct CauFinalArgs { const void* src; const float* w; const float* bias; float* out; int B, F; int64_t N; };
hipError_t launch_cau_final(int dtype, const CauFinalArgs& a, hipStream_t s);

// ---- Dual_Transformer(64, 64, 0, n_tstb) (CAUNet.py:152-201) at d_model 32 over [B][dim2][dim1][64].
// Matrix blob (T):
constexpr int kCauWIn = 0;                                                  // input.0 [32][64]
constexpr int kCauWOut = kCauWIn + cau_frag_elems(kCauD, kCauC);            // output.0 [64][32]
constexpr int kCauWEnc0 = kCauWOut + cau_frag_elems(kCauC, kCauD);
// one TransformerEncoderLayer (row_trans[0], col_trans[0], row_trans[1], ...)
constexpr int kCauEInProj = 0;                                              // in_proj_weight [96][32]
constexpr int kCauEOutProj = kCauEInProj + cau_frag_elems(3 * kCauD, kCauD);   // out_proj.weight [32][32]
constexpr int kCauEIh = kCauEOutProj + cau_frag_elems(kCauD, kCauD);        // weight_ih_l0 [192][32], then _reverse
constexpr int kCauEIhSize = cau_frag_elems(3 * kCauHid, kCauD);
constexpr int kCauEHh = kCauEIh + 2 * kCauEIhSize;                          // weight_hh_l0 [192][64], then _reverse
constexpr int kCauEHhSize = cau_frag_elems(3 * kCauHid, kCauHid);
constexpr int kCauELin2 = kCauEHh + 2 * kCauEHhSize;                        // linear2.weight [32][128]
constexpr int kCauEncW = kCauELin2 + cau_frag_elems(kCauD, 2 * kCauHid);
// Vector blob (fp32): input bias 32 | input PReLU 32 | output bias 64 | output PReLU 64 | encoders
constexpr int kCauVInB = 0, kCauVInA = 32, kCauVOutB = 64, kCauVOutA = 128, kCauVEnc0 = 192;
// per encoder: in_proj_bias 96 | out_proj.bias 32 | norm1 w, b | bias_ih, bias_hh (forward) | bias_ih,
// bias_hh (reverse) | linear2.bias | norm2 w, b | row_norm / col_norm w, b
constexpr int kCauVInProjB = 0, kCauVOutProjB = 96, kCauVLn1W = 128, kCauVLn1B = 160, kCauVBih = 192,
              kCauVBhh = 384, kCauVLin2B = 960, kCauVLn2W = 992, kCauVLn2B = 1024, kCauVGnW = 1056,
              kCauVGnB = 1088, kCauEncV = 1120;   // reverse direction: kCauVBih / kCauVBhh + 384

constexpr int kCauTokTile = 64;   // tokens per block of the per-token kernels = one GroupNorm partial
struct CauDtArgs {
  const void* x;              // [B][dim2][dim1][64] (T)
  void* out;                  // [B][dim2][dim1][64] (T)
  const void* wmat; const float* wvec;
  char* ws;                   // cau_dt_ws_bytes(dtype, B, dim2 * dim1) bytes
  int B, dim2, dim1, n_tstb;
  int prelu_first;            // the output stage of tstnn.py:139-141: PReLU (the 32 slopes at kCauVOutA), then
                              // the conv with its bias and nothing after it; 0: conv, then PReLU(64) (CAUNet)
};
size_t cau_dt_ws_bytes(int dtype, int64_t B, int64_t P);
// 2 + 10 n_tstb launches: input conv; per encoder in_proj, attention, out_proj + norm1, GRU,
// linear2 + norm2; output conv.  An image's GroupNorm statistics cross the kernel boundary as
// per-block partials; no block waits for another.
hipError_t launch_cau_dual_transformer(int dtype, const CauDtArgs& a, hipStream_t s);

}  // namespace sddm
