// Dual_Transformer (reference model/UNetTST.py:113-233) at d_model 80, 4 heads, GRU hidden 160:
// kernel arguments, the packed weight layout and the host launchers (dual_transformer.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sddm {

// Geometry the kernel is built for (sddm_configure refuses anything else).
constexpr int kTstC = 160;        // channels in and out (the UNet's bottom width)
constexpr int kTstD = 80;         // d_model = C / 2
constexpr int kTstHeads = 4;      // nn.MultiheadAttention(80, 4): head dimension 20
constexpr int kTstHid = 160;      // GRU hidden size per direction (2 d_model)
constexpr int kTstMaxTokens = 64; // dim2 * dim1 of one image: the LDS budget (dt_lds_bytes)

// Matrix weights: one blob in the compute dtype, every matrix W[N][K] (torch's [out][in]) as MFMA
// A fragments [N / 16][ceil(K / 32)][64 lanes][8]: lane l of fragment (nt, kc) holds
// W[16 nt + (l & 15)][32 kc + 8 (l >> 4) + j], j = 0..7, zero where k >= K.
constexpr int tst_frag_elems(int N, int K) { return (N / 16) * ((K + 31) / 32) * 512; }
constexpr int kTstWIn = 0;                                               // input conv1x1 [80][160]
constexpr int kTstWOut = kTstWIn + tst_frag_elems(kTstD, kTstC);         // output conv1x1 [160][80]
constexpr int kTstWEnc0 = kTstWOut + tst_frag_elems(kTstC, kTstD);       // first encoder
// one TransformerEncoderLayer (row_trans[0], col_trans[0], row_trans[1], ...)
constexpr int kTstEInProj = 0;                                           // in_proj_weight [240][80]
constexpr int kTstEOutProj = kTstEInProj + tst_frag_elems(3 * kTstD, kTstD);   // out_proj.weight [80][80]
constexpr int kTstEIh = kTstEOutProj + tst_frag_elems(kTstD, kTstD);     // weight_ih_l0 [480][80], then _reverse
constexpr int kTstEIhSize = tst_frag_elems(3 * kTstHid, kTstD);
constexpr int kTstEHh = kTstEIh + 2 * kTstEIhSize;                       // weight_hh_l0 [480][160], then _reverse
constexpr int kTstEHhSize = tst_frag_elems(3 * kTstHid, kTstHid);
constexpr int kTstELin2 = kTstEHh + 2 * kTstEHhSize;                     // linear2.weight [80][320]
constexpr int kTstEncW = kTstELin2 + tst_frag_elems(kTstD, 2 * kTstHid); // elements per encoder

// Vectors: one fp32 blob.
constexpr int kTstVInB = 0, kTstVInA = 80, kTstVOutB = 96, kTstVOutA = 256, kTstVEnc0 = 272;
// per encoder: in_proj_bias 240 | out_proj.bias 80 | norm1 w, b | bias_ih, bias_hh (forward) |
// bias_ih, bias_hh (reverse) | linear2.bias | norm2 w, b | row_norm / col_norm w, b
constexpr int kTstVInProjB = 0, kTstVOutProjB = 240, kTstVLn1W = 320, kTstVLn1B = 400, kTstVBih = 480,
              kTstVBhh = 960, kTstVLin2B = 2400, kTstVLn2W = 2480, kTstVLn2B = 2560, kTstVGnW = 2640,
              kTstVGnB = 2720, kTstEncV = 2800;   // reverse direction: kTstVBih / kTstVBhh + 960

struct DualTransformerArgs {
  const void* x;              // [B][dim2][dim1][160] in the compute dtype (the last Downsample's output)
  void* out;                  // [B][dim2][dim1][160] in the compute dtype
  float* stats;               // [B][1 tile][160][2]: (sum, M2 about the image mean) of each output channel, or null
  const void* wmat;           // matrix blob (compute dtype)
  const float* wvec;          // vector blob
  int dim2, dim1, n_tstb;
};
// one launch, one block per image (grid = B): input conv, the 2 n_tstb encoders, output conv
hipError_t launch_dual_transformer(int dtype, const DualTransformerArgs& a, int B, hipStream_t s);
size_t dt_lds_bytes();

// fp32 NCHW <-> NHWC in the compute dtype (the stand-alone export only)
hipError_t launch_dt_pack(int dtype, const float* nchw, void* nhwc, int B, int C, int P, hipStream_t s);
hipError_t launch_dt_unpack(int dtype, const void* nhwc, float* nchw, int B, int C, int P, hipStream_t s);

}  // namespace sddm
