// Dual_Transformer (reference model/UNetTST.py:113-233) for gfx950: Conv1x1 160 -> 80 + PReLU, then
// n_TSTB times a TransformerEncoderLayer over the rows (sequences along dim1) and one over the
// columns (sequences along dim2), each followed by GroupNorm(1, 80, eps 1e-8) and a residual, then
// Conv1x1 80 -> 160 + PReLU.  An encoder layer is nn.MultiheadAttention(80, 4), a residual and
// LayerNorm, a bidirectional nn.GRU(80, 160), ReLU, Linear(320, 80), a residual and LayerNorm.
//
// One launch, one block of ten waves per image.  The image (at most 64 tokens of 80 channels) stays
// in LDS in fp32 from the input conv to the output conv; every matrix product is an MFMA with the
// weights as A fragments read from global memory (the packed images of dual_transformer.h) and the
// tokens as B fragments read from LDS.  In a float32 context the operands are fp32 (16x16x4 MFMA);
// in a 16-bit context the weights are stored in that type and the fp32 activations are rounded to
// it where they enter an MFMA, nowhere else.  Softmax, LayerNorm, GroupNorm, the GRU's gates and
// PReLU are fp32.  No atomics; every reduction runs in an order fixed by the block shape, and a
// block reads nothing of another image, so an image's result does not depend on its batch.
//
// The GRU: wave j owns hidden channels 16 j .. 16 j + 15, one direction after the other.  Per time
// step it accumulates the r, z and n gate tiles of its channels (input part, K = 80; recurrent part,
// K = 160; columns = the sequences of the pass) in four accumulators whose lanes hold the same
// (channel, sequence) pair, so the gates combine in registers and only h goes back to LDS.  In the
// 16-bit types the wave's 24 weight fragments of a direction stay in registers over the time steps.
#include "dual_transformer.h"

#include "conv_common.h"

namespace sddm {
namespace {

constexpr int kNT = 640;                 // threads: ten waves, one per GRU channel tile
constexpr int kNW = kNT / 64;
constexpr int kLd = 96;                  // row stride of the 80-wide buffers; columns 80..95 stay zero (K padding)
constexpr int kLdBig = 320;
constexpr int kTok = kTstMaxTokens;
constexpr int kLdsFloats = 3 * kTok * kLd + kTok * kLdBig + 32;

static_assert(kTstHid / 16 == kNW, "one wave per GRU channel tile");

// B fragment (tokens) from fp32 LDS: lane group g = lane >> 4 takes k = 8 g .. 8 g + 7 of the chunk
template <typename T, bool RELU> __device__ __forceinline__ Frag<T> load_act(const float* p) {
  f32x4 lo = *(const f32x4*)p, hi = *(const f32x4*)(p + 4);
  if (RELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo[j] = fmaxf(lo[j], 0.f); hi[j] = fmaxf(hi[j], 0.f); }
  }
  if constexpr (sizeof(T) == 4) {
    return {lo, hi};
  } else {
    Frag<T> f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = (T)lo[j]; f.v[4 + j] = (T)hi[j]; }
    return f;
  }
}

template <typename T> __device__ __forceinline__ Frag<T> load_wgt(const T* w, int nt, int KC, int kc, int lane) {
  return load_frag<T>((const char*)(w + ((size_t)(nt * KC + kc) * 64 + lane) * 8));
}

// out[tok][n] = bias[n] + sum_k W[n][k] x[tok][k] for tok < Nt, n < 16 NT; x rows are ldx floats
// apart and hold finite values up to column 32 KC.  (n tile, token tile) pairs go round the waves.
template <typename T, bool RELU>
__device__ __forceinline__ void tok_gemm(const T* w, int NT, int KC, const float* x, int ldx, int Nt, float* out, int ldo,
                                         const float* bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int TT = (Nt + 15) >> 4;
  for (int item = wave; item < NT * TT; item += kNW) {
    const int nt = item / TT, tt = item - nt * TT;
    const int tok = tt * 16 + col, tk = min(tok, Nt - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < KC; ++kc)
      mfma_frag(acc, load_wgt<T>(w, nt, KC, kc, lane), load_act<T, RELU>(x + tk * ldx + kc * 32 + 8 * g));
    if (tok < Nt) *(f32x4*)(out + tok * ldo + nt * 16 + 4 * g) = acc + *(const f32x4*)(bias + nt * 16 + 4 * g);
  }
}

// dst[tok][c] = LayerNorm(a[tok][c] + b[tok][c]) over the 80 channels; sixteen lanes per token
__device__ __forceinline__ void layer_norm_add(float* dst, const float* a, int lda, const float* b, int ldb, const float* w,
                                               const float* bs, int Nt) {
  const int grp = threadIdx.x >> 4, sub = threadIdx.x & 15;
  for (int t0 = 0; t0 < Nt; t0 += kNT / 16) {
    const int tok = t0 + grp, tk = min(tok, Nt - 1);
    float v[5], s = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) { v[i] = a[tk * lda + sub + 16 * i] + b[tk * ldb + sub + 16 * i]; s += v[i]; }
    const float mean = row_sum16(s) * (1.0f / kTstD);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < 5; ++i) { v[i] -= mean; q += v[i] * v[i]; }
    const float rstd = 1.0f / sqrtf(row_sum16(q) * (1.0f / kTstD) + 1e-5f);
    if (tok < Nt) {
#pragma unroll
      for (int i = 0; i < 5; ++i) dst[tok * kLd + sub + 16 * i] = v[i] * rstd * w[sub + 16 * i] + bs[sub + 16 * i];
    }
  }
}

// sum over the block in a fixed order; every thread gets it
__device__ __forceinline__ float block_sum(float v, float* red) {
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int w = 0; w < kNW; ++w) s += red[w];
  return s;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

template <typename T>
__global__ __launch_bounds__(kNT) void dual_transformer_kernel(DualTransformerArgs a) {
  extern __shared__ __align__(16) char dt_smem[];
  float* cur = (float*)dt_smem;          // [tok][96] the block's running output
  float* src = cur + kTok * kLd;         // [tok][96] the encoder's src after norm1 / its output after norm2
  float* att = src + kTok * kLd;         // [tok][96] attention output, then linear2's output
  float* big = att + kTok * kLd;         // [tok][320] input | q, k, v, out_proj | GRU output | output conv
  float* red = big + kTok * kLdBig;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, col = lane & 15;
  const int b = blockIdx.x, dim1 = a.dim1, dim2 = a.dim2, Nt = dim1 * dim2;
  const T* wm = (const T*)a.wmat;
  const float* wv = a.wvec;

  for (int i = tid; i < 3 * kTok * kLd; i += kNT) cur[i] = 0.f;
  const T* x = (const T*)a.x + (size_t)b * Nt * kTstC;
  for (int i = tid; i < Nt * kTstC; i += kNT) big[(i / kTstC) * kLdBig + i % kTstC] = to_f32<T>(x[i]);
  __syncthreads();
  tok_gemm<T, false>(wm + kTstWIn, kTstD / 16, kTstC / 32, big, kLdBig, Nt, cur, kLd, wv + kTstVInB);
  __syncthreads();
  {
    const float alpha = wv[kTstVInA];
    for (int i = tid; i < Nt * kTstD; i += kNT) {
      float& v = cur[(i / kTstD) * kLd + i % kTstD];
      v = v >= 0.f ? v : alpha * v;
    }
  }
  __syncthreads();

  for (int e = 0; e < 2 * a.n_tstb; ++e) {
    const T* we = wm + kTstWEnc0 + (size_t)e * kTstEncW;
    const float* ve = wv + kTstVEnc0 + (size_t)e * kTstEncV;
    // the pass's view of the image: token of (sequence s, time t) = s * ss + t * ts
    const bool colp = (e & 1) != 0;
    const int nseq = colp ? dim1 : dim2, L = colp ? dim2 : dim1, ss = colp ? 1 : dim1, ts = colp ? dim1 : 1;

    // ---- self attention: q, k, v -> big[:, 0..240)
    tok_gemm<T, false>(we + kTstEInProj, 3 * kTstD / 16, 3, cur, kLd, Nt, big, kLdBig, ve + kTstVInProjB);
    __syncthreads();
    for (int item = tid; item < Nt * kTstHeads; item += kNT) {
      const int tok = item >> 2, h = item & 3;
      const int s = colp ? tok % dim1 : tok / dim1;
      float q[20];
#pragma unroll
      for (int j = 0; j < 20; ++j) q[j] = big[tok * kLdBig + h * 20 + j] * 0.22360679774997896f;   // 20^-0.5
      float m = -INFINITY;
      for (int u = 0; u < L; ++u) {
        const float* k = big + (s * ss + u * ts) * kLdBig + kTstD + h * 20;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 20; ++j) d += q[j] * k[j];
        m = fmaxf(m, d);
      }
      float sum = 0.f, acc[20];
#pragma unroll
      for (int j = 0; j < 20; ++j) acc[j] = 0.f;
      for (int u = 0; u < L; ++u) {
        const float* k = big + (s * ss + u * ts) * kLdBig + kTstD + h * 20;
        float d = 0.f;
#pragma unroll
        for (int j = 0; j < 20; ++j) d += q[j] * k[j];
        const float p = expf(d - m);
        sum += p;
#pragma unroll
        for (int j = 0; j < 20; ++j) acc[j] += p * k[kTstD + j];
      }
      const float rs = 1.0f / sum;
#pragma unroll
      for (int j = 0; j < 20; ++j) att[tok * kLd + h * 20 + j] = acc[j] * rs;
    }
    __syncthreads();
    tok_gemm<T, false>(we + kTstEOutProj, kTstD / 16, 3, att, kLd, Nt, big + 3 * kTstD, kLdBig, ve + kTstVOutProjB);
    __syncthreads();
    layer_norm_add(src, cur, kLd, big + 3 * kTstD, kLdBig, ve + kTstVLn1W, ve + kTstVLn1B, Nt);
    __syncthreads();

    // ---- bidirectional GRU over src -> big[:, 0..160) forward, [160..320) reverse
    // One direction after the other.  16-bit types: the wave's 24 weight fragments of a direction
    // (9 of weight_ih, 15 of weight_hh: 96 registers) are loaded once and stay in registers over the
    // time steps, so a step waits for LDS only; fp32 fragments are twice as wide and are loaded per step
    constexpr bool kHold = sizeof(T) == 2;
    for (int d = 0; d < 2; ++d) {
      const T* wih = we + kTstEIh + d * kTstEIhSize;
      const T* whh = we + kTstEHh + d * kTstEHhSize;
      const float* bih = ve + kTstVBih + d * 960 + wave * 16 + 4 * g;
      const float* bhh = ve + kTstVBhh + d * 960 + wave * 16 + 4 * g;
      const f32x4 brz[2] = {*(const f32x4*)bih + *(const f32x4*)bhh, *(const f32x4*)(bih + 160) + *(const f32x4*)(bhh + 160)};
      const f32x4 bin = *(const f32x4*)(bih + 320), bhn = *(const f32x4*)(bhh + 320);
      Frag<T> wi[kHold ? 3 : 1][kHold ? 3 : 1], wh[kHold ? 3 : 1][kHold ? 5 : 1];
      if constexpr (kHold) {
#pragma unroll
        for (int gt = 0; gt < 3; ++gt) {
#pragma unroll
          for (int kc = 0; kc < 3; ++kc) wi[gt][kc] = load_wgt<T>(wih, 10 * gt + wave, 3, kc, lane);
#pragma unroll
          for (int kc = 0; kc < 5; ++kc) wh[gt][kc] = load_wgt<T>(whh, 10 * gt + wave, 5, kc, lane);
        }
      }
      for (int step = 0; step < L; ++step) {
        const int t = d ? L - 1 - step : step, tp = d ? t + 1 : t - 1;
        for (int s0 = 0; s0 < nseq; s0 += 16) {
          const int s = s0 + col, sc = min(s, nseq - 1);
          const int tok = sc * ss + t * ts, tokp = sc * ss + tp * ts;
          f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, ani = ar, anh = ar, hp = ar;
#pragma unroll
          for (int kc = 0; kc < 3; ++kc) {
            const Frag<T> bx = load_act<T, false>(src + tok * kLd + kc * 32 + 8 * g);
            if constexpr (kHold) {
              mfma_frag(ar, wi[0][kc], bx);
              mfma_frag(az, wi[1][kc], bx);
              mfma_frag(ani, wi[2][kc], bx);
            } else {
              mfma_frag(ar, load_wgt<T>(wih, wave, 3, kc, lane), bx);
              mfma_frag(az, load_wgt<T>(wih, 10 + wave, 3, kc, lane), bx);
              mfma_frag(ani, load_wgt<T>(wih, 20 + wave, 3, kc, lane), bx);
            }
          }
          if (step > 0) {
            const float* hrow = big + tokp * kLdBig + d * kTstHid;
#pragma unroll
            for (int kc = 0; kc < 5; ++kc) {
              const Frag<T> bh = load_act<T, false>(hrow + kc * 32 + 8 * g);
              if constexpr (kHold) {
                mfma_frag(ar, wh[0][kc], bh);
                mfma_frag(az, wh[1][kc], bh);
                mfma_frag(anh, wh[2][kc], bh);
              } else {
                mfma_frag(ar, load_wgt<T>(whh, wave, 5, kc, lane), bh);
                mfma_frag(az, load_wgt<T>(whh, 10 + wave, 5, kc, lane), bh);
                mfma_frag(anh, load_wgt<T>(whh, 20 + wave, 5, kc, lane), bh);
              }
            }
            hp = *(const f32x4*)(hrow + wave * 16 + 4 * g);
          }
          f32x4 hn;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float r = sigmoid_f(ar[i] + brz[0][i]);
            const float z = sigmoid_f(az[i] + brz[1][i]);
            const float n = tanhf(ani[i] + bin[i] + r * (anh[i] + bhn[i]));
            hn[i] = (1.0f - z) * n + z * hp[i];
          }
          if (s < nseq) *(f32x4*)(big + tok * kLdBig + d * kTstHid + wave * 16 + 4 * g) = hn;
        }
        __syncthreads();
      }
    }

    // ---- ReLU, linear2, residual, norm2 -> src
    tok_gemm<T, true>(we + kTstELin2, kTstD / 16, 10, big, kLdBig, Nt, att, kLd, ve + kTstVLin2B);
    __syncthreads();
    layer_norm_add(src, src, kLd, att, kLd, ve + kTstVLn2W, ve + kTstVLn2B, Nt);
    __syncthreads();

    // ---- cur += GroupNorm(1, 80, eps 1e-8)(src) over the whole image
    {
      const int n = Nt * kTstD;
      float s = 0.f;
      for (int i = tid; i < n; i += kNT) s += src[(i / kTstD) * kLd + i % kTstD];
      const float mean = block_sum(s, red) / (float)n;
      float q = 0.f;
      for (int i = tid; i < n; i += kNT) {
        const float dlt = src[(i / kTstD) * kLd + i % kTstD] - mean;
        q += dlt * dlt;
      }
      const float rstd = 1.0f / sqrtf(block_sum(q, red) / (float)n + 1e-8f);
      for (int i = tid; i < n; i += kNT) {
        const int c = i % kTstD, o = (i / kTstD) * kLd + c;
        cur[o] += (src[o] - mean) * rstd * ve[kTstVGnW + c] + ve[kTstVGnB + c];
      }
    }
    __syncthreads();
  }

  // ---- output conv + PReLU, rounded to the storage type; per-channel statistics of the rounded values
  tok_gemm<T, false>(wm + kTstWOut, kTstC / 16, 3, cur, kLd, Nt, big, kLdBig, wv + kTstVOutB);
  __syncthreads();
  {
    const float alpha = wv[kTstVOutA];
    T* o = (T*)a.out + (size_t)b * Nt * kTstC;
    for (int i = tid; i < Nt * kTstC; i += kNT) {
      float& v = big[(i / kTstC) * kLdBig + i % kTstC];
      const T r = from_f32<T>(v >= 0.f ? v : alpha * v);
      o[i] = r;
      v = to_f32<T>(r);
    }
  }
  __syncthreads();
  if (a.stats) tile_channel_stats(big, kLdBig, Nt, kTstC, a.stats + (size_t)b * kTstC * 2, 2);
}

template <typename T> __global__ void dt_pack_kernel(const float* nchw, T* nhwc, int C, int P, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;   // over [B][P][C]
  if (i >= total) return;
  const int c = (int)(i % C);
  const int64_t bp = i / C, p = bp % P, b = bp / P;
  nhwc[i] = from_f32<T>(nchw[(b * C + c) * P + p]);
}
template <typename T> __global__ void dt_unpack_kernel(const T* nhwc, float* nchw, int C, int P, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const int64_t bp = i / C, p = bp % P, b = bp / P;
  nchw[(b * C + c) * P + p] = to_f32<T>(nhwc[i]);
}

}  // namespace

size_t dt_lds_bytes() { return sizeof(float) * kLdsFloats; }

hipError_t launch_dual_transformer(int dtype, const DualTransformerArgs& a, int B, hipStream_t s) {
  if (B < 1 || a.dim1 < 1 || a.dim2 < 1 || a.dim1 * a.dim2 > kTstMaxTokens || a.n_tstb < 1) return hipErrorInvalidValue;
  const size_t lds = dt_lds_bytes();
  if (dtype == DT_BF16) hipLaunchKernelGGL((dual_transformer_kernel<bf16_t>), dim3(B), dim3(kNT), lds, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((dual_transformer_kernel<f16_t>), dim3(B), dim3(kNT), lds, s, a);
  else hipLaunchKernelGGL((dual_transformer_kernel<float>), dim3(B), dim3(kNT), lds, s, a);
  return hipGetLastError();
}

hipError_t launch_dt_pack(int dtype, const float* nchw, void* nhwc, int B, int C, int P, hipStream_t s) {
  const int64_t total = (int64_t)B * C * P;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((dt_pack_kernel<bf16_t>), grid, block, 0, s, nchw, (bf16_t*)nhwc, C, P, total);
  else if (dtype == DT_F16) hipLaunchKernelGGL((dt_pack_kernel<f16_t>), grid, block, 0, s, nchw, (f16_t*)nhwc, C, P, total);
  else hipLaunchKernelGGL((dt_pack_kernel<float>), grid, block, 0, s, nchw, (float*)nhwc, C, P, total);
  return hipGetLastError();
}

hipError_t launch_dt_unpack(int dtype, const void* nhwc, float* nchw, int B, int C, int P, hipStream_t s) {
  const int64_t total = (int64_t)B * C * P;
  const dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((dt_unpack_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)nhwc, nchw, C, P, total);
  else if (dtype == DT_F16) hipLaunchKernelGGL((dt_unpack_kernel<f16_t>), grid, block, 0, s, (const f16_t*)nhwc, nchw, C, P, total);
  else hipLaunchKernelGGL((dt_unpack_kernel<float>), grid, block, 0, s, (const float*)nhwc, nchw, C, P, total);
  return hipGetLastError();
}

}  // namespace sddm
