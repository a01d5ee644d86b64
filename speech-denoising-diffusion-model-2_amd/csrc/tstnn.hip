// TSTNN (reference model/tstnn.py:216-299) for gfx950: the framing first kernel (inp_conv +
// LayerNorm(512) + PReLU), the wide-row MFMA convolution (DenseBlock depth 4, enc_conv1, dec_conv1)
// with its LayerNorm + PReLU epilogue, the gated mask and out_conv + overlap-add.  The
// Dual_Transformer between them is caunet.hip's.
//
// As in caunet.hip every matrix product is an MFMA with the weights as A fragments read from global
// memory and the activations as B fragments; in a 16-bit context activations are rounded where a
// kernel stores them; LayerNorm, tanh, sigmoid, PReLU and ReLU are fp32.  No atomics and no block
// waits for another: a block owns one whole row (frame), every reduction runs in an order fixed by
// the block shape, and a row's result does not depend on the batch it is in.
#include "tstnn.h"

#include "cau_frag.h"

namespace sddm {
namespace {

constexpr int kTstnnLdsC = 72;   // channel stride of a staged pixel: 64 + 8, as caunet.hip's

// sum over the 16 lanes that share a lane group (the positions of one tile)
__device__ __forceinline__ f32x4 tstnn_cols_sum(f32x4 s) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float v = s[i];
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 8);
    s[i] = v;
  }
  return s;
}

// sum of each of NV values over the block's 256 threads (every thread gets the sums)
template <int NV> __device__ __forceinline__ void tstnn_block_sum(float (&v)[NV], float (*red)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    for (int o = 32; o >= 1; o >>= 1) v[k] += __shfl_xor(v[k], o);
  }
  __syncthreads();                                               // red's readers of the previous call
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; ++k) red[k][wave] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = (red[k][0] + red[k][1]) + (red[k][2] + red[k][3]);
}

// ---------------------------------------------------------------------------------------------
// first kernel: one block per frame.  Thread (p0 = tid >> 4, cq = tid & 15) stores channels
// 4 cq .. 4 cq + 3 of positions p0 + 16 k, so 16 lanes write one position's 64 channels
// ---------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void tstnn_first_kernel(TstnnFirstArgs a) {
  __shared__ float su[kTstnnF], sv[kTstnnF], red[3][4];
  const int tid = threadIdx.x, row = blockIdx.x;
  if (a.t_dev && row == 0 && tid == 0) *a.t_dev -= 1;            // this step's t
  const int b = row / a.F, f = row - b * a.F;
  const float* cu = a.cond + (size_t)b * a.N + (size_t)f * kTstnnStride;
  const float* cv = a.x + (size_t)b * a.N + (size_t)f * kTstnnStride;
  float u[2] = {cu[tid], cu[tid + 256]}, v[2] = {cv[tid], cv[tid + 256]};
  float m[2] = {u[0] + u[1], v[0] + v[1]};
  tstnn_block_sum<2>(m, red);
  const float mu = m[0] * (1.0f / kTstnnF), mv = m[1] * (1.0f / kTstnnF);
  float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    u[k] -= mu; v[k] -= mv;
    su[tid + 256 * k] = u[k]; sv[tid + 256 * k] = v[k];
    q[0] += u[k] * u[k]; q[1] += u[k] * v[k]; q[2] += v[k] * v[k];
  }
  tstnn_block_sum<3>(q, red);                                      // its barriers also publish su, sv
  const int c = (tid & 15) * 4, p0 = tid >> 4;
  float w0[4], w1[4], rstd[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w0[j] = a.w[(c + j) * 2]; w1[j] = a.w[(c + j) * 2 + 1];
    const float var = (w0[j] * w0[j] * q[0] + 2.0f * w0[j] * w1[j] * q[1] + w1[j] * w1[j] * q[2]) * (1.0f / kTstnnF);
    rstd[j] = 1.0f / sqrtf(fmaxf(var, 0.f) + 1e-5f);
  }
  const f32x4 al = *(const f32x4*)(a.alpha + c);
  T* out = (T*)a.out + (size_t)row * kTstnnF * 64 + c;
  for (int w = p0; w < kTstnnF; w += 16) {
    const float du = su[w], dv = sv[w], lw = a.lnw[w], lb = a.lnb[w];
    float y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float t = (w0[j] * du + w1[j] * dv) * rstd[j] * lw + lb;
      y[j] = t >= 0.f ? t : al[j] * t;
    }
    store4<T>(out + (size_t)w * 64, y[0], y[1], y[2], y[3]);
  }
}

// ---------------------------------------------------------------------------------------------
// the convolution: one block per row of Wc = 16 NPT positions; wave j owns output channels
// 16 j .. 16 j + 15 (of each sub-pixel phase) at all of them, so the row's LayerNorm statistics are
// sums over the wave's own accumulators and 16 lanes.  One (source, kh) slab of the input row tap kh
// reads goes through LDS at a time, Win + 2 pixels wide (a zero column each side); a slab above the
// image is all zeros and is skipped.  The six weight fragments of a slab are read before it is staged
// ---------------------------------------------------------------------------------------------
template <typename T, int MODE, int NPT> __global__ __launch_bounds__(256) void tstnn_conv_kernel(TstnnConvArgs a) {
  constexpr int NR = MODE == CAU_UP ? 2 : 1, KH = MODE == CAU_DENSE ? 2 : 1;
  constexpr int Wc = 16 * NPT, Win = MODE == CAU_DOWN ? 2 * Wc : Wc, Wout = NR * Wc, WP = Win + 2;
  constexpr int PS = MODE == CAU_DOWN ? 2 : 1;                   // input pixels per conv position
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int F = a.F, row = blockIdx.x, b = row / F, h = row - b * F;
  f32x4 acc[NR][NPT];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) acc[r][pt] = f32x4{0.f, 0.f, 0.f, 0.f};

  extern __shared__ __align__(16) char tstnn_smem[];
  T* tile = (T*)tstnn_smem;
  const T* wgt = (const T*)a.w;
  const int KS = a.nsrc * KH * 3 * 2;
  const int lb = PS * col * kTstnnLdsC + 8 * g;
  bool staged = false;
  for (int s = 0; s < a.nsrc; ++s) {
    const T* sp = (const T*)a.src[s];
    for (int kh = 0; kh < KH; ++kh) {
      const int hin = MODE == CAU_DENSE ? h - (1 - kh) * a.dil : h;
      if (hin < 0) continue;                                     // the causal padding: nothing to add
      const int ks0 = (s * KH + kh) * 6;
      Frag<T> wa[6][NR];
#pragma unroll
      for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int r = 0; r < NR; ++r) wa[k][r] = load_wgt<T>(wgt, r * 4 + wave, KS, ks0 + k, lane);
      if (staged) __syncthreads();                               // the previous slab's readers
      const T* rowp = sp + ((size_t)b * F + hin) * Win * 64;
      for (int i = threadIdx.x; i < WP * 8; i += 256) {
        const int c8 = (i & 7) * 8, pix = i >> 3, win = pix - 1;
        const Frag<T> v = (win >= 0 && win < Win) ? load_t<T>(rowp + (size_t)win * 64 + c8) : zero_frag<T>();
        *(Frag<T>*)(tile + (size_t)pix * kTstnnLdsC + c8) = v;
      }
      __syncthreads();
      staged = true;
#pragma unroll
      for (int kw = 0; kw < 3; ++kw)
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
          const T* tap = tile + kw * kTstnnLdsC + lb + kc * 32;
#pragma unroll
          for (int pt = 0; pt < NPT; ++pt) {
            const Frag<T> bx = *(const Frag<T>*)(tap + pt * (16 * PS * kTstnnLdsC));
#pragma unroll
            for (int r = 0; r < NR; ++r) mfma_frag(acc[r][pt], wa[kw * 2 + kc][r], bx);
          }
        }
    }
  }

  // ---- + bias, LayerNorm over the row's Wout outputs (eps 1e-5, two passes), PReLU, store
  const float inv = 1.0f / (float)Wout;
  const int co = wave * 16 + 4 * g;
  f32x4 sm = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const f32x4 bias = *(const f32x4*)(a.bias + r * 64 + co);
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) { acc[r][pt] += bias; sm += acc[r][pt]; }
  }
  const f32x4 mean = tstnn_cols_sum(sm) * inv;
  f32x4 sq = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int pt = 0; pt < NPT; ++pt) { acc[r][pt] -= mean; sq += acc[r][pt] * acc[r][pt]; }
  sq = tstnn_cols_sum(sq);
  f32x4 rstd;
#pragma unroll
  for (int i = 0; i < 4; ++i) rstd[i] = 1.0f / sqrtf(sq[i] * inv + 1e-5f);
  const f32x4 alpha = *(const f32x4*)(a.alpha + co);
  T* out = (T*)a.out + (size_t)row * Wout * 64 + co;
#pragma unroll
  for (int pt = 0; pt < NPT; ++pt) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int wo = NR * (pt * 16 + col) + r;
      const float lw_ = a.lnw[wo], lb_ = a.lnb[wo];
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = acc[r][pt][i] * rstd[i] * lw_ + lb_;
        y[i] = v >= 0.f ? v : alpha[i] * v;
      }
      store4<T>(out + (size_t)wo * 64, y[0], y[1], y[2], y[3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// the gated mask: a block is four waves of 16 tokens
// ---------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void tstnn_gate_kernel(TstnnGateArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int64_t tok = (int64_t)blockIdx.x * 64 + wave * 16 + col;
  const bool valid = tok < a.tokens;
  const size_t gt = (size_t)(valid ? tok : a.tokens - 1);
  const T* w1 = (const T*)a.w1;
  const T* w2 = (const T*)a.w2;
  const T* wm = (const T*)a.wm;
  f32x4 t[4], s[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) t[nt] = s[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kc = 0; kc < 2; ++kc) {
    const Frag<T> by = load_t<T>((const T*)a.y + gt * 64 + kc * 32 + 8 * g);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      mfma_frag(t[nt], load_wgt<T>(w1, nt, 2, kc, lane), by);
      mfma_frag(s[nt], load_wgt<T>(w2, nt, 2, kc, lane), by);
    }
  }
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int c = nt * 16 + 4 * g;
    const f32x4 b1 = *(const f32x4*)(a.b1 + c), b2 = *(const f32x4*)(a.b2 + c);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[nt][i] = tanhf(t[nt][i] + b1[i]) * sigmoid_f(s[nt][i] + b2[i]);
  }
  // lane (g, col) holds the gate's channels 16 nt + 4 g + i: K slots 8 g + j of chunk kc are tiles
  // 2 kc (j < 4) and 2 kc + 1 (j >= 4), the order wm's fragments were packed in (tstnn_gate_k)
  const Frag<T> bg[2] = {frag_from_f32<T>(t[0], t[1]), frag_from_f32<T>(t[2], t[3])};
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const int c = nt * 16 + 4 * g;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) mfma_frag(m, load_wgt<T>(wm, nt, 2, kc, lane), bg[kc]);
    m += *(const f32x4*)(a.bm + c);
    const f32x4 x = load4<T>((const T*)a.x1 + gt * 64 + c);
    if (valid) store4<T>((T*)a.out + gt * 64 + c, x[0] * fmaxf(m[0], 0.f), x[1] * fmaxf(m[1], 0.f), x[2] * fmaxf(m[2], 0.f), x[3] * fmaxf(m[3], 0.f));
  }
}

template <typename T> __global__ __launch_bounds__(256) void tstnn_final_kernel(TstnnFinalArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;    // over [B][N]
  if (i >= (int64_t)a.B * a.N) return;
  const int64_t b = i / a.N, n = i - b * a.N;
  const int f1 = (int)(n / kTstnnStride), wlo = (int)(n % kTstnnStride);
  float out = 0.f;
  // overlapAdd adds the frames in ascending order (tstnn.py:37-39): frame f1 - 1, then f1
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int f = f1 - 1 + k, w = k ? wlo : wlo + kTstnnStride;
    if (f < 0 || f >= a.F) continue;
    const T* p = (const T*)a.src + ((b * a.F + f) * kTstnnF + w) * 64;
    float s = a.bias[0];
    for (int c = 0; c < 64; c += 4) {
      const f32x4 v = load4<T>(p + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += a.w[c + j] * v[j];
    }
    out += s;
  }
  a.out[i] = out;
}

template <typename T, int MODE, int NPT> hipError_t tstnn_conv_launch(const TstnnConvArgs& a, size_t lds, hipStream_t s) {
  hipLaunchKernelGGL((tstnn_conv_kernel<T, MODE, NPT>), dim3(a.B * a.F), dim3(256), lds, s, a);
  return hipGetLastError();
}

template <typename T> hipError_t tstnn_conv_run(const TstnnConvArgs& a, hipStream_t s) {
  const int Win = a.mode == CAU_DOWN ? 2 * a.Wc : a.Wc;
  const size_t lds = sizeof(T) * (size_t)(Win + 2) * kTstnnLdsC;
  int dev = 0, cap = 0;                                          // refuse a slab the device's LDS does not hold
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) return e;
  if (lds > (size_t)cap) return hipErrorInvalidValue;
  if (a.mode == CAU_DOWN) return tstnn_conv_launch<T, CAU_DOWN, 16>(a, lds, s);
  if (a.mode == CAU_UP) return tstnn_conv_launch<T, CAU_UP, 16>(a, lds, s);
  if (a.Wc == 256) return tstnn_conv_launch<T, CAU_DENSE, 16>(a, lds, s);
  return tstnn_conv_launch<T, CAU_DENSE, 32>(a, lds, s);
}

bool tstnn_frames_ok(int B, int F, int64_t N) {
  return B >= 1 && F >= 1 && (int64_t)B * F <= ((int64_t)1 << 21) && N == kTstnnF + kTstnnStride * (int64_t)(F - 1);
}

}  // namespace

hipError_t launch_tstnn_first(int dtype, const TstnnFirstArgs& a, hipStream_t s) {
  if (!tstnn_frames_ok(a.B, a.F, a.N)) return hipErrorInvalidValue;
  const dim3 grid(a.B * a.F), blk(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((tstnn_first_kernel<bf16_t>), grid, blk, 0, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((tstnn_first_kernel<f16_t>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((tstnn_first_kernel<float>), grid, blk, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tstnn_conv(int dtype, const TstnnConvArgs& a, hipStream_t s) {
  if (a.B < 1 || a.F < 1 || (int64_t)a.B * a.F > ((int64_t)1 << 21)) return hipErrorInvalidValue;   // 32-bit row indices
  if (a.mode < CAU_DENSE || a.mode > CAU_UP || a.nsrc < 1 || a.nsrc > 4) return hipErrorInvalidValue;
  if (a.mode == CAU_DENSE ? (a.dil < 1 || (a.Wc != 256 && a.Wc != 512)) : (a.nsrc != 1 || a.Wc != 256)) return hipErrorInvalidValue;
  if (dtype == DT_BF16) return tstnn_conv_run<bf16_t>(a, s);
  if (dtype == DT_F16) return tstnn_conv_run<f16_t>(a, s);
  return tstnn_conv_run<float>(a, s);
}

hipError_t launch_tstnn_gate(int dtype, const TstnnGateArgs& a, hipStream_t s) {
  if (a.tokens < 1 || a.tokens > ((int64_t)1 << 36)) return hipErrorInvalidValue;   // the grid stays below 2^31
  const dim3 grid((unsigned)((a.tokens + 63) / 64)), blk(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((tstnn_gate_kernel<bf16_t>), grid, blk, 0, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((tstnn_gate_kernel<f16_t>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((tstnn_gate_kernel<float>), grid, blk, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_tstnn_final(int dtype, const TstnnFinalArgs& a, hipStream_t s) {
  if (!tstnn_frames_ok(a.B, a.F, a.N)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)a.B * a.N;
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((tstnn_final_kernel<bf16_t>), grid, blk, 0, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((tstnn_final_kernel<f16_t>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((tstnn_final_kernel<float>), grid, blk, 0, s, a);
  return hipGetLastError();
}

}  // namespace sddm
