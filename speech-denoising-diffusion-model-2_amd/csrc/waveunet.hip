// Waveunet3 denoiser (reference model/waveunet3.py:314-416 at the arguments of config_waveunet3.json)
// for SDDM.infer (model.py:50-124).  wu_runtime.h holds the layer sequence.
//
// Activations are channels-last [B][L][C] in the compute dtype, so a position's channels are
// contiguous and an MFMA operand fragment (8 channels) is one (bf16 / f16) or two (fp32) 16-byte
// loads.  Every 5-tap Block conv, the 4-tap stride-2 DownsampleLayer conv and the 4-tap stride-2
// transposed UpsampleLayer conv is one launch of wu_conv_kernel (wu_conv_impl.h, shared with
// Waveunet2) under the policy Wu3Conv below: an implicit GEMM over (tap, ci) whose input slab is
// staged through LDS in 32-channel chunks with GroupNorm + SiLU applied once per element on the way
// in, and whose epilogue adds bias, the per-row noise-level constant, the residual and the shortcut,
// stores, and leaves per-wave (sum, sum of squares) partials of what it stored.  The partials are
// plain stores into per-slot cells, reduced in a fixed order by wu_gn_finalize in fp64: the
// statistics of a row do not depend on the batch it sits in.
#include "wu_conv_impl.h"

#include <algorithm>

namespace sddm {

// ---------------- GroupNorm finalize ----------------
// one block per (group, row): thread i sums the cells i, i + 256, ... of its group in fp64, a xor
// butterfly combines the lanes of a wave (every lane ends with the same bits), the four wave sums
// are added in wave order; var = E[x^2] - mean^2 in fp64
__global__ __launch_bounds__(256) void wu_gn_finalize_kernel(WUGnArgs a) {
  __shared__ double red[2][4];
  const int g = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  const int cpg = a.C / a.G, c0 = g * cpg;
  const int items = a.nslots * cpg;
  const float* base = a.stats + (size_t)b * a.nslots * a.C * 2;
  double s = 0.0, ss = 0.0;
  for (int i = lane; i < items; i += 256) {
    const int slot = i / cpg, c = i - slot * cpg;
    const float* e = base + ((size_t)slot * a.C + c0 + c) * 2;
    s += (double)e[0];
    ss += (double)e[1];
  }
  for (int o = 1; o < 64; o <<= 1) {
    s += __shfl_xor(s, o);
    ss += __shfl_xor(ss, o);
  }
  if ((lane & 63) == 0) {
    red[0][lane >> 6] = s;
    red[1][lane >> 6] = ss;
  }
  __syncthreads();
  s = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
  ss = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
  const double n = (double)a.L * cpg;
  const double mean = s / n;
  double var = ss / n - mean * mean;
  var = var > 0.0 ? var : 0.0;
  const double rstd = 1.0 / sqrt(var + (double)a.eps);
  for (int c = lane; c < cpg; c += 256) {
    const double scale = (double)a.gamma[c0 + c] * rstd;
    a.scale[(size_t)b * a.C + c0 + c] = (float)scale;
    a.shift[(size_t)b * a.C + c0 + c] = (float)((double)a.beta[c0 + c] - mean * scale);
  }
}

hipError_t launch_wu_gn_finalize(const WUGnArgs& a, hipStream_t s) {
  if (a.B < 1 || a.G < 1 || a.C % a.G || a.nslots < 1 || a.L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wu_gn_finalize_kernel, dim3(a.G, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------- statistics of the two raw input channels ----------------
__global__ __launch_bounds__(256) void wu_in_stats_kernel(WUInStatsArgs a) {
  __shared__ double red[4][256];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (a.t_dev && b == 0 && tid == 0) *a.t_dev -= 1;   // this step's t
  const float* c = a.cond + (size_t)b * a.L;
  const float* x = a.x + (size_t)b * a.L;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < a.L; i += 256) {
    const double p = (double)c[i], q = (double)x[i];
    v[0] += p; v[1] += p * p; v[2] += q; v[3] += q * q;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) red[k][tid] = v[k];
  __syncthreads();
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int k = 0; k < 4; ++k) red[k][tid] += red[k][tid + o];
    }
    __syncthreads();
  }
  if (tid < 2) {
    const double n = (double)a.L;
    const double mean = red[2 * tid][0] / n;
    double var = red[2 * tid + 1][0] / n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double scale = (double)a.gamma[tid] / sqrt(var + (double)a.eps);
    a.scale[b * 2 + tid] = (float)scale;
    a.shift[b * 2 + tid] = (float)((double)a.beta[tid] - mean * scale);
  }
}

hipError_t launch_wu_in_stats(const WUInStatsArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wu_in_stats_kernel, dim3(a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------- stem: GN(2, 2) + SiLU -> Conv1d(2, 32, 5, padding 2) + noise constant ----------------
hipError_t launch_wu_stem(int dtype, const WUStemArgs& a, hipStream_t s) { return wu_stem_launch<32, true>(dtype, a, s); }

// ---------------- the MFMA convolution: Waveunet3's side of wu_conv_kernel ----------------
// Cin % 32 == 0 and Cout = 16 NCO; input transform GroupNorm + SiLU; the residual paths of the
// kernel; the bias carries the noise constant
struct Wu3Conv {
  using Args = WUConvArgs;
  static constexpr bool kPartial = false, kResidual = true, kSplit = false;
  struct Lds { alignas(16) float sc[128]; alignas(16) float sh[128]; };   // 16-byte aligned: transform reads them as b128
  struct Epi { float lvl; };                           // the row's noise level
  struct Row { float bias[4]; };

  static __device__ __forceinline__ void prologue(const Args&, Lds&, int, int) {}

  template <typename T>
  static __device__ __forceinline__ f32x4 transform(const Args&, const Lds& l, f32x4 v, int, int, int cq) {
    return transform_vec<T>(v, l.sc + cq, l.sh + cq, true);
  }

  static __device__ __forceinline__ Epi epi(const Args& a, int b) { return Epi{a.nw ? wu_level(a.lv, b) : 0.f}; }

  static __device__ __forceinline__ Row row(const Args& a, const Lds&, const Epi& e, int cb, bool) {
    Row r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.bias[i] = a.bias[cb + i] + (a.nw ? a.nw[cb + i] * e.lvl + a.nb[cb + i] : 0.f);
    return r;
  }

  static __device__ __forceinline__ void value(const Epi&, const Row&, float*) {}

  template <typename T, int MODE>
  static hipError_t launch_nco(const Args& a, dim3 grid, hipStream_t s) {
    if constexpr (MODE == WU_CONV3) {
      return hipErrorInvalidValue;                       // Waveunet3 has no 3-tap conv
    } else {
      switch (a.Cout) {
        case 32:
          if (MODE != WU_CONV5) return hipErrorInvalidValue;   // the resampling layers are 64 / 96 / 128 wide
          hipLaunchKernelGGL((wu_conv_kernel<T, WU_CONV5, 2, Wu3Conv>), grid, dim3(256), 0, s, a);
          break;
        case 64: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 4, Wu3Conv>), grid, dim3(256), 0, s, a); break;
        case 96: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 6, Wu3Conv>), grid, dim3(256), 0, s, a); break;
        case 128: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 8, Wu3Conv>), grid, dim3(256), 0, s, a); break;
        default: return hipErrorInvalidValue;
      }
      return hipGetLastError();
    }
  }
};

hipError_t launch_wu_conv(int dtype, const WUConvArgs& a, hipStream_t s) {
  if ((a.mode != WU_CONV5 && a.mode != WU_DOWN4 && a.mode != WU_UP4) || a.B < 1 || a.Lin < 1 || a.Lout < 1) return hipErrorInvalidValue;
  if (a.Cin % 32 || a.Cin < 32 || a.Cin > 128 || a.Cout % 32 || a.Cout < 32 || a.Cout > 128) return hipErrorInvalidValue;
  if ((a.mode == WU_CONV5 && a.Lout != a.Lin) || (a.mode == WU_DOWN4 && a.Lin != 2 * a.Lout) ||
      (a.mode == WU_UP4 && a.Lout != 2 * a.Lin))
    return hipErrorInvalidValue;
  if (a.res_mode < 0 || a.res_mode > 3 || (a.res_mode && a.mode != WU_CONV5)) return hipErrorInvalidValue;
  if ((a.res_mode == 1 && !a.res) || (a.res_mode == 2 && (!a.res || !a.rw || a.RC % 32 || a.RC < 32)) ||
      (a.res_mode == 3 && (!a.cond || !a.x || !a.rw2)))
    return hipErrorInvalidValue;
  if ((a.scale == nullptr) != (a.shift == nullptr) || (a.nw && !a.nb)) return hipErrorInvalidValue;
  if (a.nw && !a.lv.levels && (!a.lv.t_dev || (!a.lv.time_step && !a.lv.table))) return hipErrorInvalidValue;
  return wu_conv_dispatch<Wu3Conv>(dtype, a, s);
}

// ---------------- ConvLayer norm: y = ReLU(GN(raw)) + the statistics of y ----------------
// Block = 64 positions; thread (cq, r) of a (C / 4) x 8 block owns 4 channels of the positions
// r, r + 8, ...; the 8 row partials of a channel are summed in ascending r -- 1 slot per block
template <typename T>
__global__ __launch_bounds__(256) void wu_act_kernel(WUActArgs a) {
  __shared__ float part[8][128][2];
  const int q = a.C / 4, tid = threadIdx.x, cq = tid % q, r = tid / q;
  const int b = blockIdx.y, t0 = blockIdx.x * kWuActTile, c = cq * 4;
  const f32x4 sc = *(const f32x4*)(a.scale + (size_t)b * a.C + c), sh = *(const f32x4*)(a.shift + (size_t)b * a.C + c);
  float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
  for (int p = r; p < kWuActTile; p += 8) {
    const int t = t0 + p;
    if (t >= a.L) break;
    const size_t o = ((size_t)b * a.L + t) * a.C + c;
    const f32x4 x = load4<T>((const T*)a.src + o);
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      v[i] = round_t<T>(fmaxf(x[i] * sc[i] + sh[i], 0.f));
      s[i] += v[i];
      ss[i] += v[i] * v[i];
    }
    store4<T>((T*)a.out + o, v[0], v[1], v[2], v[3]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    part[r][c + i][0] = s[i];
    part[r][c + i][1] = ss[i];
  }
  __syncthreads();
  if (tid < a.C) {
    float ts = 0.f, tss = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      ts += part[k][tid][0];
      tss += part[k][tid][1];
    }
    float* st = a.stats + (((size_t)b * gridDim.x + blockIdx.x) * a.C + tid) * 2;
    st[0] = ts;
    st[1] = tss;
  }
}

hipError_t launch_wu_act(int dtype, const WUActArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1 || a.C % 4 || a.C < 4 || a.C > 128 || !a.stats) return hipErrorInvalidValue;
  const dim3 grid((a.L + kWuActTile - 1) / kWuActTile, a.B), block(a.C / 4 * 8);
  if (dtype == DT_F32) hipLaunchKernelGGL(wu_act_kernel<float>, grid, block, 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(wu_act_kernel<bf16_t>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(wu_act_kernel<f16_t>, grid, block, 0, s, a);
  return hipGetLastError();
}

// ---------------- head: Conv1d(32, 1, 1) + clamp ----------------
template <typename T>
__global__ __launch_bounds__(256) void wu_head_kernel(WUHeadArgs a) {
  const int64_t total = (int64_t)a.B * a.L;
  float w[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) w[i] = a.w[i];
  const float bias = a.bias[0];
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const T* p = (const T*)a.src + i * 32;
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 v = load4<T>(p + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) s += w[q * 4 + e] * v[e];
    }
    a.out[i] = clamp_pm1(s + bias);
  }
}

hipError_t launch_wu_head(int dtype, const WUHeadArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1) return hipErrorInvalidValue;
  const int64_t total = (int64_t)a.B * a.L;
  const dim3 grid((unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 16384)));
  if (dtype == DT_F32) hipLaunchKernelGGL(wu_head_kernel<float>, grid, dim3(256), 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(wu_head_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wu_head_kernel<f16_t>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sddm
