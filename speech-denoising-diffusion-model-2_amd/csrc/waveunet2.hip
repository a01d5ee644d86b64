// Waveunet2 denoiser (reference model/waveunet2.py:226-324 at the arguments of config_waveunet2.json)
// for SDDM.infer (model.py:50-124).  wu2_runtime.h holds the layer sequence.
//
// Activations are channels-last [B][L][C] in the compute dtype at the true C (24 / 48 / 72 / 96), so
// an MFMA operand fragment (8 channels) is one (bf16 / f16) or two (fp32) 16-byte loads.  Every
// ConvLayer stores its raw conv output and (sum, sum of squares) partials of it; its GroupNorm +
// ReLU -- and on the way up the per-position FiLM -- is applied by the consumer while it stages its
// input slab, once per element.  The convs are launches of wu_conv_kernel (wu_conv_impl.h, shared
// with Waveunet3) under the policy Wu2Conv below.  The channel counts are no multiples of the MFMA K
// of 32 or of the 16 rows of a fragment: the policy sets kPartial, so the last 32-channel chunk of
// the input and the last 16-row fragment of the output are zero-filled where they are staged, never
// in memory, and stores and statistics are masked to the true Cout.
#include "wu2_conv_policy.h"

#include <algorithm>

namespace sddm {

// ---------------- stem: Conv1d(2, 24, 5, padding 2) on the two raw fp32 sources ----------------
hipError_t launch_wu2_stem(int dtype, const WUStemArgs& a, hipStream_t s) { return wu_stem_launch<kWu2StemC, false>(dtype, a, s); }

// ---------------- the MFMA convolution: Waveunet2's side of wu_conv_kernel ----------------
// Wu2ConvBase (wu2_conv_policy.h): Cin, Cout multiples of 8; input transform GroupNorm + ReLU + FiLM;
// no residual paths; the epilogue value is acc + bias, then with enc_dim > 0 leaky_relu(0.2) + the
// level's encoding.  Every launch holds the whole Cout in one block
struct Wu2Conv : Wu2ConvBase<WU2ConvArgs, 96, false> {
  template <typename T, int MODE>
  static hipError_t launch_nco(const Args& a, dim3 grid, hipStream_t s) {
    // fragments per launch: ConvLayers 24 / 48 / 72 / 96 -> 2 / 3 / 5 / 6 (the resampling layers are 48 / 72 / 96
    // wide), the FiLM output_conv 48 / 96 / 144 -> 3 / 6 / 9
    switch ((a.Cout + 15) / 16) {
      case 2:
        if constexpr (MODE == WU_CONV5 || MODE == WU_CONV3) {
          hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 2, Wu2Conv>), grid, dim3(256), 0, s, a);
          break;
        } else {
          return hipErrorInvalidValue;
        }
      case 3: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 3, Wu2Conv>), grid, dim3(256), 0, s, a); break;
      case 5: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 5, Wu2Conv>), grid, dim3(256), 0, s, a); break;
      case 6: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 6, Wu2Conv>), grid, dim3(256), 0, s, a); break;
      case 9:
        if constexpr (MODE == WU_CONV3) {
          hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 9, Wu2Conv>), grid, dim3(256), 0, s, a);
          break;
        } else {
          return hipErrorInvalidValue;
        }
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
};

hipError_t launch_wu2_conv(int dtype, const WU2ConvArgs& a, hipStream_t s) {
  const hipError_t e = wu2_conv_check(a, 96, 144, 144);
  if (e != hipSuccess) return e;
  return wu_conv_dispatch<Wu2Conv>(dtype, a, s);
}

// ---------------- head: Conv1d(24, 1, 1) of ReLU(GN(raw)) + clamp ----------------
template <typename T>
__global__ __launch_bounds__(256) void wu2_head_kernel(WU2HeadArgs a) {
  constexpr int C = kWu2StemC;
  __shared__ float sc[C], sh[C], w[C];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < C) {
    sc[tid] = a.scale[b * C + tid];
    sh[tid] = a.shift[b * C + tid];
    w[tid] = a.w[tid];
  }
  __syncthreads();
  const int t = blockIdx.x * 256 + tid;
  if (t >= a.L) return;
  const size_t i = (size_t)b * a.L + t;
  const T* p = (const T*)a.src + i * C;
  float s = 0.f;
#pragma unroll
  for (int q = 0; q < C / 4; ++q) {
    const f32x4 v = load4<T>(p + q * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += w[q * 4 + e] * fmaxf(v[e] * sc[q * 4 + e] + sh[q * 4 + e], 0.f);
  }
  a.out[i] = clamp_pm1(s + a.bias[0]);
}

hipError_t launch_wu2_head(int dtype, const WU2HeadArgs& a, hipStream_t s) {
  if (a.B < 1 || a.B > 65535 || a.L < 1 || !a.scale || !a.shift) return hipErrorInvalidValue;
  const dim3 grid((a.L + 255) / 256, a.B);
  if (dtype == DT_F32) hipLaunchKernelGGL(wu2_head_kernel<float>, grid, dim3(256), 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(wu2_head_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wu2_head_kernel<f16_t>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace sddm
