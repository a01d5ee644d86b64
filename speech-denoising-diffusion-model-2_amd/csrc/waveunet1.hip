// Waveunet denoiser (reference model/waveunet.py:358-506 at the arguments of config_waveunet.json:
// twelve levels, 24 ... 288 channels) for SDDM.infer (model.py:50-124).  wu2_runtime.h holds the
// layer sequence, which is Waveunet2's with another table.
//
// The layers are Waveunet2's (waveunet2.hip) with more channels: the convs are launches of
// wu_conv_kernel (wu_conv_impl.h) under the policy Wu1Conv below, which is Waveunet2's input
// transform and epilogue (wu2_conv_policy.h) with kSplit set.  A block then computes one group of
// at most 96 (WU_CONV3: 144) output channels, chosen by blockIdx.z, so its accumulators (NCO <= 6,
// WU_CONV3 <= 9) and, in 16-bit, the weight image it keeps in LDS are no larger than Waveunet2's.
// The policy's sc / sh / enc arrays for 288 channels add 2.3 KB to Waveunet2's LDS: 54.8 KB at most
// (WU_DOWN4, NCO = 6, 16-bit; Waveunet2: 52.5 KB).  The 16-bit instantiations with five or more
// fragments run two blocks per CU by registers, as Waveunet2's do, the smaller ones three or four.
// Every group stages and transforms the input slab again.  The statistics partials [B][slots][C][2] are unchanged: the groups own disjoint channels.
#include "wu2_conv_policy.h"

namespace sddm {

struct Wu1Conv : Wu2ConvBase<WU1ConvArgs, kWu1MaxC, true> {
  template <typename T, int MODE>
  static hipError_t launch_nco(const Args& a, dim3 grid, hipStream_t s) {
    grid.z = (a.Cout + a.gco - 1) / a.gco;
    // fragments per group: 2 ... 6, the FiLM convs (WU_CONV3) up to 9
    switch (a.gco / 16) {
      case 2: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 2, Wu1Conv>), grid, dim3(256), 0, s, a); break;
      case 3: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 3, Wu1Conv>), grid, dim3(256), 0, s, a); break;
      case 4: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 4, Wu1Conv>), grid, dim3(256), 0, s, a); break;
      case 5: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 5, Wu1Conv>), grid, dim3(256), 0, s, a); break;
      case 6: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 6, Wu1Conv>), grid, dim3(256), 0, s, a); break;
      default:
        if constexpr (MODE == WU_CONV3) {
          if (a.gco == 112) hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 7, Wu1Conv>), grid, dim3(256), 0, s, a);
          else if (a.gco == 128) hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 8, Wu1Conv>), grid, dim3(256), 0, s, a);
          else if (a.gco == 144) hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 9, Wu1Conv>), grid, dim3(256), 0, s, a);
          else return hipErrorInvalidValue;
          break;
        } else {
          return hipErrorInvalidValue;
        }
    }
    return hipGetLastError();
  }
};

hipError_t launch_wu1_conv(int dtype, const WU2ConvArgs& a2, hipStream_t s) {
  WU1ConvArgs a{};
  static_cast<WU2ConvArgs&>(a) = a2;
  const hipError_t e = wu2_conv_check(a, kWu1MaxC, kWu1MaxC, 2 * kWu1MaxC);
  if (e != hipSuccess) return e;
  a.gco = wu1_conv_group(a.mode, a.Cout);
  return wu_conv_dispatch<Wu1Conv>(dtype, a, s);
}

}  // namespace sddm
