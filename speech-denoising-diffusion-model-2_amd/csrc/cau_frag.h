// Fragment helpers shared by caunet.hip and tstnn.hip: a Frag<T> from and to fp32, a token's eight
// channels and a weight fragment of caunet.h's layout from global memory.
#pragma once
#include "conv_common.h"

namespace sddm {
namespace {

template <typename T> __device__ __forceinline__ Frag<T> zero_frag() {
  if constexpr (sizeof(T) == 4) {
    return {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  } else {
    Frag<T> f;
#pragma unroll
    for (int j = 0; j < 8; ++j) f.v[j] = (T)0.f;
    return f;
  }
}
// eight fp32 values -> a fragment (rounded to T: where an activation enters an MFMA)
template <typename T> __device__ __forceinline__ Frag<T> frag_from_f32(f32x4 lo, f32x4 hi) {
  if constexpr (sizeof(T) == 4) {
    return {lo, hi};
  } else {
    Frag<T> f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { f.v[j] = (T)lo[j]; f.v[4 + j] = (T)hi[j]; }
    return f;
  }
}
template <typename T> __device__ __forceinline__ void frag_to_f32(const Frag<T>& f, f32x4& lo, f32x4& hi) {
  if constexpr (sizeof(T) == 4) {
    lo = f.lo; hi = f.hi;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { lo[j] = (float)f.v[j]; hi[j] = (float)f.v[4 + j]; }
  }
}
template <typename T> __device__ __forceinline__ Frag<T> load_t(const T* p) { return load_frag<T>((const char*)p); }
template <typename T> __device__ __forceinline__ Frag<T> load_wgt(const T* w, int nt, int KC, int kc, int lane) {
  return load_frag<T>((const char*)(w + ((size_t)(nt * KC + kc) * 64 + lane) * 8));
}
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace
}  // namespace sddm
