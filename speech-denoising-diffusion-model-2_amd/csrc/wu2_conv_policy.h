// The Waveunet2 family's side of wu_conv_kernel (wu_conv_impl.h): the input transform and the
// epilogue that Waveunet2 (waveunet2.hip) and the 12-level Waveunet (waveunet1.hip) share.  Each
// network derives its policy from Wu2ConvBase and adds launch_nco, the choice among its
// instantiations.
#pragma once
#include "wu2_kernels.h"
#include "wu_conv_impl.h"

namespace sddm {

// ReLU(GroupNorm) and the FiLM (fs * v + fh) of one 16-byte unit, rounded to T once
template <typename T>
__device__ __forceinline__ f32x4 wu2_transform(f32x4 raw, const float* sc, const float* sh, bool film, f32x4 fs, f32x4 fh) {
  constexpr int VE = 16 / (int)sizeof(T);
  typedef T vec __attribute__((ext_vector_type(VE)));
  vec v = __builtin_bit_cast(vec, raw);
  const vec s = __builtin_bit_cast(vec, fs), h = __builtin_bit_cast(vec, fh);
#pragma unroll
  for (int j = 0; j < VE; ++j) {
    float y = fmaxf(to_f32<T>(v[j]) * sc[j] + sh[j], 0.f);
    if (film) y = to_f32<T>(s[j]) * y + to_f32<T>(h[j]);
    v[j] = from_f32<T>(y);
  }
  return __builtin_bit_cast(f32x4, v);
}

// Cin, Cout multiples of 8; input transform GroupNorm + ReLU + FiLM; no residual paths; the
// epilogue value is acc + bias, then with enc_dim > 0 leaky_relu(0.2) + the level's encoding
//   ARGS   WU2ConvArgs, or a struct derived from it (SPLIT: with gco, wu_conv_impl.h)
//   MAXC   the widest Cin (scale / shift) and enc_dim the policy's LDS arrays hold
template <typename ARGS, int MAXC, bool SPLIT>
struct Wu2ConvBase {
  using Args = ARGS;
  static constexpr bool kPartial = true, kResidual = false, kSplit = SPLIT;
  struct Lds { alignas(16) float sc[MAXC]; alignas(16) float sh[MAXC]; alignas(16) float enc[MAXC]; };   // 16-byte aligned: read as b128
  struct Epi { int enc; };                             // enc_dim > 0 (an int: a one-byte struct ends up in LDS)
  struct Row { float bias[4], e4[4]; };

  // PositionalEncoding (waveunet2.py:34-39), fp32 as torch, accurate sinf / cosf
  static __device__ __forceinline__ void prologue(const Args& a, Lds& l, int b, int tid) {
    if constexpr (MAXC <= 256) {
      if (a.enc_dim > 0 && tid < a.enc_dim) {
        const int half = a.enc_dim / 2, k = tid < half ? tid : tid - half;
        const float arg = wu_level(a.lv, b) * expf(-9.210340371976184f * ((float)k / (float)half));
        l.enc[tid] = tid < half ? sinf(arg) : cosf(arg);
      }
    } else {                               // more channels than threads
      for (int i = tid; i < a.enc_dim; i += 256) {
        const int half = a.enc_dim / 2, k = i < half ? i : i - half;
        const float arg = wu_level(a.lv, b) * expf(-9.210340371976184f * ((float)k / (float)half));
        l.enc[i] = i < half ? sinf(arg) : cosf(arg);
      }
    }
  }

  template <typename T>
  static __device__ __forceinline__ f32x4 transform(const Args& a, const Lds& l, f32x4 v, int b, int pos, int cq) {
    const bool film = a.film != nullptr;
    f32x4 fs = f32x4{0.f, 0.f, 0.f, 0.f}, fh = fs;
    if (film) {
      const T* fp = (const T*)a.film + ((size_t)b * a.Lin + pos) * (2 * a.Cin) + cq;
      fh = *(const f32x4*)fp;
      fs = *(const f32x4*)(fp + a.Cin);
    }
    return wu2_transform<T>(v, l.sc + cq, l.sh + cq, film, fs, fh);
  }

  static __device__ __forceinline__ Epi epi(const Args& a, int) { return Epi{a.enc_dim > 0 ? 1 : 0}; }

  static __device__ __forceinline__ Row row(const Args& a, const Lds& l, const Epi& e, int cb, bool okc) {
    Row r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      r.bias[i] = okc ? a.bias[cb + i] : 0.f;
      r.e4[i] = e.enc && okc ? l.enc[cb + i] : 0.f;
    }
    return r;
  }

  static __device__ __forceinline__ void value(const Epi& e, const Row& r, float* v) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (e.enc) v[i] = (v[i] > 0.f ? v[i] : 0.2f * v[i]) + r.e4[i];
  }
};

}  // namespace sddm
