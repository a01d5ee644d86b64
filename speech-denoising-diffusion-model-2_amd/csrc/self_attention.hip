// Spatial self-attention of UNetModified (reference model/UNetModified.py:140-169) for gfx950, wave64.
//
//   attn_qkv    GroupNorm of the input finalized from the producer's per-tile statistics (no SiLU), then
//               [P x C] . [C x 3C] on MFMA into the scratch tensor qkv [B][P][3C]
//   attn_core   one workgroup per (image, query tile): K / V streamed from qkv in tiles of 32 keys,
//               S = Q K^T, the scale log2(e) / sqrt(C) folded into exp2, running maximum and sum in
//               fp32, O rescaled by 2^((m_old - m_new) scale) at every tile, O += P V; then O / sum, the
//               1x1 out conv, bias, + input, the store and the GroupNorm statistics of the fp32 results
//
// Every matrix product is the 16x16 MFMA of conv_common.h: A rows on lane & 15, B columns on lane & 15,
// 8 K elements per lane (K = 8 (lane >> 4) + j), D[row 4 (lane >> 4) + i][column lane & 15].  float32
// runs MFMA 16x16x4 f32: true fp32 products.  The products are laid out transposed, S^T = K Q^T and
// O^T = V^T P^T, so that a lane's accumulators of S^T (keys 4 g + i of two 16-key tiles, one query) are
// the B operand of the next product as they stand: K index 8 g + j stands for key 16 (j / 4) + 4 g + j % 4
// of the tile, and V^T is staged in LDS in that key order.
//
// What a 16-bit context rounds to 16 bits: the normalized input, the stored q / k / v, the
// probabilities where they enter P V (the running sum adds the unrounded fp32 values), O before the out
// conv, the weights and the stored result.  Scores, maximum, sum, O's accumulation, the out conv's
// accumulation, bias, residual and statistics are fp32.
//
// Partial tiles: query rows and key rows past the end are zero in LDS, masked keys score -inf (every
// key tile starts inside the image, so a tile's maximum is finite), stores are guarded.  Nothing is
// padded in memory.  All combination orders are fixed: a row's result depends on that row alone.
#include "sddm_common.h"
#include "self_attention.h"
#include "conv_common.h"

namespace sddm {

typedef unsigned int au32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// attn_qkv: grid (ceil(P / 64), C / 32, B); a block computes 64 positions x 96 of the 3C outputs
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_qkv_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = (int)sizeof(T);
  const int C = a.C, P = a.P, KC = C / 32;
  const int p0 = blockIdx.x * 64, nz = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, wv = tid >> 6;
  float* sc = (float*)smem;
  float* sh = sc + C;
  char* xs = smem + (size_t)C * 8;
  const int ld = C * ES + 16;
  const GNFuse gf{a.gst, a.gtiles, a.gntile, nullptr, 0, 0, a.gamma, a.beta, a.groups, a.eps};
  gn_fused_prologue(gf, b, C, 0, sc, sh);
  __syncthreads();
  const T* x = (const T*)a.x + (size_t)b * P * C;
  const int c4n = C / 4;
  for (int i = tid; i < 64 * c4n; i += 256) {
    const int r = i / c4n, c4 = (i - r * c4n) * 4;
    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
    if (p0 + r < P) {
      v = load4<T>(x + (size_t)(p0 + r) * C + c4);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = v[j] * sc[c4 + j] + sh[c4 + j];
    }
    store4<T>((T*)(xs + (size_t)r * ld) + c4, v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  const int q = wv * 16 + (lane & 15);
  const char* brow = xs + (size_t)q * ld + g * 8 * ES;
  const T* wf = (const T*)a.wqkv_f + (size_t)lane * 8;
  T* o = (T*)a.qkv + ((size_t)b * P + p0 + q) * 3 * C;
  for (int nf = 0; nf < 6; ++nf) {
    const int nt = nz * 6 + nf;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = 0; kc < KC; ++kc)
      mfma_frag(acc, load_frag<T>((const char*)(wf + ((size_t)nt * KC + kc) * 512)), load_frag<T>(brow + kc * 32 * ES));
    if (p0 + q < P) store4<T>(o + nt * 16 + 4 * g, acc[0], acc[1], acc[2], acc[3]);
  }
}

// ---------------------------------------------------------------------------------------------
// attn_core: grid (P / QT, B), 4 waves; wave w owns queries 16 w .. 16 w + 15 of the tile
// ---------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ Frag<T> prob_frag(f32x4 a, f32x4 b);
template <> __device__ __forceinline__ Frag<float> prob_frag<float>(f32x4 a, f32x4 b) { return {a, b}; }
template <> __device__ __forceinline__ Frag<bf16_t> prob_frag<bf16_t>(f32x4 a, f32x4 b) {
  return {bf16x8{(bf16_t)a[0], (bf16_t)a[1], (bf16_t)a[2], (bf16_t)a[3], (bf16_t)b[0], (bf16_t)b[1], (bf16_t)b[2], (bf16_t)b[3]}};
}
template <> __device__ __forceinline__ Frag<f16_t> prob_frag<f16_t>(f32x4 a, f32x4 b) {
  return {f16x8{(f16_t)a[0], (f16_t)a[1], (f16_t)a[2], (f16_t)a[3], (f16_t)b[0], (f16_t)b[1], (f16_t)b[2], (f16_t)b[3]}};
}

template <typename T, int CF> struct AttnLds {
  static constexpr int ES = (int)sizeof(T), C = 32 * CF;
  static constexpr int LDQ = C * ES + 16;                // bytes per row of Q / O and of K
  static constexpr int LDV = kAttnKeyTile * ES + 16;     // bytes per channel row of V^T
  static constexpr int LDT = C + 4;                      // floats per row of the statistics tile
  static constexpr int kQ = 0;
  static constexpr int kK = kAttnQueryTile * LDQ;
  static constexpr int kV = kK + kAttnKeyTile * LDQ;
  static constexpr int kvBytes = kAttnKeyTile * LDQ + C * LDV, tileBytes = kAttnQueryTile * LDT * 4;
  static constexpr int total = kK + (kvBytes > tileBytes ? kvBytes : tileBytes);
};

template <typename T, int CF>
__global__ __launch_bounds__(256) void attn_core_kernel(AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef AttnLds<T, CF> L;
  constexpr int ES = L::ES, C = L::C, NF = 2 * CF, LDQ = L::LDQ, LDV = L::LDV, LDT = L::LDT;
  constexpr int U = C * ES / 16;       // 16-byte units per row of q, k or v
  constexpr int VE = 16 / ES;
  typedef T tvec __attribute__((ext_vector_type(VE)));
  const int P = a.P, QT = a.QT;
  const int tile = blockIdx.x, b = blockIdx.y, q0 = tile * QT;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, wv = tid >> 6;
  char* Qs = smem + L::kQ;
  char* Ks = smem + L::kK;
  char* Vt = smem + L::kV;
  float* tl = (float*)(smem + L::kK);
  const char* qkv = (const char*)a.qkv + (size_t)b * P * 3 * C * ES;
  const au32x4 zero4 = au32x4{0u, 0u, 0u, 0u};

  for (int i = tid; i < kAttnQueryTile * U; i += 256) {
    const int r = i / U, u = i - r * U;
    const au32x4 v = r < QT ? *(const au32x4*)(qkv + (size_t)(q0 + r) * 3 * C * ES + u * 16) : zero4;
    *(au32x4*)(Qs + r * LDQ + u * 16) = v;
  }
  const int qrow = wv * 16 + (lane & 15);
  f32x4 O[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) O[f] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const float sl = a.scale_log2;

  for (int kbase = 0; kbase < P; kbase += kAttnKeyTile) {
    __syncthreads();                   // Q staged; the previous tile's K / V^T reads are done
    for (int i = tid; i < kAttnKeyTile * U; i += 256) {
      const int r = i / U, u = i - r * U;
      const bool ok = kbase + r < P;
      const char* src = qkv + (size_t)(kbase + r) * 3 * C * ES + u * 16;
      const au32x4 kv = ok ? *(const au32x4*)(src + C * ES) : zero4;
      const au32x4 vv = ok ? *(const au32x4*)(src + 2 * C * ES) : zero4;
      *(au32x4*)(Ks + r * LDQ + u * 16) = kv;
      // key r of the tile sits at K index 8 ((r % 16) / 4) + 4 (r / 16) + r % 4 of V^T's rows
      const int pr = 8 * ((r & 15) >> 2) + 4 * (r >> 4) + (r & 3);
      const tvec e = __builtin_bit_cast(tvec, vv);
#pragma unroll
      for (int j = 0; j < VE; ++j) *(T*)(Vt + (u * VE + j) * LDV + pr * ES) = e[j];
    }
    __syncthreads();
    // S^T = K Q^T: keys 4 g + i (s0) and 16 + 4 g + i (s1) of the tile, query lane & 15
    f32x4 s0 = f32x4{0.f, 0.f, 0.f, 0.f}, s1 = s0;
#pragma unroll
    for (int kc = 0; kc < CF; ++kc) {
      const Frag<T> bq = load_frag<T>(Qs + qrow * LDQ + (kc * 32 + g * 8) * ES);
      mfma_frag(s0, load_frag<T>(Ks + (lane & 15) * LDQ + (kc * 32 + g * 8) * ES), bq);
      mfma_frag(s1, load_frag<T>(Ks + (16 + (lane & 15)) * LDQ + (kc * 32 + g * 8) * ES), bq);
    }
    float tmax = -INFINITY;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (kbase + 4 * g + i >= P) s0[i] = -INFINITY;
      if (kbase + 16 + 4 * g + i >= P) s1[i] = -INFINITY;
      tmax = fmaxf(tmax, fmaxf(s0[i], s1[i]));
    }
    tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
    const float m_new = fmaxf(m_run, tmax);              // finite: key kbase is inside the image
    const float alpha = exp2f((m_run - m_new) * sl);     // 0 at the first tile (m_run = -inf)
    float psum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s0[i] = exp2f((s0[i] - m_new) * sl);
      s1[i] = exp2f((s1[i] - m_new) * sl);
    }
    psum = ((s0[0] + s0[1]) + (s0[2] + s0[3])) + ((s1[0] + s1[1]) + (s1[2] + s1[3]));
    psum += __shfl_xor(psum, 16);
    psum += __shfl_xor(psum, 32);
    l_run = l_run * alpha + psum;
    m_run = m_new;
    const Frag<T> pf = prob_frag<T>(s0, s1);
#pragma unroll
    for (int f = 0; f < NF; ++f) {                       // O^T[channel 16 f + 4 g + i][query] += V^T P^T
      O[f] *= alpha;
      mfma_frag(O[f], load_frag<T>(Vt + (f * 16 + (lane & 15)) * LDV + g * 8 * ES), pf);
    }
  }
  // O / sum into this wave's own rows of the Q tile (T), then the out conv reads it as a B operand
  const float inv = 1.0f / l_run;
#pragma unroll
  for (int f = 0; f < NF; ++f)
    store4<T>((T*)(Qs + qrow * LDQ) + f * 16 + 4 * g, O[f][0] * inv, O[f][1] * inv, O[f][2] * inv, O[f][3] * inv);
  __syncthreads();                     // O visible; every wave is done with K / V^T (the statistics tile)
  const bool valid = qrow < QT;
  const size_t prow = (size_t)b * P + q0 + (valid ? qrow : 0);
  const T* xin = (const T*)a.x + prow * C;
  T* out = (T*)a.out + prow * C;
  const T* wf = (const T*)a.wout_f + (size_t)lane * 8;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kc = 0; kc < CF; ++kc)
      mfma_frag(acc, load_frag<T>((const char*)(wf + ((size_t)f * CF + kc) * 512)),
                load_frag<T>(Qs + qrow * LDQ + (kc * 32 + g * 8) * ES));
    const int co = f * 16 + 4 * g;
    const f32x4 r = load4<T>(xin + co);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] += a.bout[co + i] + r[i];
    *(f32x4*)(tl + qrow * LDT + co) = acc;
    if (valid) store4<T>(out + co, acc[0], acc[1], acc[2], acc[3]);
  }
  __syncthreads();
  if (a.stats)
    tile_channel_stats(tl, LDT, QT, C, a.stats + ((size_t)b * (P / QT) + tile) * C * 2, 2);
}

size_t attn_qkv_lds_bytes(int dtype, int C) {
  const size_t es = dtype == DT_F32 ? 4 : 2;
  return (size_t)C * 8 + (size_t)64 * (C * es + 16);
}

template <typename T>
static size_t core_lds(int cf) {
  switch (cf) {
    case 1: return AttnLds<T, 1>::total; case 2: return AttnLds<T, 2>::total; case 3: return AttnLds<T, 3>::total;
    case 4: return AttnLds<T, 4>::total; case 5: return AttnLds<T, 5>::total; case 6: return AttnLds<T, 6>::total;
    case 7: return AttnLds<T, 7>::total; case 8: return AttnLds<T, 8>::total;
  }
  return (size_t)1 << 40;
}
size_t attn_core_lds_bytes(int dtype, int C) {
  if (C < 32 || C % 32 || C > kAttnMaxC) return (size_t)1 << 40;
  return dtype == DT_F32 ? core_lds<float>(C / 32) : core_lds<bf16_t>(C / 32);
}

static bool attn_args_ok(const AttnArgs& a, int B) {
  return B >= 1 && B <= 65535 && a.P >= 1 && a.C >= 32 && a.C % 32 == 0 && a.C <= kAttnMaxC && a.QT >= 1 &&
         a.QT <= kAttnQueryTile && a.P % a.QT == 0 && a.groups >= 1 && a.groups <= 256 && a.C % a.groups == 0 &&
         a.x && a.qkv && a.gst && a.gamma && a.beta;
}

hipError_t launch_attn_qkv(int dtype, const AttnArgs& a, int B, hipStream_t s) {
  if (!attn_args_ok(a, B) || !a.wqkv_f) return hipErrorInvalidValue;
  const size_t lds = attn_qkv_lds_bytes(dtype, a.C);
  const dim3 grid((a.P + 63) / 64, a.C / 32, B), blk(256);
  if (dtype == DT_F32) hipLaunchKernelGGL(attn_qkv_kernel<float>, grid, blk, lds, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(attn_qkv_kernel<bf16_t>, grid, blk, lds, s, a);
  else hipLaunchKernelGGL(attn_qkv_kernel<f16_t>, grid, blk, lds, s, a);
  return hipGetLastError();
}

template <typename T>
static hipError_t core_go(const AttnArgs& a, int B, hipStream_t s) {
  const dim3 grid(a.P / a.QT, B), blk(256);
  switch (a.C / 32) {
#define SDDM_ATTN(CFV) \
    case CFV: { const size_t lds = AttnLds<T, CFV>::total; hipLaunchKernelGGL((attn_core_kernel<T, CFV>), grid, blk, lds, s, a); } break;
    SDDM_ATTN(1) SDDM_ATTN(2) SDDM_ATTN(3) SDDM_ATTN(4) SDDM_ATTN(5) SDDM_ATTN(6) SDDM_ATTN(7) SDDM_ATTN(8)
#undef SDDM_ATTN
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_attn_core(int dtype, const AttnArgs& a, int B, hipStream_t s) {
  if (!attn_args_ok(a, B) || !a.wout_f || !a.bout || !a.out) return hipErrorInvalidValue;
  if (dtype == DT_F32) return core_go<float>(a, B, s);
  if (dtype == DT_BF16) return core_go<bf16_t>(a, B, s);
  return core_go<f16_t>(a, B, s);
}

// ---------------------------------------------------------------------------------------------
// per-tile statistics of [B][P][C]: one block per (tile, image), one thread per channel, two passes
// in pixel order
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_input_stats_kernel(const T* x, float* stats, int P, int C, int n_tile) {
  const int tile = blockIdx.x, b = blockIdx.y, tiles = P / n_tile;
  const T* src = x + ((size_t)b * P + (size_t)tile * n_tile) * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    float s = 0.f;
    for (int p = 0; p < n_tile; ++p) s += to_f32<T>(src[(size_t)p * C + c]);
    const float mean = s / (float)n_tile;
    float m2 = 0.f;
    for (int p = 0; p < n_tile; ++p) {
      const float d = to_f32<T>(src[(size_t)p * C + c]) - mean;
      m2 += d * d;
    }
    float* dst = stats + (((size_t)b * tiles + tile) * C + c) * 2;
    dst[0] = s;
    dst[1] = m2;
  }
}

hipError_t launch_attn_input_stats(int dtype, const void* x, float* stats, int B, int P, int C, int n_tile, hipStream_t s) {
  if (B < 1 || B > 65535 || P < 1 || C < 1 || n_tile < 1 || P % n_tile || !x || !stats) return hipErrorInvalidValue;
  const dim3 grid(P / n_tile, B), blk(256);
  if (dtype == DT_F32) hipLaunchKernelGGL(attn_input_stats_kernel<float>, grid, blk, 0, s, (const float*)x, stats, P, C, n_tile);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(attn_input_stats_kernel<bf16_t>, grid, blk, 0, s, (const bf16_t*)x, stats, P, C, n_tile);
  else hipLaunchKernelGGL(attn_input_stats_kernel<f16_t>, grid, blk, 0, s, (const f16_t*)x, stats, P, C, n_tile);
  return hipGetLastError();
}

}  // namespace sddm
