// Waveunet3 denoiser (reference model/waveunet3.py:314-416 at the arguments of config_waveunet3.json)
// for SDDM.infer (model.py:50-124).  wu_runtime.h holds the layer sequence.
//
// Activations are channels-last [B][L][C] in the compute dtype, so a position's channels are
// contiguous and an MFMA operand fragment (8 channels) is one (bf16 / f16) or two (fp32) 16-byte
// loads.  Every 5-tap Block conv, the 4-tap stride-2 DownsampleLayer conv and the 4-tap stride-2
// transposed UpsampleLayer conv is one launch of wu_conv_kernel: an implicit GEMM over (tap, ci)
// whose input slab is staged through LDS in 32-channel chunks with GroupNorm + SiLU applied once
// per element on the way in, and whose epilogue adds bias, the per-row noise-level constant, the
// residual and the shortcut, stores, and leaves per-wave (sum, sum of squares) partials of what it
// stored.  The partials are plain stores into per-slot cells, reduced in a fixed order by
// wu_gn_finalize in fp64: the statistics of a row do not depend on the batch it sits in.
#include "conv_common.h"
#include "wu_kernels.h"

#include <algorithm>

namespace sddm {

__device__ __forceinline__ float wu_level(const WULevel& lv, int b) {
  if (lv.levels) return lv.levels[b];
  const int t = *lv.t_dev;
  return lv.time_step ? (float)t : lv.table[t];
}

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
// One thread per position computes its 32 channels from the 5-tap windows of both fp32 sources
// (activated in registers; the zero padding applies to the activated signal).  The stored values
// go through LDS once more for the statistics: thread (c, seg) sums channel c over the 32 positions
// of segment seg in ascending order -- 8 slots per block
template <typename T>
__global__ __launch_bounds__(256) void wu_stem_kernel(WUStemArgs a) {
  __shared__ float w[32 * 10], cb[32], vals[kWuStemTile][33];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * kWuStemTile;
  for (int i = tid; i < 320; i += 256) w[i] = a.w[i];
  if (tid < 32) cb[tid] = a.bias[tid] + (a.nw[tid] * wu_level(a.lv, b) + a.nb[tid]);
  __syncthreads();
  const float s0 = a.scale[b * 2], h0 = a.shift[b * 2], s1 = a.scale[b * 2 + 1], h1 = a.shift[b * 2 + 1];
  const float* c = a.cond + (size_t)b * a.L;
  const float* x = a.x + (size_t)b * a.L;
  const int t = t0 + tid;
  float cv[5], xv[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int m = t + k - 2;
    const bool in = t < a.L && m >= 0 && m < a.L;
    cv[k] = in ? silu(c[m] * s0 + h0) : 0.f;
    xv[k] = in ? silu(x[m] * s1 + h1) : 0.f;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int co = q * 4 + e;
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 5; ++k) s += w[co * 10 + k] * cv[k];
#pragma unroll
      for (int k = 0; k < 5; ++k) s += w[co * 10 + 5 + k] * xv[k];
      v[e] = round_t<T>(s + cb[co]);
      vals[tid][co] = t < a.L ? v[e] : 0.f;
    }
    if (t < a.L) store4<T>((T*)a.out + ((size_t)b * a.L + t) * 32 + q * 4, v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  const int ch = tid & 31, seg = tid >> 5;
  float s = 0.f, ss = 0.f;
  for (int r = 0; r < 32; ++r) {
    const float v = vals[seg * 32 + r][ch];
    s += v;
    ss += v * v;
  }
  const int nslots = 8 * gridDim.x;
  float* st = a.stats + (((size_t)b * nslots + blockIdx.x * 8 + seg) * 32 + ch) * 2;
  st[0] = s;
  st[1] = ss;
}

hipError_t launch_wu_stem(int dtype, const WUStemArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1 || !a.stats) return hipErrorInvalidValue;
  const dim3 grid((a.L + kWuStemTile - 1) / kWuStemTile, a.B);
  if (dtype == DT_F32) hipLaunchKernelGGL(wu_stem_kernel<float>, grid, dim3(256), 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(wu_stem_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wu_stem_kernel<f16_t>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------- the MFMA convolution ----------------
// Block = 4 waves = 128 output positions x all Cout (<= 128) channels; wave w owns 32 positions as
// two 16-column B fragments and Cout / 16 A fragments, i.e. up to 8 x 2 accumulator tiles.  Per
// 32-channel chunk of the input the block stages the slab of input rows its outputs touch
// (GroupNorm + SiLU applied here, rows outside [0, Lin) zero), then every tap reads its B fragments
// from the slab at a row offset.  The global loads of chunk c + 1 are issued (into registers)
// before the MFMAs of chunk c and stored to LDS after them.  Weights (L2-resident: the whole
// network has 1.3 M parameters): bf16 / f16 stage the chunk's [taps][Cout][32] image through LDS
// with the slab; fp32 loads the NCO = Cout / 16 A fragments of a tap together from global memory,
// one tap ahead of the MFMAs that use them.
//   WU_CONV5: output o, tap k reads input o + k - 2; slab rows [t0 - 2, t0 + 130).
//   WU_DOWN4: output o, tap k reads input 2 o + k - 1; slab rows [2 t0 - 1, 2 t0 + 257).
//   WU_UP4:   ConvTranspose1d: out[2 i - 1 + k] += W[k] x[i].  Output 2 m + ph takes the taps of
//             its parity only: ph = 0: (k = 1, x[m]), (k = 3, x[m - 1]); ph = 1: (k = 0, x[m + 1]),
//             (k = 2, x[m]).  A block owns 64 input positions m; wave w runs phase w & 1 on the
//             32 positions m0 + 32 (w >> 1) ..., so a fragment's 16 columns share their taps.
//             Slab rows [m0 - 1, m0 + 65).
template <int MODE> struct WuGeom;
template <> struct WuGeom<WU_CONV5> { static constexpr int ROWS = kWuTile + 4, TAPS = 5, KW = 5; };
template <> struct WuGeom<WU_DOWN4> { static constexpr int ROWS = 2 * kWuTile + 2, TAPS = 4, KW = 4; };
template <> struct WuGeom<WU_UP4> { static constexpr int ROWS = kWuTile / 2 + 2, TAPS = 2, KW = 4; };

template <typename T, int MODE, int NCO>
__global__ __launch_bounds__(256) void wu_conv_kernel(WUConvArgs a) {
  constexpr int ES = (int)sizeof(T), UE = 16 / ES;          // elements per 16-byte unit
  constexpr int UPR = 32 / UE;                               // units per 32-channel row
  constexpr int RS = 32 * ES + 16;                           // padded LDS row stride (bytes)
  constexpr int ROWS = WuGeom<MODE>::ROWS, TAPS = WuGeom<MODE>::TAPS, KW = WuGeom<MODE>::KW;
  // 16-bit storage: the chunk's weights [taps][Cout][32] are staged through LDS with the slab (51 KB
  // at most with it); fp32 images would not fit the 64 KB of static LDS and come from global memory
  constexpr bool WL = ES == 2;
  constexpr int WROWS = NCO * 16 * KW;
  __shared__ __attribute__((aligned(16))) char slab[ROWS * RS];
  __shared__ __attribute__((aligned(16))) char wl[WL ? WROWS * RS : 16];
  __shared__ float sc_s[128], sh_s[128];

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, tile = blockIdx.x;
  const int Cin = a.Cin, Cout = NCO * 16;
  const int ph = MODE == WU_UP4 ? (wave & 1) : 0;
  // first output position of the block (WU_UP4: first input position m0) and first slab row
  const int t0 = MODE == WU_UP4 ? tile * (kWuTile / 2) : tile * kWuTile;
  const int in_lo = MODE == WU_CONV5 ? t0 - 2 : (MODE == WU_DOWN4 ? 2 * t0 - 1 : t0 - 1);
  // column base of the wave's fragments inside the block
  const int wcol = MODE == WU_UP4 ? (wave >> 1) * 32 : wave * 32;

  const bool gn = a.scale != nullptr;
  if (gn)
    for (int c = tid; c < Cin; c += 256) {
      sc_s[c] = a.scale[(size_t)b * Cin + c];
      sh_s[c] = a.shift[(size_t)b * Cin + c];
    }

  f32x4 acc[NCO][2];
#pragma unroll
  for (int c = 0; c < NCO; ++c)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nck = Cin / 32, nrk = a.res_mode == 2 ? a.RC / 32 : 0;
  // the A fragments of tap k of chunk ch from global memory (chunks >= nck: the res_conv's single tap)
  auto load_a = [&](int ch, int k, Frag<T>* af) {
    const bool main = ch < nck;
    const int c0 = (main ? ch : ch - nck) * 32;
    const int wk = MODE == WU_UP4 ? (1 - ph) + 2 * k : k;
    const T* wp = main ? (const T*)a.w + (size_t)wk * Cin + c0 + g * 8 : (const T*)a.rw + c0 + g * 8;
    const int wstride = main ? KW * Cin : a.RC;
#pragma unroll
    for (int c = 0; c < NCO; ++c) af[c] = load_frag<T>((const char*)(wp + (size_t)(c * 16 + l16) * wstride));
  };
  // staging registers of one chunk: the slab units and (WL) the weight units of this thread
  constexpr int SIT = (ROWS * UPR + 255) / 256, WIT = WL ? (WROWS * UPR + 255) / 256 : 1;
  f32x4 sv[SIT], wv[WIT];
  auto gload = [&](int ch) {
    const bool main = ch < nck;
    const int c0 = (main ? ch : ch - nck) * 32;
    const T* sp = main ? (const T*)a.src + (size_t)b * a.Lin * Cin : (const T*)a.res + (size_t)b * a.Lout * a.RC;
    const int Ls = main ? a.Lin : a.Lout, Cs = main ? Cin : a.RC;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r;
      sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < ROWS * UPR && pos >= 0 && pos < Ls) sv[j] = *(const f32x4*)(sp + (size_t)pos * Cs + c0 + q * UE);
    }
    if (WL) {                              // weight rows (co, tap) of the chunk, in their global order
      const int kwn = main ? KW : 1, wrows = Cout * kwn;
      const T* wp = main ? (const T*)a.w : (const T*)a.rw;
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        if (u < wrows * UPR) wv[j] = *(const f32x4*)(wp + (size_t)r * Cs + c0 + q * UE);
      }
    }
  };
  auto lstore = [&](int ch) {
    const bool main = ch < nck;
    const int c0 = (main ? ch : ch - nck) * 32;
    const int Ls = main ? a.Lin : a.Lout;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r;
      if (u < ROWS * UPR) {
        f32x4 v = sv[j];
        if (main && gn && pos >= 0 && pos < Ls) v = transform_vec<T>(v, sc_s + c0 + q * UE, sh_s + c0 + q * UE, true);
        *(f32x4*)(slab + r * RS + q * 16) = v;
      }
    }
    if (WL) {                              // LDS row = tap * Cout + co: a tap's channels are consecutive rows
      const int kwn = main ? KW : 1, wrows = Cout * kwn;
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        const int co = r / kwn, wk = r - co * kwn;
        if (u < wrows * UPR) *(f32x4*)(wl + (wk * Cout + co) * RS + q * 16) = wv[j];
      }
    }
  };
  Frag<T> af[NCO];
  if (!WL) load_a(0, 0, af);
  gload(0);
  for (int ch = 0; ch < nck + nrk; ++ch) {
    const bool main = ch < nck;
    __syncthreads();                       // the previous chunk's fragments are read; sc_s / sh_s are visible
    lstore(ch);
    __syncthreads();
    if (ch + 1 < nck + nrk) gload(ch + 1); // the next chunk's loads fly during this chunk's MFMAs
    const int ntap = main ? TAPS : 1;
    for (int k = 0; k < ntap; ++k) {
      Frag<T> an[NCO];
      const bool more = !WL && (k + 1 < ntap || ch + 1 < nck + nrk);
      if (more) load_a(k + 1 < ntap ? ch : ch + 1, k + 1 < ntap ? k + 1 : 0, an);
      if (WL) {
        const int wk = !main ? 0 : (MODE == WU_UP4 ? (1 - ph) + 2 * k : k);
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = load_frag<T>(wl + (wk * Cout + c * 16 + l16) * RS + g * 8 * ES);
      }
      // slab row of column 0 of the wave's first fragment
      int r0, rstep = 1;
      if (!main) r0 = wcol + 2;                                              // res_conv: the centre row
      else if (MODE == WU_CONV5) r0 = wcol + k;
      else if (MODE == WU_DOWN4) { r0 = 2 * wcol + k; rstep = 2; }
      else r0 = wcol + ph - k + 1;
      Frag<T> bf[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) bf[p] = load_frag<T>(slab + (r0 + (p * 16 + l16) * rstep) * RS + g * 8 * ES);
#pragma unroll
      for (int c = 0; c < NCO; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) mfma_frag(acc[c][p], af[c], bf[p]);
      if (more) {
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = an[c];
      }
    }
  }

  // epilogue
  const float lvl = a.nw ? wu_level(a.lv, b) : 0.f;
  const int nslots = 4 * gridDim.x;
  int opos[2];
  bool ok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = wcol + p * 16 + l16;
    opos[p] = MODE == WU_UP4 ? 2 * (t0 + col) + ph : t0 + col;
    ok[p] = opos[p] < a.Lout;
  }
  float rc[2] = {0.f, 0.f}, rx[2] = {0.f, 0.f};
  if (a.res_mode == 3) {
#pragma unroll
    for (int p = 0; p < 2; ++p)
      if (ok[p]) {
        rc[p] = a.cond[(size_t)b * a.Lout + opos[p]];
        rx[p] = a.x[(size_t)b * a.Lout + opos[p]];
      }
  }
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    {
      const int cb = c * 16 + 4 * g;
      float bias[4], s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 4; ++i) bias[i] = a.bias[cb + i] + (a.nw ? a.nw[cb + i] * lvl + a.nb[cb + i] : 0.f);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (ok[p]) {
          const size_t o = ((size_t)b * a.Lout + opos[p]) * Cout + cb;
          float v[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] = acc[c][p][i] + bias[i];
          if (a.res_mode == 1) {
            const f32x4 r = load4<T>((const T*)a.res + o);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] += r[i];
          } else if (a.res_mode == 3) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] += a.rw2[(cb + i) * 2] * rc[p] + a.rw2[(cb + i) * 2 + 1] * rx[p];
          }
          if (a.shortcut) {
            const f32x4 r = load4<T>((const T*)a.shortcut + o);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] += r[i];
          }
          store4<T>((T*)a.out + o, v[0], v[1], v[2], v[3]);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float r = round_t<T>(v[i]);
            s[i] += r;
            ss[i] += r * r;
          }
        }
      }
      if (a.stats) {                       // (block-uniform) every lane takes part in the row sums
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float ts = row_sum16(s[i]), tss = row_sum16(ss[i]);
          if (l16 == 0) {
            float* st = a.stats + (((size_t)b * nslots + tile * 4 + wave) * Cout + cb + i) * 2;
            st[0] = ts;
            st[1] = tss;
          }
        }
      }
    }
  }
}

template <typename T, int MODE>
static hipError_t wu_conv_dispatch_nco(const WUConvArgs& a, dim3 grid, hipStream_t s) {
  switch (a.Cout) {
    case 32:
      if (MODE != WU_CONV5) return hipErrorInvalidValue;   // the resampling layers are 64 / 96 / 128 wide
      hipLaunchKernelGGL((wu_conv_kernel<T, WU_CONV5, 2>), grid, dim3(256), 0, s, a);
      break;
    case 64: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 4>), grid, dim3(256), 0, s, a); break;
    case 96: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 6>), grid, dim3(256), 0, s, a); break;
    case 128: hipLaunchKernelGGL((wu_conv_kernel<T, MODE, 8>), grid, dim3(256), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T>
static hipError_t wu_conv_dispatch(const WUConvArgs& a, dim3 grid, hipStream_t s) {
  if (a.mode == WU_CONV5) return wu_conv_dispatch_nco<T, WU_CONV5>(a, grid, s);
  if (a.mode == WU_DOWN4) return wu_conv_dispatch_nco<T, WU_DOWN4>(a, grid, s);
  return wu_conv_dispatch_nco<T, WU_UP4>(a, grid, s);
}

hipError_t launch_wu_conv(int dtype, const WUConvArgs& a, hipStream_t s) {
  if (a.mode < WU_CONV5 || a.mode > WU_UP4 || a.B < 1 || a.Lin < 1 || a.Lout < 1) return hipErrorInvalidValue;
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
  const dim3 grid((a.Lout + kWuTile - 1) / kWuTile, a.B);
  if (dtype == DT_F32) return wu_conv_dispatch<float>(a, grid, s);
  if (dtype == DT_BF16) return wu_conv_dispatch<bf16_t>(a, grid, s);
  return wu_conv_dispatch<f16_t>(a, grid, s);
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
