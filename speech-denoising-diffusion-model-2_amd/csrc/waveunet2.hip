// Waveunet2 denoiser (reference model/waveunet2.py:226-324 at the arguments of config_waveunet2.json)
// for SDDM.infer (model.py:50-124).  wu2_runtime.h holds the layer sequence.
//
// Activations are channels-last [B][L][C] in the compute dtype at the true C (24 / 48 / 72 / 96), so
// an MFMA operand fragment (8 channels) is one (bf16 / f16) or two (fp32) 16-byte loads.  Every
// ConvLayer stores its raw conv output and (sum, sum of squares) partials of it; its GroupNorm +
// ReLU -- and on the way up the per-position FiLM -- is applied by the consumer while it stages its
// input slab, once per element.  The channel counts are no multiples of the MFMA K of 32 or of the
// 16 rows of a fragment: the last 32-channel chunk of the input and the last 16-row fragment of the
// output are zero-filled where they are staged (LDS, or the fragment registers in fp32), never in
// memory, and stores and statistics are masked to the true Cout.
#include "conv_common.h"
#include "wu2_kernels.h"

#include <algorithm>

namespace sddm {

__device__ __forceinline__ float wu2_level(const WULevel& lv, int b) {
  if (lv.levels) return lv.levels[b];
  const int t = *lv.t_dev;
  return lv.time_step ? (float)t : lv.table[t];
}

// ---------------- stem: Conv1d(2, 24, 5, padding 2) on the two raw fp32 sources ----------------
// One thread per position computes its 24 channels from the 5-tap windows of both sources.  The
// stored values go through LDS once more for the statistics: thread (c, seg) sums channel c over the
// 32 positions of segment seg in ascending order -- 8 slots per block
template <typename T>
__global__ __launch_bounds__(256) void wu2_stem_kernel(WU2StemArgs a) {
  constexpr int C = kWu2StemC;
  __shared__ float w[C * 10], cb[C], vals[kWu2StemTile][C + 1];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * kWu2StemTile;
  if (a.t_dev && blockIdx.x == 0 && b == 0 && tid == 0) *a.t_dev -= 1;   // this step's t
  for (int i = tid; i < C * 10; i += 256) w[i] = a.w[i];
  if (tid < C) cb[tid] = a.bias[tid];
  __syncthreads();
  const float* c = a.cond + (size_t)b * a.L;
  const float* x = a.x + (size_t)b * a.L;
  const int t = t0 + tid;
  float cv[5], xv[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int m = t + k - 2;
    const bool in = t < a.L && m >= 0 && m < a.L;
    cv[k] = in ? c[m] : 0.f;
    xv[k] = in ? x[m] : 0.f;
  }
#pragma unroll
  for (int q = 0; q < C / 4; ++q) {
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
    if (t < a.L) store4<T>((T*)a.out + ((size_t)b * a.L + t) * C + q * 4, v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  if (tid < C * 8) {
    const int ch = tid % C, seg = tid / C;
    float s = 0.f, ss = 0.f;
    for (int r = 0; r < 32; ++r) {
      const float v = vals[seg * 32 + r][ch];
      s += v;
      ss += v * v;
    }
    const int nslots = 8 * gridDim.x;
    float* st = a.stats + (((size_t)b * nslots + blockIdx.x * 8 + seg) * C + ch) * 2;
    st[0] = s;
    st[1] = ss;
  }
}

hipError_t launch_wu2_stem(int dtype, const WU2StemArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1 || !a.stats) return hipErrorInvalidValue;
  const dim3 grid((a.L + kWu2StemTile - 1) / kWu2StemTile, a.B);
  if (dtype == DT_F32) hipLaunchKernelGGL(wu2_stem_kernel<float>, grid, dim3(256), 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL(wu2_stem_kernel<bf16_t>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(wu2_stem_kernel<f16_t>, grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------- the MFMA convolution ----------------
// Block = 4 waves = 128 output positions x all Cout channels; wave w owns 32 positions as two
// 16-column B fragments and NCO = ceil(Cout / 16) A fragments.  Per 32-channel chunk of the input
// the block stages the slab of input rows its outputs touch (GroupNorm + ReLU + FiLM applied here;
// rows outside [0, Lin) and channels >= Cin zero), then every tap reads its B fragments from the
// slab at a row offset.  The global loads of chunk c + 1 are issued (into registers) before the
// MFMAs of chunk c and stored to LDS after them.  Weights (L2-resident: the whole network has
// 0.45 M parameters): bf16 / f16 stage the chunk's [taps][16 NCO][32] image through LDS with the
// slab, rows >= Cout and channels >= Cin zero; fp32 loads the NCO A fragments of a tap together from
// global memory, one tap ahead of the MFMAs that use them, with the same lanes zero.
//   WU2_CONV5: output o, tap k reads input o + k - 2; slab rows [t0 - 2, t0 + 130).
//   WU2_CONV3: output o, tap k reads input o + k - 1; slab rows [t0 - 1, t0 + 129).
//   WU2_DOWN4: output o, tap k reads input 2 o + k - 1; slab rows [2 t0 - 1, 2 t0 + 257).
//   WU2_UP4:   ConvTranspose1d: out[2 i - 1 + k] += W[k] x[i].  Output 2 m + ph takes the taps of
//              its parity only: ph = 0: (k = 1, x[m]), (k = 3, x[m - 1]); ph = 1: (k = 0, x[m + 1]),
//              (k = 2, x[m]).  A block owns 64 input positions m; wave w runs phase w & 1 on the
//              32 positions m0 + 32 (w >> 1) ..., so a fragment's 16 columns share their taps.
//              Slab rows [m0 - 1, m0 + 65).
template <int MODE> struct Wu2Geom;
template <> struct Wu2Geom<WU2_CONV5> { static constexpr int ROWS = kWu2Tile + 4, TAPS = 5, KW = 5, LO = 2; };
template <> struct Wu2Geom<WU2_CONV3> { static constexpr int ROWS = kWu2Tile + 2, TAPS = 3, KW = 3, LO = 1; };
template <> struct Wu2Geom<WU2_DOWN4> { static constexpr int ROWS = 2 * kWu2Tile + 2, TAPS = 4, KW = 4, LO = 1; };
template <> struct Wu2Geom<WU2_UP4> { static constexpr int ROWS = kWu2Tile / 2 + 2, TAPS = 2, KW = 4, LO = 1; };

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

template <typename T, int MODE, int NCO>
__global__ __launch_bounds__(256) void wu2_conv_kernel(WU2ConvArgs a) {
  constexpr int ES = (int)sizeof(T), UE = 16 / ES;          // elements per 16-byte unit
  constexpr int UPR = 32 / UE;                               // units per 32-channel row
  constexpr int RS = 32 * ES + 16;                           // padded LDS row stride (bytes)
  constexpr int ROWS = Wu2Geom<MODE>::ROWS, TAPS = Wu2Geom<MODE>::TAPS, KW = Wu2Geom<MODE>::KW;
  constexpr bool WL = ES == 2;                               // 16-bit: the chunk's weights go through LDS (52 KB at most with the slab)
  constexpr int CP = NCO * 16;                               // Cout padded to whole fragments
  constexpr int WROWS = CP * KW;
  __shared__ __attribute__((aligned(16))) char slab[ROWS * RS];
  __shared__ __attribute__((aligned(16))) char wl[WL ? WROWS * RS : 16];
  __shared__ float sc_s[96], sh_s[96], enc_s[96];

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, tile = blockIdx.x;
  const int Cin = a.Cin, Cout = a.Cout;
  const int ph = MODE == WU2_UP4 ? (wave & 1) : 0;
  // first output position of the block (WU2_UP4: first input position m0) and first slab row
  const int t0 = MODE == WU2_UP4 ? tile * (kWu2Tile / 2) : tile * kWu2Tile;
  const int in_lo = MODE == WU2_DOWN4 ? 2 * t0 - 1 : t0 - Wu2Geom<MODE>::LO;
  // column base of the wave's fragments inside the block
  const int wcol = MODE == WU2_UP4 ? (wave >> 1) * 32 : wave * 32;

  const bool gn = a.scale != nullptr, film = a.film != nullptr;
  if (gn)
    for (int c = tid; c < Cin; c += 256) {
      sc_s[c] = a.scale[(size_t)b * Cin + c];
      sh_s[c] = a.shift[(size_t)b * Cin + c];
    }
  if (a.enc_dim > 0 && tid < a.enc_dim) {  // PositionalEncoding (waveunet2.py:34-39), fp32 as torch, accurate sinf / cosf
    const int half = a.enc_dim / 2, k = tid < half ? tid : tid - half;
    const float arg = wu2_level(a.lv, b) * expf(-9.210340371976184f * ((float)k / (float)half));
    enc_s[tid] = tid < half ? sinf(arg) : cosf(arg);
  }

  f32x4 acc[NCO][2];
#pragma unroll
  for (int c = 0; c < NCO; ++c)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nck = (Cin + 31) / 32;
  const T* sp = (const T*)a.src + (size_t)b * a.Lin * Cin;
  // fp32: the A fragments of tap k of chunk ch from global memory; rows >= Cout and channels >= Cin zero
  auto load_a = [&](int ch, int k, Frag<T>* af) {
    const int cg = ch * 32 + g * 8;
    const int wk = MODE == WU2_UP4 ? (1 - ph) + 2 * k : k;
    const T* wp = (const T*)a.w + (size_t)wk * Cin + cg;
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      const int co = c * 16 + l16;
      if (co < Cout && cg < Cin) af[c] = load_frag<T>((const char*)(wp + (size_t)co * KW * Cin));
      else af[c] = Frag<T>{};
    }
  };
  // staging registers of one chunk: the slab units and (WL) the weight units of this thread
  constexpr int SIT = (ROWS * UPR + 255) / 256, WIT = WL ? (WROWS * UPR + 255) / 256 : 1;
  f32x4 sv[SIT], wv[WIT];
  auto gload = [&](int ch) {
    const int c0 = ch * 32;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r;
      sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < ROWS * UPR && pos >= 0 && pos < a.Lin && c0 + q * UE < Cin) sv[j] = *(const f32x4*)(sp + (size_t)pos * Cin + c0 + q * UE);
    }
    if (WL) {                              // weight rows (co, tap) of the chunk, in their global order
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < Cout * KW && c0 + q * UE < Cin) wv[j] = *(const f32x4*)((const T*)a.w + (size_t)r * Cin + c0 + q * UE);
      }
    }
  };
  auto lstore = [&](int ch) {
    const int c0 = ch * 32;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r, cq = c0 + q * UE;
      if (u < ROWS * UPR) {
        f32x4 v = sv[j];
        if (gn && pos >= 0 && pos < a.Lin && cq < Cin) {
          f32x4 fs = f32x4{0.f, 0.f, 0.f, 0.f}, fh = fs;
          if (film) {
            const T* fp = (const T*)a.film + ((size_t)b * a.Lin + pos) * (2 * Cin) + cq;
            fh = *(const f32x4*)fp;
            fs = *(const f32x4*)(fp + Cin);
          }
          v = wu2_transform<T>(v, sc_s + cq, sh_s + cq, film, fs, fh);
        }
        *(f32x4*)(slab + r * RS + q * 16) = v;
      }
    }
    if (WL) {                              // LDS row = tap * CP + co: a tap's channels are consecutive rows
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        const int co = r / KW, wk = r - co * KW;
        if (u < WROWS * UPR) *(f32x4*)(wl + (wk * CP + co) * RS + q * 16) = wv[j];
      }
    }
  };
  Frag<T> af[NCO];
  if (!WL) load_a(0, 0, af);
  gload(0);
  for (int ch = 0; ch < nck; ++ch) {
    __syncthreads();                       // the previous chunk's fragments are read; sc_s / sh_s are visible
    lstore(ch);
    __syncthreads();
    if (ch + 1 < nck) gload(ch + 1);       // the next chunk's loads fly during this chunk's MFMAs
    for (int k = 0; k < TAPS; ++k) {
      Frag<T> an[NCO];
      const bool more = !WL && (k + 1 < TAPS || ch + 1 < nck);
      if (more) load_a(k + 1 < TAPS ? ch : ch + 1, k + 1 < TAPS ? k + 1 : 0, an);
      if (WL) {
        const int wk = MODE == WU2_UP4 ? (1 - ph) + 2 * k : k;
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = load_frag<T>(wl + (wk * CP + c * 16 + l16) * RS + g * 8 * ES);
      }
      // slab row of column 0 of the wave's first fragment
      int r0, rstep = 1;
      if (MODE == WU2_CONV5 || MODE == WU2_CONV3) r0 = wcol + k;
      else if (MODE == WU2_DOWN4) { r0 = 2 * wcol + k; rstep = 2; }
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
  const int nslots = 4 * gridDim.x;
  const bool enc = a.enc_dim > 0;
  int opos[2];
  bool ok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = wcol + p * 16 + l16;
    opos[p] = MODE == WU2_UP4 ? 2 * (t0 + col) + ph : t0 + col;
    ok[p] = opos[p] < a.Lout;
  }
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    const int cb = c * 16 + 4 * g;
    const bool okc = cb < Cout;            // Cout % 8 == 0: the 4 channels of an accumulator are in or out together
    float bias[4], e4[4], s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      bias[i] = okc ? a.bias[cb + i] : 0.f;
      e4[i] = enc && okc ? enc_s[cb + i] : 0.f;
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (ok[p] && okc) {
        const size_t o = ((size_t)b * a.Lout + opos[p]) * Cout + cb;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[c][p][i] + bias[i];
          if (enc) v[i] = (v[i] > 0.f ? v[i] : 0.2f * v[i]) + e4[i];
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
    if (a.stats) {                         // (block-uniform) every lane takes part in the row sums
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ts = row_sum16(s[i]), tss = row_sum16(ss[i]);
        if (l16 == 0 && okc) {
          float* st = a.stats + (((size_t)b * nslots + tile * 4 + wave) * Cout + cb + i) * 2;
          st[0] = ts;
          st[1] = tss;
        }
      }
    }
  }
}

template <typename T, int MODE>
static hipError_t wu2_conv_dispatch_nco(const WU2ConvArgs& a, dim3 grid, hipStream_t s) {
  // fragments per launch: ConvLayers 24 / 48 / 72 / 96 -> 2 / 3 / 5 / 6 (the resampling layers are 48 / 72 / 96
  // wide), the FiLM output_conv 48 / 96 / 144 -> 3 / 6 / 9
  switch ((a.Cout + 15) / 16) {
    case 2:
      if constexpr (MODE == WU2_CONV5 || MODE == WU2_CONV3) {
        hipLaunchKernelGGL((wu2_conv_kernel<T, MODE, 2>), grid, dim3(256), 0, s, a);
        break;
      } else {
        return hipErrorInvalidValue;
      }
    case 3: hipLaunchKernelGGL((wu2_conv_kernel<T, MODE, 3>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((wu2_conv_kernel<T, MODE, 5>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((wu2_conv_kernel<T, MODE, 6>), grid, dim3(256), 0, s, a); break;
    case 9:
      if constexpr (MODE == WU2_CONV3) {
        hipLaunchKernelGGL((wu2_conv_kernel<T, MODE, 9>), grid, dim3(256), 0, s, a);
        break;
      } else {
        return hipErrorInvalidValue;
      }
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

template <typename T>
static hipError_t wu2_conv_dispatch(const WU2ConvArgs& a, dim3 grid, hipStream_t s) {
  if (a.mode == WU2_CONV5) return wu2_conv_dispatch_nco<T, WU2_CONV5>(a, grid, s);
  if (a.mode == WU2_CONV3) return wu2_conv_dispatch_nco<T, WU2_CONV3>(a, grid, s);
  if (a.mode == WU2_DOWN4) return wu2_conv_dispatch_nco<T, WU2_DOWN4>(a, grid, s);
  return wu2_conv_dispatch_nco<T, WU2_UP4>(a, grid, s);
}

hipError_t launch_wu2_conv(int dtype, const WU2ConvArgs& a, hipStream_t s) {
  if (a.mode < WU2_CONV5 || a.mode > WU2_UP4 || a.B < 1 || a.B > 65535 || a.Lin < 1 || a.Lout < 1) return hipErrorInvalidValue;
  if (!a.src || !a.w || !a.bias || !a.out) return hipErrorInvalidValue;
  if (a.Cin % 8 || a.Cin < 8 || a.Cin > 96 || a.Cout % 8 || a.Cout < 8 || a.Cout > 144) return hipErrorInvalidValue;
  if (((a.mode == WU2_CONV5 || a.mode == WU2_CONV3) && a.Lout != a.Lin) || (a.mode == WU2_DOWN4 && a.Lin != 2 * a.Lout) ||
      (a.mode == WU2_UP4 && a.Lout != 2 * a.Lin))
    return hipErrorInvalidValue;
  if ((a.scale == nullptr) != (a.shift == nullptr) || (a.film && (!a.scale || a.mode != WU2_CONV5))) return hipErrorInvalidValue;
  if (a.enc_dim && (a.enc_dim != a.Cout || a.enc_dim > 96 || a.enc_dim % 2)) return hipErrorInvalidValue;
  if (a.enc_dim && !a.lv.levels && (!a.lv.t_dev || (!a.lv.time_step && !a.lv.table))) return hipErrorInvalidValue;
  const dim3 grid((a.Lout + kWu2Tile - 1) / kWu2Tile, a.B);
  if (dtype == DT_F32) return wu2_conv_dispatch<float>(a, grid, s);
  if (dtype == DT_BF16) return wu2_conv_dispatch<bf16_t>(a, grid, s);
  return wu2_conv_dispatch<f16_t>(a, grid, s);
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
