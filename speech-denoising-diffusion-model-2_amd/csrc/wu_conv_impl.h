// The device code the two 1-D Wave-U-Nets share (included by waveunet.hip and waveunet2.hip, one
// translation unit per network): the noise level, the stem and the MFMA convolution.  What differs
// between the networks is a compile-time policy `Net` that each .hip file defines.
#pragma once
#include "conv_common.h"
#include "wu_kernels.h"

namespace sddm {

__device__ __forceinline__ float wu_level(const WULevel& lv, int b) {
  if (lv.levels) return lv.levels[b];
  const int t = *lv.t_dev;
  return lv.time_step ? (float)t : lv.table[t];
}

// ---------------- stem: Conv1d(2, C, 5, padding 2) on the two fp32 sources ----------------
// One thread per position computes its C channels from the 5-tap windows of both sources.  The
// stored values go through LDS once more for the statistics: thread (c, seg) sums channel c over the
// 32 positions of segment seg in ascending order -- 8 slots per block.
//   NORM (Waveunet3): the sources are activated in registers, SiLU(GN(2, 2)) from scale / shift (the
//     zero padding applies to the activated signal), and the noise constant rides on the bias.
//   !NORM (Waveunet2): the raw sources; the kernel steps t_dev (nothing in it reads the counter).
template <typename T, int C, bool NORM>
__global__ __launch_bounds__(256) void wu_stem_kernel(WUStemArgs a) {
  __shared__ float w[C * 10], cb[C], vals[kWuStemTile][C + 1];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * kWuStemTile;
  if (!NORM && a.t_dev && blockIdx.x == 0 && b == 0 && tid == 0) *a.t_dev -= 1;   // this step's t
  for (int i = tid; i < C * 10; i += 256) w[i] = a.w[i];
  if (tid < C) {
    if constexpr (NORM) cb[tid] = a.bias[tid] + (a.nw[tid] * wu_level(a.lv, b) + a.nb[tid]);
    else cb[tid] = a.bias[tid];
  }
  __syncthreads();
  float s0 = 1.f, h0 = 0.f, s1 = 1.f, h1 = 0.f;
  if constexpr (NORM) { s0 = a.scale[b * 2]; h0 = a.shift[b * 2]; s1 = a.scale[b * 2 + 1]; h1 = a.shift[b * 2 + 1]; }
  const float* c = a.cond + (size_t)b * a.L;
  const float* x = a.x + (size_t)b * a.L;
  const int t = t0 + tid;
  float cv[5], xv[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int m = t + k - 2;
    const bool in = t < a.L && m >= 0 && m < a.L;
    if constexpr (NORM) {
      cv[k] = in ? silu(c[m] * s0 + h0) : 0.f;
      xv[k] = in ? silu(x[m] * s1 + h1) : 0.f;
    } else {
      cv[k] = in ? c[m] : 0.f;
      xv[k] = in ? x[m] : 0.f;
    }
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

template <int C, bool NORM>
hipError_t wu_stem_launch(int dtype, const WUStemArgs& a, hipStream_t s) {
  if (a.B < 1 || a.L < 1 || !a.stats) return hipErrorInvalidValue;
  if (NORM && (!a.scale || !a.shift || !a.nw || !a.nb)) return hipErrorInvalidValue;
  const dim3 grid((a.L + kWuStemTile - 1) / kWuStemTile, a.B);
  if (dtype == DT_F32) hipLaunchKernelGGL((wu_stem_kernel<float, C, NORM>), grid, dim3(256), 0, s, a);
  else if (dtype == DT_BF16) hipLaunchKernelGGL((wu_stem_kernel<bf16_t, C, NORM>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((wu_stem_kernel<f16_t, C, NORM>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

// ---------------- the MFMA convolution ----------------
// Block = 4 waves = 128 output positions x all Cout channels; wave w owns 32 positions as two
// 16-column B fragments and NCO = ceil(Cout / 16) A fragments, i.e. up to 9 x 2 accumulator tiles.
// Per 32-channel chunk of the input the block stages the slab of input rows its outputs touch (the
// network's input transform applied here, once per element; rows outside [0, Lin) zero), then every
// tap reads its B fragments from the slab at a row offset.  The global loads of chunk c + 1 are
// issued (into registers) before the MFMAs of chunk c and stored to LDS after them.  Weights
// (L2-resident: the networks have 1.3 M and 0.45 M parameters): bf16 / f16 stage the chunk's
// [taps][16 NCO][32] image through LDS with the slab; fp32 images would not fit the 64 KB of static
// LDS, so fp32 loads the NCO A fragments of a tap together from global memory, one tap ahead of the
// MFMAs that use them.
//   WU_CONV5: output o, tap k reads input o + k - 2; slab rows [t0 - 2, t0 + 130).
//   WU_CONV3: output o, tap k reads input o + k - 1; slab rows [t0 - 1, t0 + 129).
//   WU_DOWN4: output o, tap k reads input 2 o + k - 1; slab rows [2 t0 - 1, 2 t0 + 257).
//   WU_UP4:   ConvTranspose1d: out[2 i - 1 + k] += W[k] x[i].  Output 2 m + ph takes the taps of
//             its parity only: ph = 0: (k = 1, x[m]), (k = 3, x[m - 1]); ph = 1: (k = 0, x[m + 1]),
//             (k = 2, x[m]).  A block owns 64 input positions m; wave w runs phase w & 1 on the
//             32 positions m0 + 32 (w >> 1) ..., so a fragment's 16 columns share their taps.
//             Slab rows [m0 - 1, m0 + 65).
// LO: the slab's first row sits LO (WU_DOWN4: 2 t0 - LO) in front of the block's first position.
template <int MODE> struct WuGeom;
template <> struct WuGeom<WU_CONV5> { static constexpr int ROWS = kWuTile + 4, TAPS = 5, KW = 5, LO = 2; };
template <> struct WuGeom<WU_CONV3> { static constexpr int ROWS = kWuTile + 2, TAPS = 3, KW = 3, LO = 1; };
template <> struct WuGeom<WU_DOWN4> { static constexpr int ROWS = 2 * kWuTile + 2, TAPS = 4, KW = 4, LO = 1; };
template <> struct WuGeom<WU_UP4> { static constexpr int ROWS = kWuTile / 2 + 2, TAPS = 2, KW = 4, LO = 1; };

// The policy Net of a network (Wu3Conv in waveunet.hip, Wu2Conv in waveunet2.hip) supplies
//   Args        the kernel's argument struct.  The kernel itself reads src, Lin, Cin, scale, shift,
//               w, bias, out, Lout, Cout, stats; the rest is the policy's
//   kPartial    Cin may stop short of a 32-channel chunk and Cout of a 16-row fragment (both are
//               multiples of 8): the missing channels are zero-filled where they are staged (LDS, or
//               the fragment registers in fp32), never in memory, and stores and statistics are
//               masked to the true Cout.  false: Cin % 32 == 0 and Cout == 16 NCO at compile time
//   kSplit      the layer's Cout is split over blockIdx.z in groups of Args::gco channels (a multiple
//               of 16, at most 16 NCO): block z stages its group's weight rows and owns its channels'
//               stores and statistics; every group stages and transforms the input slab again.
//               false: one block holds the whole Cout
//   kResidual   the kernel has Waveunet3's residual paths (Args then has res_mode, res, RC, rw, cond,
//               x, rw2, shortcut): res_mode == 2 appends the K chunks of a 1x1 conv over `res`
//               [B][Lout][RC] with the weights rw [Cout][RC] (one tap at the centre row of the slab, no
//               input transform); res_mode 1 / 3 and the shortcut are added in the epilogue
//   Lds         { alignas(16) float sc[], sh[]; ... }: the row's GroupNorm scale / shift, and what
//               prologue() adds.  Each array 16-byte aligned: without it the transform's reads of
//               sc + cq / sh + cq fall from ds_read_b128 to pairs of 4-byte reads
//   prologue    fills the rest of Lds (visible behind the first chunk's barriers)
//   transform   the input transform of one 16-byte unit (position pos, channels cq ...) of the main conv
//   Epi / epi   what the epilogue needs once per thread;  Row / row  the constants of the 4 channels
//               cb ... of an accumulator (okc: they are inside Cout), bias[4] among them;  value  turns
//               v = accumulator + bias (+ residual, + shortcut) into the 4 floats to store
template <typename T, int MODE, int NCO, typename Net>
__global__ __launch_bounds__(256) void wu_conv_kernel(typename Net::Args a) {
  using Geom = WuGeom<MODE>;
  constexpr int ES = (int)sizeof(T), UE = 16 / ES;          // elements per 16-byte unit
  constexpr int UPR = 32 / UE;                               // units per 32-channel row
  constexpr int RS = 32 * ES + 16;                           // padded LDS row stride (bytes)
  constexpr int ROWS = Geom::ROWS, TAPS = Geom::TAPS, KW = Geom::KW;
  constexpr bool WL = ES == 2;                               // 16-bit: the chunk's weights go through LDS (52 KB at most with the slab)
  constexpr int CP = NCO * 16;                               // Cout padded to whole fragments
  constexpr int WROWS = CP * KW;
  __shared__ __attribute__((aligned(16))) char slab[ROWS * RS];
  __shared__ __attribute__((aligned(16))) char wl[WL ? WROWS * RS : 16];
  __shared__ typename Net::Lds lds;

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, tile = blockIdx.x;
  const int Cin = a.Cin, CoutT = Net::kPartial ? a.Cout : CP;
  // kSplit: the block computes the channels [co0, co0 + Cout) of the layer's CoutT
  int co0 = 0, Cout = CoutT;
  if constexpr (Net::kSplit) { co0 = blockIdx.z * a.gco; Cout = min(CoutT - co0, a.gco); }
  const int ph = MODE == WU_UP4 ? (wave & 1) : 0;
  // first output position of the block (WU_UP4: first input position m0) and first slab row
  const int t0 = MODE == WU_UP4 ? tile * (kWuTile / 2) : tile * kWuTile;
  const int in_lo = MODE == WU_DOWN4 ? 2 * t0 - Geom::LO : t0 - Geom::LO;
  // column base of the wave's fragments inside the block
  const int wcol = MODE == WU_UP4 ? (wave >> 1) * 32 : wave * 32;

  const bool gn = a.scale != nullptr;
  if (gn)
    for (int c = tid; c < Cin; c += 256) {
      lds.sc[c] = a.scale[(size_t)b * Cin + c];
      lds.sh[c] = a.shift[(size_t)b * Cin + c];
    }
  Net::prologue(a, lds, b, tid);

  f32x4 acc[NCO][2];
#pragma unroll
  for (int c = 0; c < NCO; ++c)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nck = Net::kPartial ? (Cin + 31) / 32 : Cin / 32;
  int nch = nck;
  if constexpr (Net::kResidual) nch += a.res_mode == 2 ? a.RC / 32 : 0;
  // K chunk ch < nck: channels [32 ch, 32 ch + 32) of the main conv's input; behind them (kResidual)
  // the chunks of the 1x1 conv over `res`
  auto is_main = [&](int ch) { return !Net::kResidual || ch < nck; };
  // fp32: the A fragments of tap k of chunk ch from global memory
  auto load_a = [&](int ch, int kk, Frag<T>* af) {
    const bool main = is_main(ch);
    const int c0 = (main ? ch : ch - nck) * 32, cg = c0 + g * 8;
    const int wk = MODE == WU_UP4 ? (1 - ph) + 2 * kk : kk;
    const T* wp = (const T*)a.w + (size_t)wk * Cin + c0 + g * 8;
    int wstride = KW * Cin;
    if constexpr (Net::kResidual)
      if (!main) { wp = (const T*)a.rw + c0 + g * 8; wstride = a.RC; }
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      const int co = c * 16 + l16;
      if (!Net::kPartial || (co < Cout && cg < Cin)) af[c] = load_frag<T>((const char*)(wp + (size_t)(co0 + co) * wstride));
      else af[c] = Frag<T>{};
    }
  };
  // staging registers of one chunk: the slab units and (WL) the weight units of this thread
  constexpr int SIT = (ROWS * UPR + 255) / 256, WIT = WL ? (WROWS * UPR + 255) / 256 : 1;
  f32x4 sv[SIT], wv[WIT];
  // gload / lstore spell `ch < nck` out and pick every per-chunk value by its own select, in this
  // order.  Other forms of the same thing (is_main(ch), one struct per chunk, values overwritten
  // under `if (!main)`) made the compiler load the kernel arguments piecemeal inside the chunk loop
  // and serialise the transform's exp / rcp chains: 2 - 3 % on Waveunet3's 16-bit launches
  auto gload = [&](int ch) {
    bool main = true;
    if constexpr (Net::kResidual) main = ch < nck;
    const int c0 = (main ? ch : ch - nck) * 32;
    const T* sp; int Ls, Cs;
    if constexpr (Net::kResidual) {
      sp = main ? (const T*)a.src + (size_t)b * a.Lin * Cin : (const T*)a.res + (size_t)b * a.Lout * a.RC;
      Ls = main ? a.Lin : a.Lout, Cs = main ? Cin : a.RC;
    } else {
      sp = (const T*)a.src + (size_t)b * a.Lin * Cin, Ls = a.Lin, Cs = Cin;
    }
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r;
      sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < ROWS * UPR && pos >= 0 && pos < Ls && (!Net::kPartial || c0 + q * UE < Cs)) sv[j] = *(const f32x4*)(sp + (size_t)pos * Cs + c0 + q * UE);
    }
    if (WL) {                              // weight rows (co, tap) of the chunk, in their global order
      int kwn = KW; const T* wp = (const T*)a.w;
      if constexpr (Net::kResidual) { kwn = main ? KW : 1; wp = main ? (const T*)a.w : (const T*)a.rw; }
      if constexpr (Net::kSplit) wp += (size_t)co0 * KW * Cin;
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        if (Net::kPartial) wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // a compile-time row count lets whole iterations lose their bound check
        if ((Net::kPartial ? r < Cout * kwn && c0 + q * UE < Cs : u < CP * kwn * UPR)) wv[j] = *(const f32x4*)(wp + (size_t)r * Cs + c0 + q * UE);
      }
    }
  };
  auto lstore = [&](int ch) {
    bool main = true;
    if constexpr (Net::kResidual) main = ch < nck;
    const int c0 = (main ? ch : ch - nck) * 32;
    int Ls = a.Lin, kwn = KW;
    if constexpr (Net::kResidual) Ls = main ? a.Lin : a.Lout, kwn = main ? KW : 1;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r, cq = c0 + q * UE;
      if (u < ROWS * UPR) {
        f32x4 v = sv[j];
        if (main && gn && pos >= 0 && pos < Ls && (!Net::kPartial || cq < Cin)) v = Net::template transform<T>(a, lds, v, b, pos, cq);
        *(f32x4*)(slab + r * RS + q * 16) = v;
      }
    }
    if (WL) {                              // LDS row = tap * CP + co: a tap's channels are consecutive rows
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        const int co = r / kwn, wk = r - co * kwn;
        if (u < CP * kwn * UPR) *(f32x4*)(wl + (wk * CP + co) * RS + q * 16) = wv[j];
      }
    }
  };
  Frag<T> af[NCO];
  if (!WL) load_a(0, 0, af);
  gload(0);
  for (int ch = 0; ch < nch; ++ch) {
    const bool main = is_main(ch);
    __syncthreads();                       // the previous chunk's fragments are read; Lds is visible
    lstore(ch);
    __syncthreads();
    if (ch + 1 < nch) gload(ch + 1);       // the next chunk's loads fly during this chunk's MFMAs
    const int ntap = main ? TAPS : 1;
    for (int k = 0; k < ntap; ++k) {
      Frag<T> an[NCO];
      const bool more = !WL && (k + 1 < ntap || ch + 1 < nch);
      if (more) load_a(k + 1 < ntap ? ch : ch + 1, k + 1 < ntap ? k + 1 : 0, an);
      if (WL) {
        const int wk = !main ? 0 : (MODE == WU_UP4 ? (1 - ph) + 2 * k : k);
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = load_frag<T>(wl + (wk * CP + c * 16 + l16) * RS + g * 8 * ES);
      }
      // slab row of column 0 of the wave's first fragment
      int r0, rstep = 1;
      if (!main) r0 = wcol + Geom::LO;                                    // the 1x1 conv: the centre row (only under WU_CONV5: launch_wu_conv refuses res_mode elsewhere)
      else if (MODE == WU_CONV5 || MODE == WU_CONV3) r0 = wcol + k;
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
  const int nslots = 4 * gridDim.x;
  int opos[2];
  bool ok[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = wcol + p * 16 + l16;
    opos[p] = MODE == WU_UP4 ? 2 * (t0 + col) + ph : t0 + col;
    ok[p] = opos[p] < a.Lout;
  }
  const typename Net::Epi epi = Net::epi(a, b);
  float rc[2] = {0.f, 0.f}, rx[2] = {0.f, 0.f};      // res_mode 3: the raw fp32 inputs at the thread's positions
  if constexpr (Net::kResidual) {
    if (a.res_mode == 3) {
#pragma unroll
      for (int p = 0; p < 2; ++p)
        if (ok[p]) {
          rc[p] = a.cond[(size_t)b * a.Lout + opos[p]];
          rx[p] = a.x[(size_t)b * a.Lout + opos[p]];
        }
    }
  }
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    const int cb = c * 16 + 4 * g;
    const bool okc = !Net::kPartial || cb < Cout;   // Cout % 8 == 0: the 4 channels of an accumulator are in or out together
    const typename Net::Row row = Net::row(a, lds, epi, co0 + cb, okc);
    float s[4] = {0.f, 0.f, 0.f, 0.f}, ss[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (ok[p] && okc) {
        const size_t o = ((size_t)b * a.Lout + opos[p]) * CoutT + co0 + cb;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[c][p][i] + row.bias[i];
        // The residual and the shortcut stay in this body, not behind a hook: which product of the
        // res_mode 3 term is fused into the FMA follows how the vectoriser packs this statement,
        // and that follows the code around it (tests/test_gpu_seq_digests.py pins the bits)
        if constexpr (Net::kResidual) {
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
        }
        Net::value(epi, row, v);
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
          float* st = a.stats + (((size_t)b * nslots + tile * 4 + wave) * CoutT + co0 + cb + i) * 2;
          st[0] = ts;
          st[1] = tss;
        }
      }
    }
  }
}

// dtype, then MODE; Net::launch_nco<T, MODE> picks NCO among the network's instantiations
template <typename T, typename Net>
hipError_t wu_conv_dispatch_mode(const typename Net::Args& a, dim3 grid, hipStream_t s) {
  if (a.mode == WU_CONV5) return Net::template launch_nco<T, WU_CONV5>(a, grid, s);
  if (a.mode == WU_CONV3) return Net::template launch_nco<T, WU_CONV3>(a, grid, s);
  if (a.mode == WU_DOWN4) return Net::template launch_nco<T, WU_DOWN4>(a, grid, s);
  return Net::template launch_nco<T, WU_UP4>(a, grid, s);
}

template <typename Net>
hipError_t wu_conv_dispatch(int dtype, const typename Net::Args& a, hipStream_t s) {
  const dim3 grid((a.Lout + kWuTile - 1) / kWuTile, a.B);
  if (dtype == DT_F32) return wu_conv_dispatch_mode<float, Net>(a, grid, s);
  if (dtype == DT_BF16) return wu_conv_dispatch_mode<bf16_t, Net>(a, grid, s);
  return wu_conv_dispatch_mode<f16_t, Net>(a, grid, s);
}

}  // namespace sddm
