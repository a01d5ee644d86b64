// Waveunet's short levels: the MFMA convolution with the batch folded into the column dimension.
//
// Levels 5 to 11 of the twelve-level Waveunet are shorter than wu_conv_kernel's 128-position tile
// (64, 32, 16 and 8 positions at the config's 16384 samples, at 216 to 288 channels): launched per
// batch row, every block streams the layer's weights to fill a fraction of its columns.  Here the
// 128 columns of a block are positions of the flattened [B * L] axis -- activations are [B][L][C],
// so consecutive rows are contiguous and the slab is staged as that of one long row -- and the
// batch rows of a block share the weights it stages.
//
// A block owns whole batch rows: rpb = min(128 / L, 16) of them (WU_UP4: 64 / Lin, the block owns
// input positions), so a row's statistics lie in one block.  What depends on the row b = col / L:
//   * the halo: a tap that leaves the column's own row reads zero.  Neighbouring rows of the block
//     sit in the slab (transformed), so the B fragment of such a lane is zeroed when it is read;
//     slab rows outside the block's batch rows are staged as zero
//   * GroupNorm scale / shift: staged per K chunk as [row][32 channels], double-buffered, loaded
//     with the chunk's slab; the FiLM tensor is indexed by the flat position; the encoding and the
//     noise level are per row ([row][channel] in LDS, computed behind the K loop)
//   * the statistics: the stored values of a fragment's 16 channels go through LDS once and are
//     added in the order the per-row path adds them -- per (row, channel) the four 32-position slots
//     of wu_conv_kernel's tile, each the balanced tree of row_sum16 over a lane's two columns, then
//     per (row, group of 8) wu_gn_finalize's fp64 tree -- and the block writes the layer's scale /
//     shift itself.  No atomics, no finalize launch, a row's result does not depend on which rows
//     share its block, and the two paths give the same bits.
// The K order per output is wu_conv_kernel's (chunk-major, taps inside; fp32: the same 16x16x4
// steps), and so are the weight staging and the split of Cout over blockIdx.z.
#include "wu1_kernels.h"
#include "wu2_conv_policy.h"

namespace sddm {

template <typename T, int MODE, int NCO>
__global__ __launch_bounds__(256) void wu_fold_kernel(WU1FoldArgs a) {
  using Geom = WuGeom<MODE>;
  constexpr int ES = (int)sizeof(T), UE = 16 / ES;          // elements per 16-byte unit
  constexpr int UPR = 32 / UE;                               // units per 32-channel row
  constexpr int RS = 32 * ES + 16;                           // padded LDS row stride (bytes)
  constexpr int ROWS = Geom::ROWS, TAPS = Geom::TAPS, KW = Geom::KW;
  constexpr bool WL = ES == 2;                               // 16-bit: the chunk's weights go through LDS
  constexpr int CP = NCO * 16;
  constexpr int WROWS = CP * KW;
  constexpr int CAP = MODE == WU_UP4 ? kWuTile / 2 : kWuTile;   // columns of the block's own axis (WU_UP4: input positions)
  constexpr int SLAB = ROWS * RS, SMEM = SLAB + (WL ? WROWS * RS : 0);
  constexpr int VS = 17;                                     // padded row of the statistics image
  static_assert(SMEM >= kWuTile * VS * 4 && SMEM >= kWu1FoldRows * CP * 4, "the epilogue's images reuse the slab and weight space");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];
  // [scale | shift][buffer][row][channel of the chunk]; behind the K loop the statistics partials
  __shared__ __attribute__((aligned(16))) float sch[2][2][kWu1FoldRows][32];
  float (*scc)[kWu1FoldRows][32] = sch[0];
  float (*shc)[kWu1FoldRows][32] = sch[1];
  char* slab = smem;
  char* wl = smem + SLAB;

  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l16 = lane & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Cin = a.Cin, CoutT = a.Cout, Li = a.Lin, Lo = a.Lout;
  const int co0 = blockIdx.z * a.gco, Cout = min(CoutT - co0, a.gco);
  const int ph = MODE == WU_UP4 ? (wave & 1) : 0;
  const int LU = MODE == WU_UP4 ? Li : Lo;                   // row length on the block's own axis
  const int rpb = min(CAP / LU, kWu1FoldRows);
  const int b0 = blockIdx.x * rpb, nb = min(rpb, a.B - b0);  // the block's batch rows
  const int ncol = nb * LU;                                  // its valid columns
  const int t0 = b0 * LU;                                    // flat position of column 0
  const int in_lo = (MODE == WU_DOWN4 ? 2 * t0 : t0) - Geom::LO;   // flat input position of slab row 0
  const int i_lo = b0 * Li, i_hi = (b0 + nb) * Li;           // the block's own input positions
  const int wcol = MODE == WU_UP4 ? (wave >> 1) * 32 : wave * 32;
  const bool gn = a.scale != nullptr;
  const bool film = a.film != nullptr;

  f32x4 acc[NCO][2];
#pragma unroll
  for (int c = 0; c < NCO; ++c)
#pragma unroll
    for (int p = 0; p < 2; ++p) acc[c][p] = f32x4{0.f, 0.f, 0.f, 0.f};

  // per column: its position inside its row, for the halo mask
  int cl[2];
  bool okcol[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = wcol + p * 16 + l16;
    okcol[p] = col < ncol;
    cl[p] = col - (col / LU) * LU;
  }

  const int nch = (Cin + 31) / 32;
  auto load_a = [&](int ch, int kk, Frag<T>* af) {             // fp32: the A fragments of tap kk of chunk ch
    const int c0 = ch * 32, cg = c0 + g * 8;
    const int wk = MODE == WU_UP4 ? (1 - ph) + 2 * kk : kk;
    const T* wp = (const T*)a.w + (size_t)wk * Cin + c0 + g * 8;
    const int wstride = KW * Cin;
#pragma unroll
    for (int c = 0; c < NCO; ++c) {
      const int co = c * 16 + l16;
      if (co < Cout && cg < Cin) af[c] = load_frag<T>((const char*)(wp + (size_t)(co0 + co) * wstride));
      else af[c] = Frag<T>{};
    }
  };
  constexpr int SIT = (ROWS * UPR + 255) / 256, WIT = WL ? (WROWS * UPR + 255) / 256 : 1;
  f32x4 sv[SIT], wv[WIT];
  f32x2 scv = f32x2{0.f, 0.f}, shv = scv;                     // this thread's share of the chunk's scale / shift
  const int srow = tid >> 4, sc2 = (tid & 15) * 2;
  auto gload = [&](int ch) {
    const int c0 = ch * 32;
    const T* sp = (const T*)a.src;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r;
      sv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (u < ROWS * UPR && pos >= i_lo && pos < i_hi && c0 + q * UE < Cin) sv[j] = *(const f32x4*)(sp + (size_t)pos * Cin + c0 + q * UE);
    }
    scv = f32x2{0.f, 0.f}; shv = scv;
    if (gn && srow < nb && c0 + sc2 < Cin) {
      scv = *(const f32x2*)(a.scale + (size_t)(b0 + srow) * Cin + c0 + sc2);
      shv = *(const f32x2*)(a.shift + (size_t)(b0 + srow) * Cin + c0 + sc2);
    }
    if (WL) {
      const T* wp = (const T*)a.w + (size_t)co0 * KW * Cin;
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        wv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (r < Cout * KW && c0 + q * UE < Cin) wv[j] = *(const f32x4*)(wp + (size_t)r * Cin + c0 + q * UE);
      }
    }
  };
  auto sstore = [&](int ch) {                                  // the chunk's scale / shift image
    *(f32x2*)&scc[ch & 1][srow][sc2] = scv;
    *(f32x2*)&shc[ch & 1][srow][sc2] = shv;
  };
  auto lstore = [&](int ch) {
    const int c0 = ch * 32;
#pragma unroll
    for (int j = 0; j < SIT; ++j) {
      const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
      const int pos = in_lo + r, cq = c0 + q * UE;
      if (u < ROWS * UPR) {
        f32x4 v = sv[j];
        if (gn && pos >= i_lo && pos < i_hi && cq < Cin) {
          const int rl = (pos - i_lo) / Li;
          f32x4 fs = f32x4{0.f, 0.f, 0.f, 0.f}, fh = fs;
          if (film) {
            const T* fp = (const T*)a.film + (size_t)pos * (2 * Cin) + cq;
            fh = *(const f32x4*)fp;
            fs = *(const f32x4*)(fp + Cin);
          }
          v = wu2_transform<T>(v, &scc[ch & 1][rl][q * UE], &shc[ch & 1][rl][q * UE], film, fs, fh);
        }
        *(f32x4*)(slab + r * RS + q * 16) = v;
      }
    }
    if (WL) {
#pragma unroll
      for (int j = 0; j < WIT; ++j) {
        const int u = tid + j * 256, r = u / UPR, q = u - r * UPR;
        const int co = r / KW, wk = r - co * KW;
        if (u < CP * KW * UPR) *(f32x4*)(wl + (wk * CP + co) * RS + q * 16) = wv[j];
      }
    }
  };
  Frag<T> af[NCO];
  if (!WL) load_a(0, 0, af);
  gload(0);
  sstore(0);
  for (int ch = 0; ch < nch; ++ch) {
    __syncthreads();                       // the previous chunk's fragments are read; this chunk's scale / shift are visible
    lstore(ch);
    __syncthreads();
    if (ch + 1 < nch) gload(ch + 1);
    for (int k = 0; k < TAPS; ++k) {
      Frag<T> an[NCO];
      const bool more = !WL && (k + 1 < TAPS || ch + 1 < nch);
      if (more) load_a(k + 1 < TAPS ? ch : ch + 1, k + 1 < TAPS ? k + 1 : 0, an);
      if (WL) {
        const int wk = MODE == WU_UP4 ? (1 - ph) + 2 * k : k;
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = load_frag<T>(wl + (wk * CP + c * 16 + l16) * RS + g * 8 * ES);
      }
      // slab row of column 0 of the wave's first fragment, and the tap's offset inside the column's row
      int r0, rstep = 1, ioff, imul = 1;
      if (MODE == WU_CONV5 || MODE == WU_CONV3) { r0 = wcol + k; ioff = k - Geom::LO; }
      else if (MODE == WU_DOWN4) { r0 = 2 * wcol + k; rstep = 2; ioff = k - 1; imul = 2; }
      else { r0 = wcol + ph - k + 1; ioff = ph - k; }
      Frag<T> bf[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        bf[p] = load_frag<T>(slab + (r0 + (p * 16 + l16) * rstep) * RS + g * 8 * ES);
        const int il = imul * cl[p] + ioff;                    // the input position inside the column's own row
        if (il < 0 || il >= Li) bf[p] = Frag<T>{};             // the halo of the row is zero
      }
#pragma unroll
      for (int c = 0; c < NCO; ++c)
#pragma unroll
        for (int p = 0; p < 2; ++p) mfma_frag(acc[c][p], af[c], bf[p]);
      if (more) {
#pragma unroll
        for (int c = 0; c < NCO; ++c) af[c] = an[c];
      }
    }
    if (ch + 1 < nch) sstore(ch + 1);      // the other buffer: its last readers passed the barrier above
  }

  // epilogue: the slab and weight space is free behind this barrier
  __syncthreads();
  float* img = (float*)smem;
  float* par = &sch[0][0][0][0];           // [row][slot][channel of the fragment][2]
  const bool enc = a.enc_dim > 0;
  if (enc) {                               // PositionalEncoding of the block's rows, [row][channel of the group]
    const int half = a.enc_dim / 2;
    for (int i = tid; i < nb * Cout; i += 256) {
      const int rl = i / Cout, cc = i - rl * Cout, e = co0 + cc, k = e < half ? e : e - half;
      const float arg = wu_level(a.lv, b0 + rl) * expf(-9.210340371976184f * ((float)k / (float)half));
      img[rl * CP + cc] = e < half ? sinf(arg) : cosf(arg);
    }
    __syncthreads();
  }
  int oi[2], orow[2];                      // the column's output position inside the block, and its row
  size_t opos[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int col = wcol + p * 16 + l16;
    oi[p] = MODE == WU_UP4 ? 2 * col + ph : col;
    orow[p] = okcol[p] ? oi[p] / Lo : 0;
    opos[p] = (size_t)b0 * Lo + oi[p];
  }
  const bool stats = a.gamma != nullptr;
#pragma unroll
  for (int c = 0; c < NCO; ++c) {
    const int cb = c * 16 + 4 * g;
    const bool okc = cb < Cout;
    float bias[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bias[i] = okc ? a.bias[co0 + cb + i] : 0.f;
    float rv[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
      for (int i = 0; i < 4; ++i) rv[p][i] = 0.f;
      if (okcol[p] && okc) {
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          v[i] = acc[c][p][i] + bias[i];
          if (enc) v[i] = (v[i] > 0.f ? v[i] : 0.2f * v[i]) + img[orow[p] * CP + cb + i];
        }
        store4<T>((T*)a.out + opos[p] * CoutT + co0 + cb, v[0], v[1], v[2], v[3]);
#pragma unroll
        for (int i = 0; i < 4; ++i) rv[p][i] = round_t<T>(v[i]);
      }
    }
    if (stats) {                           // (block-uniform)
      __syncthreads();                     // the previous fragment's image and sums are read
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int i = 0; i < 4; ++i) img[oi[p] * VS + 4 * g + i] = rv[p][i];
      __syncthreads();
      // the (sum, sum of squares) of slot w of wu_conv_kernel's tile for this row: lane l of wave w
      // adds its two columns (p = 0, 1), row_sum16 adds the 16 lanes as a balanced tree
      for (int t = tid; t < nb * 64; t += 256) {
        const int rl = t >> 6, w = (t >> 4) & 3, chl = t & 15;
        const float* vp = img + (rl * Lo) * VS + chl;
        float xs[16], xq[16];
#pragma unroll
        for (int l = 0; l < 16; ++l) {
          xs[l] = 0.f;
          xq[l] = 0.f;
#pragma unroll
          for (int p = 0; p < 2; ++p) {
            const int j = MODE == WU_UP4 ? 2 * ((w >> 1) * 32 + p * 16 + l) + (w & 1) : w * 32 + p * 16 + l;
            if (j < Lo) {
              const float v = vp[j * VS];
              xs[l] += v;
              xq[l] = __builtin_fmaf(v, v, xq[l]);
            }
          }
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1)
#pragma unroll
          for (int l = 0; l < 16; l += 2 * o) {
            xs[l] += xs[l + o];
            xq[l] += xq[l + o];
          }
        par[((rl * 4 + w) * 16 + chl) * 2] = xs[0];
        par[((rl * 4 + w) * 16 + chl) * 2 + 1] = xq[0];
      }
      __syncthreads();
      // wu_gn_finalize's order: per slot the 8 channels of the group as a balanced tree in fp64,
      // then (slot 0 + slot 1) + (slot 2 + slot 3)
      for (int t = tid; t < nb * 2; t += 256) {
        const int rl = t >> 1, c8 = c * 16 + (t & 1) * 8;    // a GroupNorm group: 8 channels
        if (c8 < Cout) {
          double S[4], Q[4];
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            double e[8], q[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              e[j] = (double)par[((rl * 4 + w) * 16 + (t & 1) * 8 + j) * 2];
              q[j] = (double)par[((rl * 4 + w) * 16 + (t & 1) * 8 + j) * 2 + 1];
            }
            S[w] = ((e[0] + e[1]) + (e[2] + e[3])) + ((e[4] + e[5]) + (e[6] + e[7]));
            Q[w] = ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
          }
          const double s = (S[0] + S[1]) + (S[2] + S[3]), ss = (Q[0] + Q[1]) + (Q[2] + Q[3]);
          const double n = (double)Lo * 8;
          const double mean = s / n;
          double var = ss / n - mean * mean;
          var = var > 0.0 ? var : 0.0;
          const double rstd = 1.0 / sqrt(var + (double)a.eps);
          for (int j = 0; j < 8; ++j) {
            const int e = co0 + c8 + j;
            const double scale = (double)a.gamma[e] * rstd;
            a.oscale[(size_t)(b0 + rl) * CoutT + e] = (float)scale;
            a.oshift[(size_t)(b0 + rl) * CoutT + e] = (float)((double)a.beta[e] - mean * scale);
          }
        }
      }
    }
  }
}

template <typename T, int MODE>
static hipError_t wu_fold_launch_nco(const WU1FoldArgs& a, dim3 grid, hipStream_t s) {
  switch (a.gco / 16) {
    case 2: hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 3>), grid, dim3(256), 0, s, a); break;
    case 4: hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 4>), grid, dim3(256), 0, s, a); break;
    case 5: hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 5>), grid, dim3(256), 0, s, a); break;
    case 6: hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 6>), grid, dim3(256), 0, s, a); break;
    default:
      if constexpr (MODE == WU_CONV3) {
        if (a.gco == 112) hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 7>), grid, dim3(256), 0, s, a);
        else if (a.gco == 128) hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 8>), grid, dim3(256), 0, s, a);
        else if (a.gco == 144) hipLaunchKernelGGL((wu_fold_kernel<T, MODE, 9>), grid, dim3(256), 0, s, a);
        else return hipErrorInvalidValue;
        break;
      } else {
        return hipErrorInvalidValue;
      }
  }
  return hipGetLastError();
}

template <typename T>
static hipError_t wu_fold_launch_mode(const WU1FoldArgs& a, dim3 grid, hipStream_t s) {
  if (a.mode == WU_CONV5) return wu_fold_launch_nco<T, WU_CONV5>(a, grid, s);
  if (a.mode == WU_CONV3) return wu_fold_launch_nco<T, WU_CONV3>(a, grid, s);
  if (a.mode == WU_DOWN4) return wu_fold_launch_nco<T, WU_DOWN4>(a, grid, s);
  return wu_fold_launch_nco<T, WU_UP4>(a, grid, s);
}

hipError_t launch_wu1_fold(int dtype, const WU1FoldArgs& a0, hipStream_t s) {
  WU1FoldArgs a = a0;
  hipError_t e = wu1_conv_check(a);
  if (e != hipSuccess) return e;
  if (a.Lout >= kWuTile) return hipErrorInvalidValue;          // whole rows must fit a block
  if (a.gamma && a.enc_dim) return hipErrorInvalidValue;       // one epilogue image
  if ((a.gamma == nullptr) != (a.beta == nullptr) || (a.gamma && (!a.oscale || !a.oshift))) return hipErrorInvalidValue;
  if (a.gamma && (a.oscale == a.scale || a.oshift == a.shift)) return hipErrorInvalidValue;   // blocks of other groups still read the input's
  a.gco = wu1_conv_group(a.mode, a.Cout);
  const int rpb = wu1_fold_rows(a.mode, a.Lin, a.Lout);
  if (rpb < 1) return hipErrorInvalidValue;
  const dim3 grid((a.B + rpb - 1) / rpb, 1, (a.Cout + a.gco - 1) / a.gco);
  if (dtype == DT_F32) return wu_fold_launch_mode<float>(a, grid, s);
  if (dtype == DT_BF16) return wu_fold_launch_mode<bf16_t>(a, grid, s);
  return wu_fold_launch_mode<f16_t>(a, grid, s);
}

}  // namespace sddm
