// CAUNet (reference model/CAUNet.py) for gfx950: the conv family (first_conv, the dense / downsample /
// sub-pixel MFMA convolution with its LayerNorm + PReLU epilogue, final_conv + overlap-add), the
// FeatureWiseAffine MLPs and the Dual_Transformer at d_model 32.
//
// Every matrix product is an MFMA with the weights as A fragments read from global memory (packed once
// in the compute dtype, caunet.h) and the activations as B fragments.  In a 16-bit context activations
// are rounded where they enter an MFMA and where a conv stores them; LayerNorm, GroupNorm, softmax,
// the GRU's gates and state, PReLU and the affine are fp32.  No atomics and no block waits for
// another: every reduction runs in an order fixed by the block shape, and a row's result does not
// depend on the batch it is in.
//
// The Dual_Transformer's image ([dim2][dim1][32] fp32, 256 KiB at 256 frames) does not fit LDS, and
// nothing in an encoder layer but its GroupNorm couples the sequences, so the block is a chain of
// small kernels over token tensors in global memory: three per-token products (in_proj; out_proj +
// residual + norm1; linear2 + residual + norm2), the attention (one wave per sequence, head and 16
// queries, online softmax, scores and P V on the MFMA) and the GRU (16 sequences per block and
// direction, the state in LDS, the weights in registers).  linear2's kernel leaves (sum, M2) of its
// 64-token tile; the next per-token kernel combines an image's partials and applies
// x += GroupNorm(src) as it loads.
#include "caunet.h"

#include "cau_frag.h"

namespace sddm {
namespace {

__device__ __forceinline__ float cau_level(const WULevel& lv, int b) {
  if (lv.levels) return lv.levels[b];
  const int t = *lv.t_dev;
  return lv.time_step ? (float)t : lv.table[t];
}

// ---------------------------------------------------------------------------------------------
// first_conv, the noise MLPs, final_conv + overlap-add
// ---------------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void cau_first_kernel(CauFirstArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;    // over [B][F][128][16 channel quads]
  if (a.t_dev && i == 0) *a.t_dev -= 1;                          // this step's t
  const int64_t total = (int64_t)a.B * a.F * 128 * 16;
  if (i >= total) return;
  const int c = (int)(i & 15) * 4;
  const int64_t pos = i >> 4;
  const int w = (int)(pos & 127);
  const int64_t bf = pos >> 7;
  const int f = (int)(bf % a.F);
  const int64_t b = bf / a.F;
  const float u = a.cond[b * a.N + (int64_t)f * 64 + w], v = a.x[b * a.N + (int64_t)f * 64 + w];
  float o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = a.w[(c + j) * 2] * u + a.w[(c + j) * 2 + 1] * v + a.bias[c + j];
  store4<T>((T*)a.out + pos * 64 + c, o[0], o[1], o[2], o[3]);
}

__global__ __launch_bounds__(256) void cau_noise_kernel(CauNoiseArgs a) {
  __shared__ float enc[kCauEmb], hid[kCauMlpHid];
  const int l = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (tid < kCauEmb) {                                           // PositionalEncoding (CAUNet.py:49-57)
    const int k = tid & 31;
    const float arg = cau_level(a.lv, b) * expf(-9.210340371976184f * ((float)k / 32.0f));
    enc[tid] = tid < 32 ? sinf(arg) : cosf(arg);
  }
  __syncthreads();
  {
    const float* w = a.w1 + ((size_t)l * kCauMlpHid + tid) * kCauEmb;
    float s = a.b1[l * kCauMlpHid + tid];
    for (int k = 0; k < kCauEmb; ++k) s += w[k] * enc[k];
    hid[tid] = s >= 0.f ? s : a.a1[l * kCauMlpHid + tid] * s;
  }
  __syncthreads();
  const int OUT = a.affine ? 128 : 64;
  const size_t o = ((size_t)b * a.NL + l) * 64;
  if (tid < OUT) {
    const float* w = a.w2 + ((size_t)l * OUT + tid) * kCauMlpHid;
    float s = a.b2[l * OUT + tid];
    for (int k = 0; k < kCauMlpHid; ++k) s += w[k] * hid[k];
    if (!a.affine) { a.sc[o + tid] = 1.0f; a.sh[o + tid] = s; }
    else if (tid < 64) a.sc[o + tid] = 1.0f + s;                 // (1 + gamma) x + beta (CAUNet.py:74-76)
    else a.sh[o + tid - 64] = s;
  }
}

template <typename T> __global__ __launch_bounds__(256) void cau_final_kernel(CauFinalArgs a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;    // over [B][N]
  if (i >= (int64_t)a.B * a.N) return;
  const int64_t b = i / a.N, n = i - b * a.N;
  const int f1 = (int)(n >> 6), wlo = (int)(n & 63);
  float out = 0.f;
  // overlapAdd adds the frames in ascending order (CAUNet.py:37-39): frame f1 - 1, then f1
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int f = f1 - 1 + k, w = k ? wlo : wlo + 64;
    if (f < 0 || f >= a.F) continue;
    const T* p = (const T*)a.src + ((b * a.F + f) * 128 + w) * 64;
    float s = a.bias[0];
    for (int c = 0; c < 64; c += 4) {
      const f32x4 v = load4<T>(p + c);
#pragma unroll
      for (int j = 0; j < 4; ++j) s += a.w[c + j] * v[j];
    }
    out += s;
  }
  a.out[i] = out;
}

// ---------------------------------------------------------------------------------------------
// the convolution: wave j owns output channels 16 j .. 16 j + 15 (of each sub-pixel phase) and all
// 128 positions of the block, so a row's LayerNorm statistics are sums over the wave's own
// accumulators and lanes.  The block's input rows go through LDS one source at a time (at most
// 45 KiB in the 16-bit types, 90 KiB in fp32); the weights are read from global memory
// ---------------------------------------------------------------------------------------------
constexpr int kNPT = 8;   // position tiles of 16 per block
constexpr int kCauLdsC = 72;   // channel stride of a staged pixel: 64 + 8, so 16 neighbouring pixels spread over the banks

// s[pt][i] <- sum over the row that position tile pt (and the lane) belongs to
__device__ __forceinline__ void cau_row_sum(f32x4 (&s)[kNPT], int tpr, int lanes_w) {
#pragma unroll
  for (int st = 1; st < kNPT; st <<= 1) {
    if (st < tpr) {
      f32x4 t[kNPT];
#pragma unroll
      for (int pt = 0; pt < kNPT; ++pt) t[pt] = s[pt] + s[pt ^ st];
#pragma unroll
      for (int pt = 0; pt < kNPT; ++pt) s[pt] = t[pt];
    }
  }
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = s[pt][i];
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      if (lanes_w == 16) v += __shfl_xor(v, 8);
      s[pt][i] = v;
    }
  }
}

template <typename T, int MODE> __global__ __launch_bounds__(256) void cau_conv_kernel(CauConvArgs a) {
  constexpr int NR = MODE == CAU_UP ? 2 : 1, KH = MODE == CAU_DENSE ? 2 : 1;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int Wc = a.Wc, lw = 31 - __clz(Wc), Win = MODE == CAU_DOWN ? 2 * Wc : Wc, Wout = NR * Wc;
  const int F = a.F, R = a.B * F, row0 = blockIdx.x * (128 >> lw);
  int pb[kNPT], ph[kNPT], pw[kNPT];
  bool pv[kNPT];
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt) {
    const int p = pt * 16 + col;
    int rr = row0 + (p >> lw);
    pv[pt] = rr < R;
    rr = min(rr, R - 1);
    pb[pt] = rr / F;
    ph[pt] = rr - pb[pt] * F;
    pw[pt] = p & (Wc - 1);
  }
  f32x4 acc[NR][kNPT];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int pt = 0; pt < kNPT; ++pt) acc[r][pt] = f32x4{0.f, 0.f, 0.f, 0.f};

  // One source at a time goes through LDS: slab kh holds, for each of the block's rows, the input row
  // tap kh reads, Win + 2 pixels wide (a zero column each side) and kCauLdsC channels apart; rows above
  // the image, rows past the batch and the two side columns are zero, and the affine is applied (and
  // rounded to T) here, once per input value.  The taps then read B fragments without a mask.
  extern __shared__ __align__(16) char cau_smem[];
  T* tile = (T*)cau_smem;
  const int rpb = 128 >> lw, WP = Win + 2;
  int lbase[kNPT];
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt)
    lbase[pt] = ((((pt * 16 + col) >> lw) * WP) + (MODE == CAU_DOWN ? 2 * pw[pt] : pw[pt])) * kCauLdsC + 8 * g;
  const T* wgt = (const T*)a.w;
  const int KS = a.nsrc * KH * 3 * 2;
  int ks = 0;
  for (int s = 0; s < a.nsrc; ++s) {
    const T* sp = (const T*)a.src[s];
    const bool aff = s == a.aff_src;
    if (s > 0) __syncthreads();
    for (int i = threadIdx.x; i < KH * rpb * WP * 8; i += 256) {
      const int c8 = (i & 7) * 8, pix = i >> 3, cw = pix % WP, t = pix / WP, rl = t % rpb, kh = t / rpb;
      const int rr = row0 + rl, b = min(rr, R - 1) / F, h = rr - b * F;
      const int hin = MODE == CAU_DENSE ? h - (1 - kh) * a.dil : h, win = cw - 1;
      Frag<T> v = zero_frag<T>();
      if (rr < R && hin >= 0 && win >= 0 && win < Win) {
        v = load_t<T>(sp + (((size_t)b * F + hin) * Win + win) * 64 + c8);
        if (aff) {
          f32x4 lo, hi;
          frag_to_f32<T>(v, lo, hi);
          const float* sc = a.sc + (size_t)b * a.aff_ld + c8;
          const float* sh = a.sh + (size_t)b * a.aff_ld + c8;
          lo = lo * *(const f32x4*)sc + *(const f32x4*)sh;
          hi = hi * *(const f32x4*)(sc + 4) + *(const f32x4*)(sh + 4);
          v = frag_from_f32<T>(lo, hi);
        }
      }
      *(Frag<T>*)(tile + (size_t)pix * kCauLdsC + c8) = v;
    }
    __syncthreads();
    for (int kh = 0; kh < KH; ++kh)
      for (int kw = 0; kw < 3; ++kw) {
        const T* tap = tile + (kh * rpb * WP + kw) * kCauLdsC;
        for (int kc = 0; kc < 2; ++kc, ++ks) {
          Frag<T> wa[NR];
#pragma unroll
          for (int r = 0; r < NR; ++r) wa[r] = load_wgt<T>(wgt, r * 4 + wave, KS, ks, lane);
#pragma unroll
          for (int pt = 0; pt < kNPT; ++pt) {
            const Frag<T> bx = *(const Frag<T>*)(tap + lbase[pt] + kc * 32);
#pragma unroll
            for (int r = 0; r < NR; ++r) mfma_frag(acc[r][pt], wa[r], bx);
          }
        }
      }
  }

  // ---- + bias, LayerNorm over the row's Wout outputs (eps 1e-5), PReLU, store
  const int tpr = max(Wc >> 4, 1), lanes_w = min(Wc, 16);
  const float inv = 1.0f / (float)Wout;
  const int co = wave * 16 + 4 * g;
  f32x4 s[kNPT];
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt) s[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const f32x4 bias = *(const f32x4*)(a.bias + r * 64 + co);
#pragma unroll
    for (int pt = 0; pt < kNPT; ++pt) { acc[r][pt] += bias; s[pt] += acc[r][pt]; }
  }
  cau_row_sum(s, tpr, lanes_w);
  f32x4 mean[kNPT];
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt) {
    mean[pt] = s[pt] * inv;
    s[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < NR; ++r) { acc[r][pt] -= mean[pt]; s[pt] += acc[r][pt] * acc[r][pt]; }
  }
  cau_row_sum(s, tpr, lanes_w);
  const f32x4 alpha = *(const f32x4*)(a.alpha + co);
#pragma unroll
  for (int pt = 0; pt < kNPT; ++pt) {
    if (!pv[pt]) continue;
    f32x4 rstd;
#pragma unroll
    for (int i = 0; i < 4; ++i) rstd[i] = 1.0f / sqrtf(s[pt][i] * inv + 1e-5f);
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      const int wo = NR * pw[pt] + r;
      const float lw_ = a.lnw[wo], lb_ = a.lnb[wo];
      float y[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = acc[r][pt][i] * rstd[i] * lw_ + lb_;
        y[i] = v >= 0.f ? v : alpha[i] * v;
      }
      store4<T>((T*)a.out + (((size_t)pb[pt] * F + ph[pt]) * Wout + wo) * 64 + co, y[0], y[1], y[2], y[3]);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Dual_Transformer: per-token kernels.  A block is four waves of 16 tokens of one image.
// ---------------------------------------------------------------------------------------------
// TOK_OUTP: the output stage of tstnn.py:139-141, PReLU before the conv and nothing after it
enum { TOK_IN = 0, TOK_QKV = 1, TOK_PROJ = 2, TOK_LIN2 = 3, TOK_OUT = 4, TOK_OUTP = 5 };
struct CauTokArgs {
  int B, P;                     // images, tokens per image
  const void* xin;              // IN: x [tok][64]; PROJ: attention [tok][32]; LIN2: ReLU(GRU) [tok][128] (T)
  float* cur;                   // [tok][32] the block's running output (IN writes, QKV updates, OUT reads)
  const float* res;             // PROJ: cur; LIN2: norm1's output
  const float* gsrc;            // QKV / OUT: norm2's output whose GroupNorm is still to be added, or null
  const float* part; int npart; // its partials [B][npart][2]
  const float* gnw; const float* gnb;
  const void* w; const float* bias; const float* lnw; const float* lnb; const float* alpha;
  void* out;                    // QKV: [tok][96] (T); OUT: [tok][64] (T)
  float* dst;                   // PROJ / LIN2: the norm's output [tok][32]
  float* part_out;              // LIN2: [B][npart][2]
};

template <typename T, int MODE> __global__ __launch_bounds__(256) void cau_tok_kernel(CauTokArgs a) {
  __shared__ float red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int b = blockIdx.y, P = a.P;
  const int tok = blockIdx.x * kCauTokTile + wave * 16 + col;
  const bool valid = tok < P;
  const size_t gt = (size_t)b * P + min(tok, P - 1);
  const T* wgt = (const T*)a.w;

  if constexpr (MODE == TOK_IN) {
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const Frag<T> bx = load_t<T>((const T*)a.xin + gt * 64 + kc * 32 + 8 * g);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) mfma_frag(acc[nt], load_wgt<T>(wgt, nt, 2, kc, lane), bx);
    }
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int c = nt * 16 + 4 * g;
      f32x4 v = acc[nt] + *(const f32x4*)(a.bias + c);
      const f32x4 al = *(const f32x4*)(a.alpha + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = v[i] >= 0.f ? v[i] : al[i] * v[i];
      if (valid) *(f32x4*)(a.cur + gt * 32 + c) = v;
    }
  } else if constexpr (MODE == TOK_QKV || MODE == TOK_OUT || MODE == TOK_OUTP) {
    // cur += GroupNorm(1, 32, eps 1e-8)(gsrc) over the image: Chan's combination of the tile partials
    f32x4 lo = *(const f32x4*)(a.cur + gt * 32 + 8 * g), hi = *(const f32x4*)(a.cur + gt * 32 + 8 * g + 4);
    if (a.gsrc) {
      const float* pp = a.part + (size_t)b * a.npart * 2;
      const double n = (double)P * kCauD;
      double sm = 0.0;
      for (int i = 0; i < a.npart; ++i) sm += (double)pp[2 * i];
      const double mean = sm / n;
      double m2 = 0.0;
      for (int i = 0; i < a.npart; ++i) {
        const double cnt = (double)(min(kCauTokTile, P - i * kCauTokTile) * kCauD);
        const double dm = (double)pp[2 * i] / cnt - mean;
        m2 += (double)pp[2 * i + 1] + cnt * dm * dm;
      }
      const float mu = (float)mean, rstd = (float)(1.0 / sqrt(m2 / n + 1e-8));
      const f32x4 slo = *(const f32x4*)(a.gsrc + gt * 32 + 8 * g), shi = *(const f32x4*)(a.gsrc + gt * 32 + 8 * g + 4);
      lo += (slo - mu) * rstd * *(const f32x4*)(a.gnw + 8 * g) + *(const f32x4*)(a.gnb + 8 * g);
      hi += (shi - mu) * rstd * *(const f32x4*)(a.gnw + 8 * g + 4) + *(const f32x4*)(a.gnb + 8 * g + 4);
      if (MODE == TOK_QKV && valid) {
        *(f32x4*)(a.cur + gt * 32 + 8 * g) = lo;
        *(f32x4*)(a.cur + gt * 32 + 8 * g + 4) = hi;
      }
    }
    if constexpr (MODE == TOK_OUTP) {
      const f32x4 alo = *(const f32x4*)(a.alpha + 8 * g), ahi = *(const f32x4*)(a.alpha + 8 * g + 4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        lo[i] = lo[i] >= 0.f ? lo[i] : alo[i] * lo[i];
        hi[i] = hi[i] >= 0.f ? hi[i] : ahi[i] * hi[i];
      }
    }
    const Frag<T> bx = frag_from_f32<T>(lo, hi);
    constexpr int NT = MODE == TOK_QKV ? 6 : 4;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int c = nt * 16 + 4 * g;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      mfma_frag(v, load_wgt<T>(wgt, nt, 1, 0, lane), bx);
      v += *(const f32x4*)(a.bias + c);
      if constexpr (MODE == TOK_QKV) {
        if (nt < 2) v *= 0.35355339059327373f;                   // q scaled by head_dim^-0.5 = 8^-0.5
        if (valid) store4<T>((T*)a.out + gt * 96 + c, v[0], v[1], v[2], v[3]);
      } else if constexpr (MODE == TOK_OUT) {
        const f32x4 al = *(const f32x4*)(a.alpha + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = v[i] >= 0.f ? v[i] : al[i] * v[i];
        if (valid) store4<T>((T*)a.out + gt * 64 + c, v[0], v[1], v[2], v[3]);
      } else {
        if (valid) store4<T>((T*)a.out + gt * 64 + c, v[0], v[1], v[2], v[3]);
      }
    }
  } else {
    // PROJ / LIN2: product + bias + residual, LayerNorm over the token's 32 channels (eps 1e-5)
    constexpr int KC = MODE == TOK_PROJ ? 1 : 4;
    f32x4 v[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int kc = 0; kc < KC; ++kc) {
      const Frag<T> bx = load_t<T>((const T*)a.xin + gt * (32 * KC) + kc * 32 + 8 * g);
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) mfma_frag(v[nt], load_wgt<T>(wgt, nt, KC, kc, lane), bx);
    }
    float sum = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int c = nt * 16 + 4 * g;
      v[nt] += *(const f32x4*)(a.bias + c) + *(const f32x4*)(a.res + gt * 32 + c);
      sum += (v[nt][0] + v[nt][1]) + (v[nt][2] + v[nt][3]);
    }
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float mean = sum * (1.0f / kCauD);
    float q = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      v[nt] -= mean;
      q += (v[nt][0] * v[nt][0] + v[nt][1] * v[nt][1]) + (v[nt][2] * v[nt][2] + v[nt][3] * v[nt][3]);
    }
    q += __shfl_xor(q, 16);
    q += __shfl_xor(q, 32);
    const float rstd = 1.0f / sqrtf(q * (1.0f / kCauD) + 1e-5f);
    float ps = 0.f;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int c = nt * 16 + 4 * g;
      v[nt] = v[nt] * rstd * *(const f32x4*)(a.lnw + c) + *(const f32x4*)(a.lnb + c);
      if (valid) *(f32x4*)(a.dst + gt * 32 + c) = v[nt];
      ps += (v[nt][0] + v[nt][1]) + (v[nt][2] + v[nt][3]);
    }
    if constexpr (MODE == TOK_LIN2) {
      // the tile's (sum, M2 about the tile mean) of what it stored, for the image's GroupNorm
      if (!valid) ps = 0.f;
      for (int o = 32; o >= 1; o >>= 1) ps += __shfl_xor(ps, o);
      if (lane == 0) red[wave] = ps;
      __syncthreads();
      const float tot = (red[0] + red[1]) + (red[2] + red[3]);
      const float bm = tot / (float)(min(kCauTokTile, P - (int)blockIdx.x * kCauTokTile) * kCauD);
      float pq = 0.f;
      if (valid) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int i = 0; i < 4; ++i) pq += (v[nt][i] - bm) * (v[nt][i] - bm);
      }
      for (int o = 32; o >= 1; o >>= 1) pq += __shfl_xor(pq, o);
      __syncthreads();
      if (lane == 0) red[wave] = pq;
      __syncthreads();
      if (threadIdx.x == 0) {
        float* po = a.part_out + ((size_t)b * a.npart + blockIdx.x) * 2;
        po[0] = tot;
        po[1] = (red[0] + red[1]) + (red[2] + red[3]);
      }
    }
  }
}

// ---- self attention: one wave per (image, sequence, head, 16 queries); token of (sequence s,
// time t) = s * ss + t * ts.  Scores transposed (keys x queries) so the probabilities leave the
// MFMA in the layout the P V product takes them as B fragments: of every 32 keys, K slot 8 g + j
// is key 4 g + j of the first 16 and slot 8 g + 4 + j key 4 g + j of the second.
struct CauAttnArgs { const void* qkv; void* att; int nseq, L, ss, ts, P, QT; };

template <typename T> __global__ __launch_bounds__(256) void cau_attn_kernel(CauAttnArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int item = blockIdx.x * 4 + wave;
  if (item >= a.nseq * kCauHeads * a.QT) return;
  const int qt = item % a.QT, h = (item / a.QT) & 3, s = item / (a.QT * kCauHeads), L = a.L;
  const T* qkv = (const T*)a.qkv;
  const size_t base = (size_t)blockIdx.y * a.P + (size_t)s * a.ss;
  const int tq = qt * 16 + col;
  const Frag<T> bq = g == 0 ? load_t<T>(qkv + (base + (size_t)min(tq, L - 1) * a.ts) * 96 + h * 8) : zero_frag<T>();
  float m = -INFINITY, l = 0.f;
  f32x4 o = {0.f, 0.f, 0.f, 0.f};
  for (int kb = 0; kb < L; kb += 32) {
    f32x4 p[2];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int key = kb + 16 * i + col;
      const Frag<T> ak = (g == 0 && key < L) ? load_t<T>(qkv + (base + (size_t)key * a.ts) * 96 + kCauD + h * 8) : zero_frag<T>();
      p[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      mfma_frag(p[i], ak, bq);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (kb + 16 * i + 4 * g + j >= L) p[i][j] = -INFINITY;
        mx = fmaxf(mx, p[i][j]);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx), alpha = expf(m - mn);
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) { p[i][j] = expf(p[i][j] - mn); rs += p[i][j]; }
    rs += __shfl_xor(rs, 16);
    rs += __shfl_xor(rs, 32);
    l = l * alpha + rs;
    o *= alpha;
    m = mn;
    f32x4 vlo = {0.f, 0.f, 0.f, 0.f}, vhi = vlo;
    if (col < 8) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k0 = kb + 4 * g + j, k1 = k0 + 16;
        if (k0 < L) vlo[j] = to_f32<T>(qkv[(base + (size_t)k0 * a.ts) * 96 + 2 * kCauD + h * 8 + col]);
        if (k1 < L) vhi[j] = to_f32<T>(qkv[(base + (size_t)k1 * a.ts) * 96 + 2 * kCauD + h * 8 + col]);
      }
    }
    mfma_frag(o, frag_from_f32<T>(vlo, vhi), frag_from_f32<T>(p[0], p[1]));
  }
  if (g < 2 && tq < L) {
    const float rl = 1.0f / l;
    store4<T>((T*)a.att + (base + (size_t)tq * a.ts) * 32 + h * 8 + 4 * g, o[0] * rl, o[1] * rl, o[2] * rl, o[3] * rl);
  }
}

// ---- bidirectional GRU(32, 64): a block is 16 sequences of one direction (blockIdx.y).  Wave j owns
// hidden channels 16 j .. 16 j + 15: per time step it accumulates its r, z and n gate tiles (input
// part K = 32, recurrent part K = 64) in four accumulators whose lanes hold the same (channel,
// sequence) pair, so the gates combine in registers.  The state is fp32 in LDS, double-buffered (one
// barrier per step); the wave's nine weight fragments stay in registers.  Stores ReLU(h) as T: where
// linear2's MFMA takes it.
struct CauGruArgs {
  const float* src; void* out;            // [tok][32] fp32 -> [tok][128] (T): forward | reverse
  const void* wih; const void* whh; const float* bih; const float* bhh;   // the forward direction's; reverse follows
  int nseq, L, ss, ts, P, total;          // sequences per image; total = B nseq
};
constexpr int kGruLd = 68;                // row stride of the state: 16 sequences do not share a bank

template <typename T> __global__ __launch_bounds__(256) void cau_gru_kernel(CauGruArgs a) {
  __shared__ __align__(16) float hs[2][16][kGruLd];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, col = lane & 15;
  const int d = blockIdx.y, L = a.L;
  const int sq = blockIdx.x * 16 + col;
  const bool sv = sq < a.total;
  const int sqc = min(sq, a.total - 1), b = sqc / a.nseq, s = sqc - b * a.nseq;
  const size_t base = (size_t)b * a.P + (size_t)s * a.ss;
  for (int i = tid; i < 2 * 16 * kGruLd; i += 256) (&hs[0][0][0])[i] = 0.f;
  const T* wih = (const T*)a.wih + (size_t)d * kCauEIhSize;
  const T* whh = (const T*)a.whh + (size_t)d * kCauEHhSize;
  Frag<T> wi[3], wh[3][2];
#pragma unroll
  for (int gt = 0; gt < 3; ++gt) {
    wi[gt] = load_wgt<T>(wih, 4 * gt + wave, 1, 0, lane);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) wh[gt][kc] = load_wgt<T>(whh, 4 * gt + wave, 2, kc, lane);
  }
  const int ch = wave * 16 + 4 * g;
  const float* bih = a.bih + d * 384 + ch;
  const float* bhh = a.bhh + d * 384 + ch;
  const f32x4 br = *(const f32x4*)bih + *(const f32x4*)bhh, bz = *(const f32x4*)(bih + 64) + *(const f32x4*)(bhh + 64);
  const f32x4 bin = *(const f32x4*)(bih + 128), bhn = *(const f32x4*)(bhh + 128);
  __syncthreads();
  const int t0 = d ? L - 1 : 0, dt = d ? -1 : 1;
  const float* xp = a.src + (base + (size_t)t0 * a.ts) * 32 + 8 * g;
  f32x4 xlo = *(const f32x4*)xp, xhi = *(const f32x4*)(xp + 4);
  int p = 0;
  for (int step = 0; step < L; ++step) {
    const int t = t0 + dt * step;
    const size_t tok = base + (size_t)t * a.ts;
    const Frag<T> bx = frag_from_f32<T>(xlo, xhi);
    if (step + 1 < L) {                                 // the next step's input, ahead of this step's math
      const float* xn = a.src + (base + (size_t)(t + dt) * a.ts) * 32 + 8 * g;
      xlo = *(const f32x4*)xn; xhi = *(const f32x4*)(xn + 4);
    }
    f32x4 ar = {0.f, 0.f, 0.f, 0.f}, az = ar, ani = ar, anh = ar;
    mfma_frag(ar, wi[0], bx);
    mfma_frag(az, wi[1], bx);
    mfma_frag(ani, wi[2], bx);
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const float* hr = &hs[p][col][kc * 32 + 8 * g];
      const Frag<T> bh = frag_from_f32<T>(*(const f32x4*)hr, *(const f32x4*)(hr + 4));
      mfma_frag(ar, wh[0][kc], bh);
      mfma_frag(az, wh[1][kc], bh);
      mfma_frag(anh, wh[2][kc], bh);
    }
    const f32x4 hp = *(const f32x4*)&hs[p][col][ch];
    f32x4 hn;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = sigmoid_f(ar[i] + br[i]);
      const float z = sigmoid_f(az[i] + bz[i]);
      const float n = tanhf(ani[i] + bin[i] + r * (anh[i] + bhn[i]));
      hn[i] = (1.0f - z) * n + z * hp[i];
    }
    *(f32x4*)&hs[p ^ 1][col][ch] = hn;
    if (sv) store4<T>((T*)a.out + tok * 128 + d * kCauHid + ch, fmaxf(hn[0], 0.f), fmaxf(hn[1], 0.f), fmaxf(hn[2], 0.f), fmaxf(hn[3], 0.f));
    __syncthreads();
    p ^= 1;
  }
}

template <typename T> hipError_t cau_dt_run(const CauDtArgs& a, hipStream_t s) {
  const int B = a.B, P = a.dim2 * a.dim1, npart = (P + kCauTokTile - 1) / kCauTokTile;
  const size_t tokens = (size_t)B * P;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  char* w = a.ws;
  float* cur = (float*)w; w += up(tokens * 32 * 4);
  float* s1 = (float*)w; w += up(tokens * 32 * 4);
  float* s2 = (float*)w; w += up(tokens * 32 * 4);
  T* qkv = (T*)w; w += up(tokens * 96 * sizeof(T));
  T* att = (T*)w; w += up(tokens * 32 * sizeof(T));
  T* gout = (T*)w; w += up(tokens * 128 * sizeof(T));
  float* part = (float*)w;
  const T* wm = (const T*)a.wmat;
  const float* wv = a.wvec;
  const dim3 tgrid(npart, B), blk(256);
  CauTokArgs t{};
  t.B = B; t.P = P; t.npart = npart; t.cur = cur;
  {
    CauTokArgs x = t;
    x.xin = a.x; x.w = wm + kCauWIn; x.bias = wv + kCauVInB; x.alpha = wv + kCauVInA;
    hipLaunchKernelGGL((cau_tok_kernel<T, TOK_IN>), tgrid, blk, 0, s, x);
  }
  const float* gnw = nullptr;
  const float* gnb = nullptr;
  for (int e = 0; e < 2 * a.n_tstb; ++e) {
    const T* we = wm + kCauWEnc0 + (size_t)e * kCauEncW;
    const float* ve = wv + kCauVEnc0 + (size_t)e * kCauEncV;
    const bool colp = (e & 1) != 0;
    const int nseq = colp ? a.dim1 : a.dim2, L = colp ? a.dim2 : a.dim1, ss = colp ? 1 : a.dim1, ts = colp ? a.dim1 : 1;
    {
      CauTokArgs x = t;
      if (e > 0) { x.gsrc = s2; x.part = part; x.gnw = gnw; x.gnb = gnb; }
      x.w = we + kCauEInProj; x.bias = ve + kCauVInProjB; x.out = qkv;
      hipLaunchKernelGGL((cau_tok_kernel<T, TOK_QKV>), tgrid, blk, 0, s, x);
    }
    {
      CauAttnArgs x{qkv, att, nseq, L, ss, ts, P, (L + 15) / 16};
      const int items = nseq * kCauHeads * x.QT;
      hipLaunchKernelGGL((cau_attn_kernel<T>), dim3((items + 3) / 4, B), blk, 0, s, x);
    }
    {
      CauTokArgs x = t;
      x.xin = att; x.res = cur; x.w = we + kCauEOutProj; x.bias = ve + kCauVOutProjB; x.lnw = ve + kCauVLn1W; x.lnb = ve + kCauVLn1B;
      x.dst = s1;
      hipLaunchKernelGGL((cau_tok_kernel<T, TOK_PROJ>), tgrid, blk, 0, s, x);
    }
    {
      CauGruArgs x{s1, gout, we + kCauEIh, we + kCauEHh, ve + kCauVBih, ve + kCauVBhh, nseq, L, ss, ts, P, B * nseq};
      hipLaunchKernelGGL((cau_gru_kernel<T>), dim3((B * nseq + 15) / 16, 2), blk, 0, s, x);
    }
    {
      CauTokArgs x = t;
      x.xin = gout; x.res = s1; x.w = we + kCauELin2; x.bias = ve + kCauVLin2B; x.lnw = ve + kCauVLn2W; x.lnb = ve + kCauVLn2B;
      x.dst = s2; x.part_out = part;
      hipLaunchKernelGGL((cau_tok_kernel<T, TOK_LIN2>), tgrid, blk, 0, s, x);
    }
    gnw = ve + kCauVGnW;
    gnb = ve + kCauVGnB;
  }
  {
    CauTokArgs x = t;
    x.gsrc = s2; x.part = part; x.gnw = gnw; x.gnb = gnb;
    x.w = wm + kCauWOut; x.bias = wv + kCauVOutB; x.alpha = wv + kCauVOutA; x.out = a.out;
    if (a.prelu_first) hipLaunchKernelGGL((cau_tok_kernel<T, TOK_OUTP>), tgrid, blk, 0, s, x);
    else hipLaunchKernelGGL((cau_tok_kernel<T, TOK_OUT>), tgrid, blk, 0, s, x);
  }
  return hipGetLastError();
}

template <typename T> hipError_t cau_conv_run(const CauConvArgs& a, hipStream_t s) {
  const int rows = a.B * a.F, rpb = 128 / a.Wc;
  const dim3 grid((rows + rpb - 1) / rpb), blk(256);
  // one source's slabs: at most 2 x 16 rows x 10 pixels x 72 channels = 45 KiB in the 16-bit types, 90 KiB in fp32
  const size_t lds = sizeof(T) * (size_t)(a.mode == CAU_DENSE ? 2 : 1) * rpb * ((a.mode == CAU_DOWN ? 2 * a.Wc : a.Wc) + 2) * kCauLdsC;
  if (a.mode == CAU_DENSE) hipLaunchKernelGGL((cau_conv_kernel<T, CAU_DENSE>), grid, blk, lds, s, a);
  else if (a.mode == CAU_DOWN) hipLaunchKernelGGL((cau_conv_kernel<T, CAU_DOWN>), grid, blk, lds, s, a);
  else hipLaunchKernelGGL((cau_conv_kernel<T, CAU_UP>), grid, blk, lds, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_cau_first(int dtype, const CauFirstArgs& a, hipStream_t s) {
  if (a.B < 1 || a.F < 1 || a.N != 128 + 64 * (int64_t)(a.F - 1)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)a.B * a.F * 128 * 16;
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((cau_first_kernel<bf16_t>), grid, blk, 0, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((cau_first_kernel<f16_t>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((cau_first_kernel<float>), grid, blk, 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cau_noise(const CauNoiseArgs& a, hipStream_t s) {
  if (a.B < 1 || a.B > 65535 || a.NL < 1) return hipErrorInvalidValue;
  if (!a.lv.levels && (!a.lv.t_dev || (!a.lv.time_step && !a.lv.table))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(cau_noise_kernel, dim3(a.NL, a.B), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_cau_conv(int dtype, const CauConvArgs& a, hipStream_t s) {
  if (a.B < 1 || a.F < 1 || a.Wc < 8 || a.Wc > 128 || (a.Wc & (a.Wc - 1))) return hipErrorInvalidValue;
  if (a.mode < CAU_DENSE || a.mode > CAU_UP || a.nsrc < 1 || a.nsrc > 3 || a.aff_src >= a.nsrc) return hipErrorInvalidValue;
  if ((a.mode == CAU_DOWN && a.nsrc != 1) || (a.mode == CAU_UP && a.nsrc != 2) || (a.mode == CAU_DENSE && a.dil < 1)) return hipErrorInvalidValue;
  if (a.aff_src >= 0 && (!a.sc || !a.sh)) return hipErrorInvalidValue;
  if (dtype == DT_BF16) return cau_conv_run<bf16_t>(a, s);
  if (dtype == DT_F16) return cau_conv_run<f16_t>(a, s);
  return cau_conv_run<float>(a, s);
}

hipError_t launch_cau_final(int dtype, const CauFinalArgs& a, hipStream_t s) {
  if (a.B < 1 || a.F < 1 || a.N != 128 + 64 * (int64_t)(a.F - 1)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)a.B * a.N;
  const dim3 grid((unsigned)((total + 255) / 256)), blk(256);
  if (dtype == DT_BF16) hipLaunchKernelGGL((cau_final_kernel<bf16_t>), grid, blk, 0, s, a);
  else if (dtype == DT_F16) hipLaunchKernelGGL((cau_final_kernel<f16_t>), grid, blk, 0, s, a);
  else hipLaunchKernelGGL((cau_final_kernel<float>), grid, blk, 0, s, a);
  return hipGetLastError();
}

size_t cau_dt_ws_bytes(int dtype, int64_t B, int64_t P) {
  const size_t es = dtype == DT_F32 ? 4 : 2, tokens = (size_t)B * P;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t npart = (size_t)(P + kCauTokTile - 1) / kCauTokTile;
  return 3 * up(tokens * 32 * 4) + up(tokens * 96 * es) + up(tokens * 32 * es) + up(tokens * 128 * es) + up((size_t)B * npart * 2 * 4);
}

hipError_t launch_cau_dual_transformer(int dtype, const CauDtArgs& a, hipStream_t s) {
  if (a.B < 1 || a.B > 65535 || a.dim1 < 1 || a.dim2 < 1 || a.n_tstb < 1 || !a.ws) return hipErrorInvalidValue;
  if ((int64_t)a.B * a.dim1 * a.dim2 > (int64_t)1 << 24) return hipErrorInvalidValue;   // token offsets * 128 stay far below 2^63, grids below 2^31
  if (dtype == DT_BF16) return cau_dt_run<bf16_t>(a, s);
  if (dtype == DT_F16) return cau_dt_run<f16_t>(a, s);
  return cau_dt_run<float>(a, s);
}

}  // namespace sddm
