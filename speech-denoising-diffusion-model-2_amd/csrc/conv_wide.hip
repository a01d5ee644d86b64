// K-chunked 3x3 convolution for the layers no other kernel holds (gfx950, wave64).
//
// conv_deep keeps a layer's whole K (every input channel's halo) in LDS; at about 256 input channels
// plus a res_conv that no longer fits in float32.  This kernel stages the halo of 32 input channels at a
// time instead, applies GroupNorm + SiLU as it stages them and accumulates in registers, so its LDS does
// not grow with the channels.  It takes everything a ConvArgs can ask for: stride 1, stride 2
// (Downsample), the nearest-2x upsampled source (Upsample), the virtual two-source concat, the noise
// embedding, the three residual modes, and it leaves the same per-tile GroupNorm statistics.
//
// One block (4 waves) computes a tile of at most 64 output pixels (TR x TW) for 32 output channels; wave
// w owns pixels 16 w .. 16 w + 15 and two 16-channel accumulator fragments.  Weights come from the
// MFMA-fragment images (ConvArgs::wgt_f / res_wgt_f) straight from global memory.  float32 products are
// MFMA 16x16x4 f32, i.e. true fp32.  This is a correctness path: nothing here is tuned.
#include "sddm_common.h"
#include "kernels.h"
#include "conv_common.h"

namespace sddm {

struct WideGeo { int HR, HC, HP, rows; };
__host__ __device__ inline WideGeo wide_geo(bool s2, int TR, int TW) {
  WideGeo g;
  g.HR = s2 ? 2 * TR + 1 : TR + 2;
  g.HC = s2 ? 2 * TW + 1 : TW + 2;
  g.HP = g.HR * g.HC;
  g.rows = g.HP > 64 ? g.HP : 64;     // the res_conv input reuses the halo rows: one per output pixel
  return g;
}
static constexpr int kWideRedLd = 36;  // floats per pixel of the epilogue tile (32 channels + pad)

template <typename T, bool S2>
__global__ __launch_bounds__(256) void conv_wide_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int ES = (int)sizeof(T);
  constexpr int LDH = 32 * ES + 16;    // bytes per halo position: 32 channels + pad
  const int tile = blockIdx.x, zb = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, wv = tid >> 6;
  const int Cin = a.CA + a.CB, nck = Cin / 32;
  const int RC = a.res_mode == 2 ? a.RCA + a.RCB : 0, rck = RC / 32;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const int y0 = ty * a.TR, x0 = tx * a.TW, npv = a.TR * a.TW;
  const WideGeo geo = wide_geo(S2, a.TR, a.TW);
  const int HC = geo.HC, HP = geo.HP;
  float* sc = (float*)smem;
  float* sh = sc + Cin;
  char* halo = smem + (size_t)Cin * 8;
  float* red = (float*)(halo + (size_t)geo.rows * LDH);
  const bool gn = a.gamma != nullptr;
  if (gn) {
    const GNFuse gf{a.gstA, a.gtilesA, a.gntileA, a.gstB, a.gtilesB, a.gntileB, a.gamma, a.beta, a.groups, a.eps};
    gn_fused_prologue(gf, b, a.CA, a.CB, sc, sh);
  }
  const size_t img_in = (size_t)a.Hi * a.Wi, img_out = (size_t)a.Ho * a.Wo;
  const T* srcA = (const T*)a.srcA + (size_t)b * img_in * a.CA;
  const T* srcB = a.CB ? (const T*)a.srcB + (size_t)b * img_in * a.CB : nullptr;

  // this lane's output pixel and the top-left corner of its 3x3 window in the halo
  const int p = wv * 16 + (lane & 15);
  const int pv = p < npv ? p : 0;
  const int py = pv / a.TW, px = pv - py * a.TW;
  const int off = S2 ? (2 * py) * HC + 2 * px : py * HC + px;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  const T* wbase = (const T*)a.wgt_f + (size_t)lane * 8;

  for (int ck = 0; ck < nck; ++ck) {
    __syncthreads();                   // scale / shift written; the previous chunk's reads are done
    for (int i = tid; i < HP * 8; i += 256) {
      const int pos = i >> 3, c4 = (i & 7) * 4;
      const int hy = pos / HC, hx = pos - hy * HC;
      int iy, ix;
      bool ok;
      if (S2) {
        iy = 2 * y0 - 1 + hy; ix = 2 * x0 - 1 + hx;
        ok = iy >= 0 && iy < a.Hi && ix >= 0 && ix < a.Wi;
      } else {
        iy = y0 - 1 + hy; ix = x0 - 1 + hx;
        ok = iy >= 0 && iy < a.Ho && ix >= 0 && ix < a.Wo;
        if (a.upsample) { iy >>= 1; ix >>= 1; }
      }
      f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
      if (ok) {                        // zero padding stays zero: GroupNorm + SiLU only inside the image
        const int cg = ck * 32 + c4;
        const size_t pix = (size_t)iy * a.Wi + ix;
        v = cg < a.CA ? load4<T>(srcA + pix * a.CA + cg) : load4<T>(srcB + pix * a.CB + (cg - a.CA));
        if (gn) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = silu(v[j] * sc[cg + j] + sh[cg + j]);
        }
      }
      store4<T>((T*)(halo + (size_t)pos * LDH) + c4, v[0], v[1], v[2], v[3]);
    }
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      const Frag<T> bf = load_frag<T>(halo + (size_t)(off + dy * HC + dx) * LDH + g * 8 * ES);
#pragma unroll
      for (int fc = 0; fc < 2; ++fc) {
        const Frag<T> wa = load_frag<T>((const char*)(wbase + ((size_t)(zb * 2 + fc) * (nck * 9) + ck * 9 + tap) * 512));
        mfma_frag(acc[fc], wa, bf);
      }
    }
  }
  // the res_conv (1x1 over the raw concat) as further K chunks at the output pixels
  if (rck) {
    const T* rawA = (const T*)a.rawA + (size_t)b * img_out * a.RCA;
    const T* rawB = a.RCB ? (const T*)a.rawB + (size_t)b * img_out * a.RCB : nullptr;
    const T* rbase = (const T*)a.res_wgt_f + (size_t)lane * 8;
    for (int rk = 0; rk < rck; ++rk) {
      __syncthreads();
      for (int i = tid; i < 64 * 8; i += 256) {
        const int q = i >> 3, c4 = (i & 7) * 4;
        f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q < npv) {
          const int qy = q / a.TW, qx = q - qy * a.TW;
          const size_t pix = (size_t)(y0 + qy) * a.Wo + (x0 + qx);
          const int cg = rk * 32 + c4;
          v = cg < a.RCA ? load4<T>(rawA + pix * a.RCA + cg) : load4<T>(rawB + pix * a.RCB + (cg - a.RCA));
        }
        store4<T>((T*)(halo + (size_t)q * LDH) + c4, v[0], v[1], v[2], v[3]);
      }
      __syncthreads();
      const Frag<T> bf = load_frag<T>(halo + (size_t)p * LDH + g * 8 * ES);
#pragma unroll
      for (int fc = 0; fc < 2; ++fc) {
        const Frag<T> wa = load_frag<T>((const char*)(rbase + ((size_t)(zb * 2 + fc) * rck + rk) * 512));
        mfma_frag(acc[fc], wa, bf);
      }
    }
  }

  // epilogue: bias, noise embedding, identity residual; the fp32 values go to the statistics tile
  const int t_now = a.temb_per_b ? b : (a.t_dev ? *a.t_dev : 0);
  const float* trow = a.temb ? a.temb + (size_t)t_now * a.temb_ld : nullptr;
  const size_t opix = (size_t)(y0 + py) * a.Wo + (x0 + px);
#pragma unroll
  for (int fc = 0; fc < 2; ++fc) {
    const int cl = fc * 16 + 4 * g, co = zb * 32 + cl;
    f32x4 v = acc[fc];
    if (a.res_mode == 1 && p < npv) v += load4<T>((const T*)a.res_src + ((size_t)b * img_out + opix) * a.Cout + co);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += a.bias[co + i] + (trow ? trow[co + i] : 0.f);
    *(f32x4*)(red + p * kWideRedLd + cl) = v;
    if (p < npv) store4<T>((T*)a.out + ((size_t)b * img_out + opix) * a.Cout + co, v[0], v[1], v[2], v[3]);
  }
  __syncthreads();
  if (a.stats)
    tile_channel_stats(red, kWideRedLd, npv, 32, a.stats + (((size_t)b * a.n_tiles + tile) * a.Cout + zb * 32) * 2, 2);
}

size_t conv_wide_lds_bytes(int dtype, bool s2, const ConvArgs& a) {
  const size_t es = dtype == DT_F32 ? 4 : 2;
  const WideGeo geo = wide_geo(s2, a.TR, a.TW);
  return (size_t)(a.CA + a.CB) * 8 + (size_t)geo.rows * (32 * es + 16) + (size_t)64 * kWideRedLd * 4;
}

template <typename T>
static hipError_t wide_go(bool s2, const ConvArgs& a, int B, hipStream_t s, size_t lds) {
  const dim3 grid(a.n_tiles, a.Cout / 32, B), blk(256);
  if (s2) hipLaunchKernelGGL((conv_wide_kernel<T, true>), grid, blk, lds, s, a);
  else hipLaunchKernelGGL((conv_wide_kernel<T, false>), grid, blk, lds, s, a);
  return hipGetLastError();
}

hipError_t launch_conv_wide(int dtype, bool s2, const ConvArgs& a, int B, hipStream_t s) {
  const int RC = a.res_mode == 2 ? a.RCA + a.RCB : 0;
  if (B < 1 || B > 65535 || a.TR < 1 || a.TW < 1 || a.TR * a.TW > 64 || a.Ho % a.TR || a.Wo % a.TW ||
      a.tiles_x != a.Wo / a.TW || a.n_tiles != a.tiles_x * (a.Ho / a.TR) || a.Cout % 32 || a.Cout / 32 > 65535 ||
      a.CA % 32 || a.CB % 32 || a.CA < 32 || RC % 32 || (RC && a.RCA % 32) || (s2 && a.upsample))
    return hipErrorInvalidValue;
  if (s2 ? (a.Hi != 2 * a.Ho || a.Wi != 2 * a.Wo) : a.upsample ? (2 * a.Hi != a.Ho || 2 * a.Wi != a.Wo) : (a.Hi != a.Ho || a.Wi != a.Wo))
    return hipErrorInvalidValue;
  if (a.gamma && (a.groups < 1 || a.groups > 256)) return hipErrorInvalidValue;
  const size_t lds = conv_wide_lds_bytes(dtype, s2, a);
  if (lds > (size_t)kLdsBytes) return hipErrorInvalidValue;
  if (dtype == DT_F32) return wide_go<float>(s2, a, B, s, lds);
  if (dtype == DT_BF16) return wide_go<bf16_t>(s2, a, B, s, lds);
  return wide_go<f16_t>(s2, a, B, s, lds);
}

}  // namespace sddm
