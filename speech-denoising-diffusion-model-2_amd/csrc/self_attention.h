// Spatial self-attention of UNetModified (reference model/UNetModified.py:140-169): GroupNorm, 1x1 qkv
// conv without bias, softmax(Q K^T / sqrt(C)) V over all H*W positions with one head, 1x1 out conv,
// residual.  Kernels in self_attention.hip; activations are [B][P][C] (P = H*W) in the compute dtype.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sddm {

constexpr int kAttnMaxC = 256;        // channels: multiples of 32 up to this (the accumulators of one wave)
constexpr int kAttnQueryTile = 64;    // queries per workgroup of attn_core: 4 waves x 16
constexpr int kAttnKeyTile = 32;      // keys staged per iteration

// queries per workgroup and per GroupNorm statistics tile of the output: the largest divisor of P up
// to kAttnQueryTile, so that every tile holds the same count (the consumers' Chan combination)
inline int attn_query_tile(int P) {
  int q = P < kAttnQueryTile ? P : kAttnQueryTile;
  while (P % q) --q;
  return q;
}

struct AttnArgs {
  const void* x;              // [B][P][C] (T): the block's input, also the residual
  const float* gst; int gtiles, gntile;          // the producer's per-tile statistics of x
  const float* gamma; const float* beta; int groups; float eps;
  const void* wqkv_f;         // qkv weight [3C][C] as MFMA fragments [3C/16][C/32][64 lanes][8] (T)
  void* qkv;                  // scratch [B][P][3C] (T): q, k, v = channels [0,C), [C,2C), [2C,3C)
  const void* wout_f;         // out weight [C][C] as MFMA fragments (T)
  const float* bout;          // [C]
  void* out;                  // [B][P][C] (T)
  float* stats;               // [B][P / QT][C][2] (sum, M2 about the tile mean) of the fp32 results, or null
  int P, C, QT;               // positions, channels, queries per workgroup (attn_query_tile(P))
  float scale_log2;           // log2(e) / sqrt(C): the softmax runs in base 2
};
// GroupNorm (no SiLU) + [P x C] . [C x 3C] -> qkv
hipError_t launch_attn_qkv(int dtype, const AttnArgs& a, int B, hipStream_t s);
// softmax(Q K^T / sqrt(C)) V with a running maximum, then the out conv, bias, residual and statistics
hipError_t launch_attn_core(int dtype, const AttnArgs& a, int B, hipStream_t s);
size_t attn_qkv_lds_bytes(int dtype, int C);
size_t attn_core_lds_bytes(int dtype, int C);
// per-tile statistics of a tensor [B][P][C] (T) nobody produced with them (sddm_self_attention's input)
hipError_t launch_attn_input_stats(int dtype, const void* x, float* stats, int B, int P, int C, int n_tile, hipStream_t s);

}  // namespace sddm
