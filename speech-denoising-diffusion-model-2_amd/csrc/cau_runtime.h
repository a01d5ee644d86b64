// CAUNet path of the runtime (included by sddm_runtime.cpp after sddm_ctx and SeqNet): configuration
// check, weight packing, workspace and forward of reference model/CAUNet.py:307-374 at the arguments
// of config_caunet.json as a SeqNet; seq_sample runs SDDM.infer (model.py:50-124) over it.
// Kernels: caunet.hip.
//
// Layers (64 channels throughout; F frames of W positions, W = 128 at the top):
//   first_conv      Conv1x1 2 -> 64 over the frames of (cond, y_t)
//   downs i = 0..3  affine (FeatureWiseAffine) -> DenseBlock at W_i = 128 >> i -> Conv (1,3) / stride
//                   (1,2) -> LayerNorm(W_i / 2) -> PReLU; the output is also the skip
//   mid             Dual_Transformer(64, 64, 0, n_TSTB) over [F][8]
//   ups i = 0..3    affine -> DenseBlock at W = 8 << i -> cat(x, skip) -> sub-pixel Conv (1,3) ->
//                   LayerNorm(2 W) -> PReLU
//   final_conv      Conv1x1 64 -> 1, overlap-add
// A DenseBlock is three (2,3) convs with frame dilation 1, 2, 4 over cat(newest .. oldest, input),
// each followed by LayerNorm(W) and PReLU(64); the affine rides on the loads of the block's input.
//
// Launches per reverse step: first_conv 1, noise MLPs 1, 8 layers of 4 convs, the Dual_Transformer
// 2 + 10 n_TSTB, final_conv 1, transition 1 -- 98 at n_TSTB = 6.
#pragma once
#include "caunet.h"
#include "dual_transformer.h"

namespace cau {
constexpr int kLayers = 8;       // 4 encode + 4 decode
inline std::string layer(int l) { return (l < 4 ? "downs." : "ups.") + std::to_string(l & 3) + "."; }
inline int width(int l) { return l < 4 ? 128 >> l : 8 << (l - 4); }   // the DenseBlock's frame length
}  // namespace cau

struct CAUState : SeqNet {
  int n_tstb = 6, affine = 0;
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  WULevel lv{};                                       // the noise level of the current call (begin)
  int F = 0;
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) override;
  int network(sddm_ctx* c, const float* cond, const float* x_t, int per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
};

// refuses everything the kernels are not built for, by the argument's name
static int cau_check_config(const Json& na, CAUState& d) {
  struct { const char* k; int want, dflt; } fixed[] = {{"inner_channel", 64, 64}, {"n_encode_layers", 4, 4}, {"dense_depth", 3, 3},
                                                        {"segment_len", 128, 128}, {"segment_stride", 64, 64}};
  for (const auto& f : fixed)
    if ((int)na.number(f.k, f.dflt) != f.want) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "CAUNet %s %d (%d)", f.k, (int)na.number(f.k, f.dflt), f.want);
  d.n_tstb = (int)na.number("n_TSTB", 6);
  if (d.n_tstb < 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "CAUNet n_TSTB %d (at least 1)", d.n_tstb);
  d.affine = na.number("use_affine_level", 0) != 0;
  return SDDM_OK;
}

// state-dict shapes (CAUNet.py:307-345) without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> cau_param_shapes(const CAUState& d) {
  std::map<std::string, std::vector<int64_t>> s;
  s["first_conv.weight"] = {64, 2, 1, 1}; s["first_conv.bias"] = {64};
  for (int l = 0; l < cau::kLayers; ++l) {
    const std::string p = cau::layer(l);
    const int W = cau::width(l);
    for (int k = 1; k <= 3; ++k) {
      const std::string ks = std::to_string(k);
      s[p + "dense.conv" + ks + ".weight"] = {64, 64 * k, 2, 3}; s[p + "dense.conv" + ks + ".bias"] = {64};
      s[p + "dense.norm" + ks + ".weight"] = {W}; s[p + "dense.norm" + ks + ".bias"] = {W};
      s[p + "dense.prelu" + ks + ".weight"] = {64};
    }
    const int out = d.affine ? 128 : 64;
    s[p + "noise_func.noise_func.0.weight"] = {256, 64}; s[p + "noise_func.noise_func.0.bias"] = {256};
    s[p + "noise_func.noise_func.1.weight"] = {256};
    s[p + "noise_func.noise_func.2.weight"] = {out, 256}; s[p + "noise_func.noise_func.2.bias"] = {out};
    if (l < 4) {
      s[p + "downsample.0.weight"] = {64, 64, 1, 3}; s[p + "downsample.0.bias"] = {64};
      s[p + "downsample.1.weight"] = {W / 2}; s[p + "downsample.1.bias"] = {W / 2};
      s[p + "downsample.2.weight"] = {64};
    } else {
      s[p + "upsample.0.conv.weight"] = {128, 128, 1, 3}; s[p + "upsample.0.conv.bias"] = {128};
      s[p + "upsample.1.weight"] = {2 * W}; s[p + "upsample.1.bias"] = {2 * W};
      s[p + "upsample.2.weight"] = {64};
    }
  }
  dt_param_shapes(s, "mid", kCauC, d.n_tstb, kDtPreluPerChannel);       // CAUNet.py:152-178: one PReLU slope per channel
  s["final_conv.weight"] = {1, 64, 1, 1}; s["final_conv.bias"] = {1};
  return s;
}

// conv weight [co][ci][KH][3] (ci = nsrc * 64) -> fragments of W[co][k], k = ((s KH + kh) 3 + kw) 64 + c
static void cau_add_conv(sddm_ctx* c, WeightPacker& pk, const std::string& name, int co, int nsrc, int KH, const std::vector<float>& w) {
  const int K = nsrc * KH * 3 * 64, ci = nsrc * 64;
  std::vector<float> m((size_t)co * K);
  for (int o = 0; o < co; ++o)
    for (int s = 0; s < nsrc; ++s)
      for (int kh = 0; kh < KH; ++kh)
        for (int kw = 0; kw < 3; ++kw)
          for (int ch = 0; ch < 64; ++ch)
            m[(size_t)o * K + ((s * KH + kh) * 3 + kw) * 64 + ch] = w[(((size_t)o * ci + s * 64 + ch) * KH + kh) * 3 + kw];
  store_frags(pk.raw(name, m.size() * dtype_size(c->dtype)), 0, m.data(), co, K, c->dtype);
}

size_t CAUState::pack(sddm_ctx* c, WeightPacker& pk) {
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  pk.f32("first.w", P("first_conv.weight"));
  pk.f32("first.b", P("first_conv.bias"));
  std::vector<float> w1, b1, a1, w2, b2;               // the eight noise MLPs, layer-major
  auto cat = [](std::vector<float>& d, const std::vector<float>& v) { d.insert(d.end(), v.begin(), v.end()); };
  for (int l = 0; l < cau::kLayers; ++l) {
    const std::string p = cau::layer(l);
    for (int k = 1; k <= 3; ++k) {
      const std::string ks = std::to_string(k);
      cau_add_conv(c, pk, p + "w" + ks, 64, k, 2, P(p + "dense.conv" + ks + ".weight"));
      pk.f32(p + "b" + ks, P(p + "dense.conv" + ks + ".bias"));
      pk.f32(p + "g" + ks, P(p + "dense.norm" + ks + ".weight"));
      pk.f32(p + "e" + ks, P(p + "dense.norm" + ks + ".bias"));
      pk.f32(p + "a" + ks, P(p + "dense.prelu" + ks + ".weight"));
    }
    const std::string r = p + (l < 4 ? "downsample." : "upsample.");
    if (l < 4) cau_add_conv(c, pk, p + "ws", 64, 1, 1, P(r + "0.weight"));
    else cau_add_conv(c, pk, p + "ws", 128, 2, 1, P(r + "0.conv.weight"));
    pk.f32(p + "bs", P(r + (l < 4 ? "0.bias" : "0.conv.bias")));
    pk.f32(p + "gs", P(r + "1.weight"));
    pk.f32(p + "es", P(r + "1.bias"));
    pk.f32(p + "as", P(r + "2.weight"));
    cat(w1, P(p + "noise_func.noise_func.0.weight")); cat(b1, P(p + "noise_func.noise_func.0.bias"));
    cat(a1, P(p + "noise_func.noise_func.1.weight"));
    cat(w2, P(p + "noise_func.noise_func.2.weight")); cat(b2, P(p + "noise_func.noise_func.2.bias"));
  }
  pk.f32("mlp.w1", w1); pk.f32("mlp.b1", b1); pk.f32("mlp.a1", a1); pk.f32("mlp.w2", w2); pk.f32("mlp.b2", b2);
  dt_pack(c, pk, "mid", kCauLayout, n_tstb, kDtPreluPerChannel);           // at the offsets of caunet.h
  pk.f32("final.w", P("final_conv.weight"));
  pk.f32("final.b", P("final_conv.bias"));
  return 0;                                            // no table of its own: the level is one scalar per t
}

// activation buffers for (B, N): [B][F][W][64] in the compute dtype
int CAUState::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  if (B < 1 || B > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)B);
  if (N < 128 || (N - 128) % 64) FAIL(SDDM_ERR_SHAPE, "%lld samples: CAUNet frames 128 samples every 64, (num_samples - 128) %% 64 == 0", (long long)N);
  const int64_t frames = (N - 128) / 64 + 1;
  if (B * frames > (int64_t)1 << 21) FAIL(SDDM_ERR_SHAPE, "%lld x %lld frames: CAUNet row indices are 32-bit", (long long)B, (long long)frames);
  if (this->B == B && this->N == N) return SDDM_OK;
  const size_t es = dtype_size(c->dtype);
  act.reset();
  aoff.clear();
  auto buf = [&](const std::string& n, int W) { aoff[n] = act.reserve(es * (size_t)B * frames * W * 64); };
  buf("first", 128);
  for (int k = 1; k <= 3; ++k) buf("d" + std::to_string(k), 128);       // the DenseBlocks' outputs, reused by every layer
  for (int l = 0; l < cau::kLayers; ++l) buf("o" + std::to_string(l), l < 4 ? cau::width(l) / 2 : cau::width(l) * 2);
  buf("mid", 8);
  aoff["dtws"] = act.reserve(cau_dt_ws_bytes(c->dtype, B, frames * 8));
  aoff["sc"] = act.reserve(sizeof(float) * (size_t)B * cau::kLayers * 64);
  aoff["sh"] = act.reserve(sizeof(float) * (size_t)B * cau::kLayers * 64);
  aoff["eps"] = act.reserve(sizeof(float) * (size_t)B * N);
  SDDM_HIP_CHECK(act.commit());
  this->B = (int)B;
  this->N = N;
  F = (int)frames;
  return SDDM_OK;
}

int CAUState::begin(sddm_ctx* c, const float*, const float* noise_level, hipStream_t) {
  lv = wu_begin_level(c, noise_level, off_sp);
  return SDDM_OK;
}

// one forward (CAUNet.py:347-374): cond, x_t [B][N] fp32 -> eps [B][N] fp32 (aoff "eps")
int CAUState::network(sddm_ctx* c, const float* cond, const float* x_t, int, int* t_dev, hipStream_t s) {
  const Arena& W = c->warena;
  const int dt = c->dtype;
  auto buf = [&](const std::string& n) -> char* { return act.base + aoff.at(n); };
  auto wf = [&](const std::string& n) -> const float* { return W.at<float>(woff.at(n)); };
  auto wt = [&](const std::string& n) -> const void* { return W.base + woff.at(n); };
  float* sc = act.at<float>(aoff.at("sc"));
  float* sh = act.at<float>(aoff.at("sh"));
  CauFirstArgs fa{cond, x_t, wf("first.w"), wf("first.b"), buf("first"), B, F, N, t_dev};
  TRY_LAUNCH("cau_first", launch_cau_first(dt, fa, s));
  CauNoiseArgs na{lv, wf("mlp.w1"), wf("mlp.b1"), wf("mlp.a1"), wf("mlp.w2"), wf("mlp.b2"), affine, B, cau::kLayers, sc, sh};
  TRY_LAUNCH("cau_noise", launch_cau_noise(na, s));
  const char* x = buf("first");
  for (int l = 0; l < cau::kLayers; ++l) {
    const std::string p = cau::layer(l);
    const int Wd = cau::width(l);
    if (l == 4) {                                      // mid between the encoder and the decoder
      CauDtArgs da{x, buf("mid"), wt("mid.wmat"), wf("mid.wvec"), buf("dtws"), B, F, 8, n_tstb};
      TRY_LAUNCH("cau_dual_transformer", launch_cau_dual_transformer(dt, da, s));
      x = buf("mid");
    }
    for (int k = 1; k <= 3; ++k) {                     // DenseBlock: sources newest first, the affined input last
      const std::string ks = std::to_string(k);
      CauConvArgs a{};
      a.mode = CAU_DENSE; a.nsrc = k; a.dil = 1 << (k - 1); a.aff_src = k - 1;
      for (int j = 0; j < k - 1; ++j) a.src[j] = buf("d" + std::to_string(k - 1 - j));
      a.src[k - 1] = x;
      a.sc = sc + l * 64; a.sh = sh + l * 64; a.aff_ld = cau::kLayers * 64;
      a.w = wt(p + "w" + ks); a.bias = wf(p + "b" + ks); a.lnw = wf(p + "g" + ks); a.lnb = wf(p + "e" + ks); a.alpha = wf(p + "a" + ks);
      a.out = buf("d" + ks); a.B = B; a.F = F; a.Wc = Wd;
      TRY_LAUNCH("cau_conv dense", launch_cau_conv(dt, a, s));
    }
    CauConvArgs a{};
    a.aff_src = -1; a.dil = 1;
    a.w = wt(p + "ws"); a.bias = wf(p + "bs"); a.lnw = wf(p + "gs"); a.lnb = wf(p + "es"); a.alpha = wf(p + "as");
    a.out = buf("o" + std::to_string(l)); a.B = B; a.F = F;
    if (l < 4) {
      a.mode = CAU_DOWN; a.nsrc = 1; a.src[0] = buf("d3"); a.Wc = Wd / 2;
    } else {                                           // cat([x, skip]) with the skip of encode layer 7 - l
      a.mode = CAU_UP; a.nsrc = 2; a.src[0] = buf("d3"); a.src[1] = buf("o" + std::to_string(7 - l)); a.Wc = Wd;
    }
    TRY_LAUNCH("cau_conv resample", launch_cau_conv(dt, a, s));
    x = buf("o" + std::to_string(l));
  }
  CauFinalArgs ea{x, wf("final.w"), wf("final.b"), act.at<float>(aoff.at("eps")), B, F, N};
  TRY_LAUNCH("cau_final", launch_cau_final(dt, ea, s));
  return SDDM_OK;
}
