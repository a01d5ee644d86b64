// TSTNN path of the runtime (included by sddm_runtime.cpp after sddm_ctx and SeqNet): configuration
// check, weight packing, workspace and forward of reference model/tstnn.py:216-299 at the arguments
// of config_tstnn.json as a SeqNet; seq_sample runs SDDM.infer (model.py:50-124) over it.
// Kernels: tstnn.hip, and caunet.hip's Dual_Transformer.
//
// Layers (64 channels throughout; Fr frames of 512 samples every 256):
//   inp_conv         Conv1x1 2 -> 64 over the frames of (cond, y_t) -> LayerNorm(512) -> PReLU
//   enc_dense1       DenseBlock(512, depth 4)
//   enc_conv1        Conv (1,3) / stride (1,2) -> LayerNorm(256) -> PReLU = x1
//   dual_transformer Dual_Transformer(64, 64, num_layers 4) over [Fr][256]: single-slope PReLUs, the
//                    output stage is PReLU then conv
//   output1, output2, maskconv   x1 * ReLU(maskconv(tanh(output1) * sigmoid(output2)))
//   dec_dense1       DenseBlock(256, depth 4)
//   dec_conv1        sub-pixel Conv (1,3) 64 -> 128 -> LayerNorm(512) -> PReLU
//   out_conv         Conv1x1 64 -> 1, overlap-add
// A DenseBlock is four (2,3) convs with frame dilation 1, 2, 4, 8 over cat(newest .. oldest, input),
// each followed by LayerNorm(W) and PReLU(64).  The noise level enters nowhere (tstnn.py:266-299).
//
// Launches per reverse step: first 1, dense convs 4 + 4, down 1, up 1, the Dual_Transformer
// 2 + 10 num_layers = 42, gate 1, final 1, transition 1 -- 56.
#pragma once
#include "tstnn.h"

struct TSTNNState : SeqNet {
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  int layers = kTstnnLayers;                          // the Dual_Transformer's num_layers
  int F = 0;                                          // frames
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx*, const float*, const float*, hipStream_t) override { return SDDM_OK; }   // no level, nothing step-invariant
  int network(sddm_ctx* c, const float* cond, const float* x_t, int per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
};

// refuses everything the kernels are not built for, by the argument's name
// (num_layers is not an argument of the reference's TSTNN, which builds its block with 4: a stand-alone
// Dual_Transformer(64, 64, 0, num_layers) configures its context with it)
static int tstnn_check_config(const Json& na, TSTNNState& d) {
  struct { const char* k; int want; } fixed[] = {{"F", kTstnnF}, {"stride", kTstnnStride}, {"n_channels", kCauC}};
  for (const auto& f : fixed)
    if ((int)na.number(f.k, f.want) != f.want) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "TSTNN %s %d (%d)", f.k, (int)na.number(f.k, f.want), f.want);
  d.layers = (int)na.number("num_layers", kTstnnLayers);
  if (d.layers < 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "TSTNN num_layers %d (at least 1)", d.layers);
  return SDDM_OK;
}

// state-dict shapes (tstnn.py:216-264) without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> tstnn_param_shapes(const TSTNNState& d) {
  std::map<std::string, std::vector<int64_t>> s;
  auto norm_act = [&](const std::string& norm, const std::string& prelu, int W) {
    s[norm + ".weight"] = {W}; s[norm + ".bias"] = {W}; s[prelu + ".weight"] = {64};
  };
  s["inp_conv.weight"] = {64, 2, 1, 1}; s["inp_conv.bias"] = {64};
  norm_act("inp_norm", "inp_prelu", kTstnnF);
  for (const char* d : {"enc_dense1.", "dec_dense1."}) {
    const int W = d[0] == 'e' ? kTstnnF : kTstnnF / 2;
    for (int k = 1; k <= 4; ++k) {
      const std::string p = d, ks = std::to_string(k);
      s[p + "conv" + ks + ".weight"] = {64, 64 * k, 2, 3}; s[p + "conv" + ks + ".bias"] = {64};
      norm_act(p + "norm" + ks, p + "prelu" + ks, W);
    }
  }
  s["enc_conv1.weight"] = {64, 64, 1, 3}; s["enc_conv1.bias"] = {64};
  norm_act("enc_norm1", "enc_prelu1", kTstnnF / 2);
  dt_param_shapes(s, "dual_transformer", kCauC, d.layers, kDtPreluSharedFirst);   // tstnn.py:122-141
  for (const char* n : {"output1.0", "output2.0", "maskconv"}) {
    s[std::string(n) + ".weight"] = {64, 64, 1, 1}; s[std::string(n) + ".bias"] = {64};
  }
  s["dec_conv1.conv.weight"] = {128, 64, 1, 3}; s["dec_conv1.conv.bias"] = {128};
  norm_act("dec_norm1", "dec_prelu1", kTstnnF);
  s["out_conv.weight"] = {1, 64, 1, 1}; s["out_conv.bias"] = {1};
  return s;
}

size_t TSTNNState::pack(sddm_ctx* c, WeightPacker& pk) {
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  auto norm_act = [&](const std::string& n, const std::string& norm, const std::string& prelu) {
    pk.f32(n + ".g", P(norm + ".weight")); pk.f32(n + ".e", P(norm + ".bias")); pk.f32(n + ".a", P(prelu + ".weight"));
  };
  pk.f32("inp.w", P("inp_conv.weight"));               // inp_conv.bias is constant over the frame: LayerNorm removes it
  norm_act("inp", "inp_norm", "inp_prelu");
  for (const std::string d : {"enc_dense1.", "dec_dense1."})
    for (int k = 1; k <= 4; ++k) {
      const std::string ks = std::to_string(k);
      cau_add_conv(c, pk, d + ks + ".w", 64, k, 2, P(d + "conv" + ks + ".weight"));
      pk.f32(d + ks + ".b", P(d + "conv" + ks + ".bias"));
      norm_act(d + ks, d + "norm" + ks, d + "prelu" + ks);
    }
  cau_add_conv(c, pk, "enc.w", 64, 1, 1, P("enc_conv1.weight"));
  pk.f32("enc.b", P("enc_conv1.bias"));
  norm_act("enc", "enc_norm1", "enc_prelu1");
  dt_pack(c, pk, "dual_transformer", kCauLayout, layers, kDtPreluSharedFirst);   // at the offsets of caunet.h
  for (const char* n : {"output1.0", "output2.0", "maskconv"}) {
    const std::vector<float>& w = P(std::string(n) + ".weight");
    std::vector<float> m(w);
    if (std::string(n) == "maskconv")                  // the gate arrives in the accumulator's channel order (tstnn.h)
      for (int o = 0; o < 64; ++o)
        for (int kk = 0; kk < 64; ++kk) m[(size_t)o * 64 + kk] = w[(size_t)o * 64 + tstnn_gate_k(kk)];
    store_frags(pk.raw(std::string(n) + ".w", m.size() * dtype_size(c->dtype)), 0, m.data(), 64, 64, c->dtype);
    pk.f32(std::string(n) + ".b", P(std::string(n) + ".bias"));
  }
  cau_add_conv(c, pk, "dec.w", 128, 1, 1, P("dec_conv1.conv.weight"));
  pk.f32("dec.b", P("dec_conv1.conv.bias"));
  norm_act("dec", "dec_norm1", "dec_prelu1");
  pk.f32("out.w", P("out_conv.weight"));
  pk.f32("out.b", P("out_conv.bias"));
  return 0;                                            // no per-t table
}

// activation buffers for (B, N): [B][Fr][W][64] in the compute dtype
int TSTNNState::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  if (B < 1 || B > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)B);
  if (N < kTstnnF || (N - kTstnnF) % kTstnnStride)
    FAIL(SDDM_ERR_SHAPE, "%lld samples: TSTNN frames 512 samples every 256, (num_samples - 512) %% 256 == 0", (long long)N);
  const int64_t frames = (N - kTstnnF) / kTstnnStride + 1;
  if (B * frames > (int64_t)1 << 21 || B * frames * 256 > (int64_t)1 << 24)
    FAIL(SDDM_ERR_SHAPE, "%lld x %lld frames: TSTNN row indices are 32-bit and the Dual_Transformer kernels index 2^24 tokens", (long long)B, (long long)frames);
  if (this->B == B && this->N == N) return SDDM_OK;
  const size_t es = dtype_size(c->dtype);
  act.reset();
  aoff.clear();
  auto buf = [&](const std::string& n, int W) { aoff[n] = act.reserve(es * (size_t)B * frames * W * 64); };
  buf("inp", kTstnnF);                                   // also dec_conv1's output
  for (int k = 1; k <= 4; ++k) buf("d" + std::to_string(k), kTstnnF);     // the DenseBlocks' outputs, reused by both
  buf("x1", 256);
  buf("dt", 256);
  buf("gate", 256);
  aoff["dtws"] = act.reserve(cau_dt_ws_bytes(c->dtype, B, frames * 256));
  aoff["eps"] = act.reserve(sizeof(float) * (size_t)B * N);
  SDDM_HIP_CHECK(act.commit());
  this->B = (int)B;
  this->N = N;
  F = (int)frames;
  return SDDM_OK;
}

// one forward (tstnn.py:266-299): cond, x_t [B][N] fp32 -> eps [B][N] fp32 (aoff "eps")
int TSTNNState::network(sddm_ctx* c, const float* cond, const float* x_t, int, int* t_dev, hipStream_t s) {
  const Arena& W = c->warena;
  const int dt = c->dtype;
  auto buf = [&](const std::string& n) -> char* { return act.base + aoff.at(n); };
  auto wf = [&](const std::string& n) -> const float* { return W.at<float>(woff.at(n)); };
  auto wt = [&](const std::string& n) -> const void* { return W.base + woff.at(n); };
  auto conv = [&](const char* what, int mode, const std::string& p, const void* src, int Wc, void* out) -> int {
    TstnnConvArgs a{};
    a.mode = mode; a.nsrc = 1; a.src[0] = src; a.dil = 1;
    a.w = wt(p + ".w"); a.bias = wf(p + ".b"); a.lnw = wf(p + ".g"); a.lnb = wf(p + ".e"); a.alpha = wf(p + ".a");
    a.out = out; a.B = B; a.F = F; a.Wc = Wc;
    TRY_LAUNCH(what, launch_tstnn_conv(dt, a, s));
    return SDDM_OK;
  };
  auto dense = [&](const std::string& d, const void* x, int Wc) -> int {   // sources newest first, the input last
    for (int k = 1; k <= 4; ++k) {
      const std::string p = d + std::to_string(k);
      TstnnConvArgs a{};
      a.mode = CAU_DENSE; a.nsrc = k; a.dil = 1 << (k - 1);
      for (int j = 0; j < k - 1; ++j) a.src[j] = buf("d" + std::to_string(k - 1 - j));
      a.src[k - 1] = x;
      a.w = wt(p + ".w"); a.bias = wf(p + ".b"); a.lnw = wf(p + ".g"); a.lnb = wf(p + ".e"); a.alpha = wf(p + ".a");
      a.out = buf("d" + std::to_string(k)); a.B = B; a.F = F; a.Wc = Wc;
      TRY_LAUNCH("tstnn_conv dense", launch_tstnn_conv(dt, a, s));
    }
    return SDDM_OK;
  };
  TstnnFirstArgs fa{cond, x_t, wf("inp.w"), wf("inp.g"), wf("inp.e"), wf("inp.a"), buf("inp"), B, F, N, t_dev};
  TRY_LAUNCH("tstnn_first", launch_tstnn_first(dt, fa, s));
  TRY(dense("enc_dense1.", buf("inp"), kTstnnF));
  TRY(conv("tstnn_conv down", CAU_DOWN, "enc", buf("d4"), 256, buf("x1")));
  CauDtArgs da{buf("x1"), buf("dt"), wt("dual_transformer.wmat"), wf("dual_transformer.wvec"), buf("dtws"), B, F, 256, layers, 1};
  TRY_LAUNCH("cau_dual_transformer", launch_cau_dual_transformer(dt, da, s));
  TstnnGateArgs ga{buf("dt"), buf("x1"), wt("output1.0.w"), wt("output2.0.w"), wt("maskconv.w"), wf("output1.0.b"), wf("output2.0.b"),
                 wf("maskconv.b"), buf("gate"), (int64_t)B * F * 256};
  TRY_LAUNCH("tstnn_gate", launch_tstnn_gate(dt, ga, s));
  TRY(dense("dec_dense1.", buf("gate"), 256));
  TRY(conv("tstnn_conv up", CAU_UP, "dec", buf("d4"), 256, buf("inp")));
  TstnnFinalArgs ea{buf("inp"), wf("out.w"), wf("out.b"), act.at<float>(aoff.at("eps")), B, F, N};
  TRY_LAUNCH("tstnn_final", launch_tstnn_final(dt, ea, s));
  return SDDM_OK;
}
