// Waveunet3 path of the runtime (included by sddm_runtime.cpp after sddm_ctx and SeqNet):
// configuration check, weight packing, workspace and forward of reference model/waveunet3.py:314-416
// at the arguments of config_waveunet3.json as a SeqNet; seq_sample runs SDDM.infer
// (model.py:50-124) over it.  Kernels: waveunet.hip.
//
// Layers (C = 32 / 64 / 96 / 128, L_i = N / 2^i; every ResnetBlock is block1 -> + noise constant ->
// block2 -> + res, a Block is GroupNorm -> SiLU -> Conv5):
//   down i = 0..2   pre_shortcut  ResnetBlock(in -> C_i) at L_i (in = 2 raw channels for i = 0)
//                   post_shortcut ResnetBlock(C_i -> C_i+1) at L_i
//                   downconv      Conv 4 / stride 2 -> GroupNorm(groups of 8) -> ReLU, to L_i+1
//   bottleneck      2 x ResnetBlock(128 -> 128) at L_3
//   up i = 3..1     upconv        ConvTranspose 4 / stride 2 -> GroupNorm(groups of 8) -> ReLU, to L_i-1
//                   pre_shortcut  ResnetBlock(C_i -> C_i-1), + shortcut of down i-1
//                   post_shortcut ResnetBlock(C_i-1 -> C_i-1)
//   output_conv     Conv 1x1 32 -> 1, clamp
// The first DownsamplingBlock is built with norm_groups = num_inputs (waveunet3.py:339-342), so all
// four GroupNorms of its two ResnetBlocks have 2 groups; every other Block has 32.
//
// Statistics.  Every producer whose output a GroupNorm reads leaves (sum, sum of squares) partials
// in the one statistics buffer; the consumer's finalize launch (it knows the group count and the
// affine) turns them into the per-(row, channel) scale / shift the consumer's staging applies.
// The ConvLayers normalise their own output: conv (partials of the raw output) -> finalize ->
// wu_act (ReLU(GN(raw)) and the partials of the result, which the next block's GroupNorm reads).
//
// Launches per reverse step: input statistics 1 (it writes the stem's scale / shift itself), stem 1,
// 27 MFMA Block convs (13 block1 + 14 block2) with one finalize each, 6 ConvLayers of three (conv,
// finalize, wu_act), head 1, transition 1 -- 1 + 1 + 27 + 27 + 18 + 1 + 1 = 76.
#pragma once
#include "wu_host.h"

namespace wu {
constexpr int kC[4] = {32, 64, 96, 128};
struct Res { std::string p; int ci, co, g; };
struct Samp { std::string p; int c; bool up; };
// the ResnetBlocks and resampling layers in forward order: item k is res[k.first] (k.second == 0) or samp[k.first]
struct Net {
  std::vector<Res> res; std::vector<Samp> samp;
  std::vector<std::pair<int, int>> order;
};
static Net build_net() {
  Net n;
  auto res = [&](const std::string& p, int ci, int co, int g) { n.order.push_back({(int)n.res.size(), 0}); n.res.push_back({p, ci, co, g}); };
  auto samp = [&](const std::string& p, int c, bool up) { n.order.push_back({(int)n.samp.size(), 1}); n.samp.push_back({p, c, up}); };
  for (int i = 0; i < 3; ++i) {
    const std::string p = "waveunet.downsampling_blocks." + std::to_string(i) + ".";
    const int cin = i == 0 ? 2 : kC[i], g = i == 0 ? 2 : 32;
    res(p + "pre_shortcut.0.res_block.", cin, kC[i], g);
    res(p + "post_shortcut.0.res_block.", kC[i], kC[i + 1], g);
    samp(p + "downconv.down.", kC[i + 1], false);
  }
  for (int j = 0; j < 2; ++j) res("waveunet.bottlenecks." + std::to_string(j) + ".res_block.", kC[3], kC[3], 32);
  for (int j = 0; j < 3; ++j) {
    const int i = 3 - j;
    const std::string p = "waveunet.upsampling_blocks." + std::to_string(j) + ".";
    samp(p + "upconv.up.", kC[i], true);
    res(p + "pre_shortcut.0.res_block.", kC[i], kC[i - 1], 32);
    res(p + "post_shortcut.0.res_block.", kC[i - 1], kC[i - 1], 32);
  }
  return n;
}
}  // namespace wu

struct WUState : SeqNet {
  wu::Net net = wu::build_net();
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  WULevel lv{};                                       // the noise level of the current call (begin)
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) override;
  int network(sddm_ctx* c, const float* cond, const float* x_t, int per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
};

// refuses everything the kernels are not instantiated for (the arguments of config_waveunet3.json are)
static int wu_check_config(const Json& na) {
  const std::vector<int> ch = na.ints("num_channels", {});
  if (ch != std::vector<int>{32, 64, 96, 128}) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 num_channels other than [32, 64, 96, 128]");
  if ((int)na.number("num_inputs", 0) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 num_inputs %d (2: condition and y_t)", (int)na.number("num_inputs", 0));
  for (const char* k : {"downconv_kernel_size", "upconv_kernel_size", "bottleneck_kernel_size"})
    if ((int)na.number(k, 0) != 5) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 %s %d (5)", k, (int)na.number(k, 0));
  if ((int)na.number("conv_stride", 0) != 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 conv_stride %d (1)", (int)na.number("conv_stride", 0));
  if (na.string("conv_type", "") != "gn") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 conv_type '%s' ('gn')", na.string("conv_type", "").c_str());
  for (const char* k : {"downsample_kernel_size", "upsample_kernel_size"})
    if ((int)na.number(k, 4) != 4) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 %s %d (4)", k, (int)na.number(k, 4));
  if ((int)na.number("resample_stride", 2) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 resample_stride %d (2)", (int)na.number("resample_stride", 2));
  if ((int)na.number("norm_groups", 32) != 32) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 norm_groups %d (32)", (int)na.number("norm_groups", 32));
  if (na.number("with_noise_level_emb", 0) != 0) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 with_noise_level_emb (waveunet3.py:325-326)");
  if (na.number("with_attn", 1) != 0) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet3 with_attn (self-attention has no kernels)");
  return SDDM_OK;
}

// state-dict shapes (waveunet3.py:314-363) without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> wu_param_shapes(const wu::Net& n) {
  std::map<std::string, std::vector<int64_t>> s;
  for (const wu::Res& r : n.res) {
    s[r.p + "noise_func.noise_func.0.weight"] = {r.co, 1};
    s[r.p + "noise_func.noise_func.0.bias"] = {r.co};
    for (int k = 1; k <= 2; ++k) {
      const std::string b = r.p + "block" + std::to_string(k) + ".block.";
      const int c = k == 1 ? r.ci : r.co;
      s[b + "0.weight"] = {c}; s[b + "0.bias"] = {c};
      s[b + "3.weight"] = {r.co, c, 5}; s[b + "3.bias"] = {r.co};
    }
    if (r.ci != r.co) { s[r.p + "res_conv.weight"] = {r.co, r.ci, 1}; s[r.p + "res_conv.bias"] = {r.co}; }
  }
  for (const wu::Samp& q : n.samp) {
    s[q.p + "filter.weight"] = {q.c, q.c, 4}; s[q.p + "filter.bias"] = {q.c};
    s[q.p + "norm.weight"] = {q.c}; s[q.p + "norm.bias"] = {q.c};
  }
  s["waveunet.output_conv.weight"] = {1, 32, 1};
  s["waveunet.output_conv.bias"] = {1};
  return s;
}

size_t WUState::pack(sddm_ctx* c, WeightPacker& pk) {
  const WUState& d = *this;
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  auto add_f32 = [&](const std::string& name, const std::vector<float>& v) { pk.f32(name, v); };
  for (const wu::Res& r : d.net.res) {
    const std::string& p = r.p;
    add_f32(p + "nw", P(p + "noise_func.noise_func.0.weight"));
    add_f32(p + "nb", P(p + "noise_func.noise_func.0.bias"));
    add_f32(p + "g1", P(p + "block1.block.0.weight"));
    add_f32(p + "e1", P(p + "block1.block.0.bias"));
    add_f32(p + "b1", P(p + "block1.block.3.bias"));
    if (r.ci == 2) add_f32(p + "w1", P(p + "block1.block.3.weight"));           // stem: fp32 [32][2][5], VALU kernel
    else wu_add_conv(c, pk, p + "w1", r.co, r.ci, 5, P(p + "block1.block.3.weight"), false);
    add_f32(p + "g2", P(p + "block2.block.0.weight"));
    add_f32(p + "e2", P(p + "block2.block.0.bias"));
    wu_add_conv(c, pk, p + "w2", r.co, r.co, 5, P(p + "block2.block.3.weight"), false);
    std::vector<float> b2 = P(p + "block2.block.3.bias");
    if (r.ci != r.co) {                                                         // res_conv's bias rides on block2's
      const std::vector<float>& rb = P(p + "res_conv.bias");
      for (int i = 0; i < r.co; ++i) b2[i] += rb[i];
      if (r.ci == 2) add_f32(p + "rw", P(p + "res_conv.weight"));               // fp32 [32][2]
      else wu_add_conv(c, pk, p + "rw", r.co, r.ci, 1, P(p + "res_conv.weight"), false);
    }
    add_f32(p + "b2", b2);
  }
  for (const wu::Samp& q : d.net.samp) {
    wu_add_conv(c, pk, q.p + "w", q.c, q.c, 4, P(q.p + "filter.weight"), q.up);
    add_f32(q.p + "b", P(q.p + "filter.bias"));
    add_f32(q.p + "g", P(q.p + "norm.weight"));
    add_f32(q.p + "e", P(q.p + "norm.bias"));
  }
  add_f32("out.w", P("waveunet.output_conv.weight"));
  add_f32("out.b", P("waveunet.output_conv.bias"));
  return 0;                                            // no table of its own: the level is one scalar per t
}

// activation buffers for (B, N): name -> [B][len][C] in the compute dtype
int WUState::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  WUState& d = *this;
  TRY(wu_check_shape("Waveunet3", B, N));
  if (d.B == B && d.N == N) return SDDM_OK;
  const size_t es = dtype_size(c->dtype);
  Arena& A = d.act;
  A.reset();
  d.aoff.clear();
  auto buf = [&](const std::string& n, int64_t len, int C) { d.aoff[n] = A.reserve(es * (size_t)B * len * C); };
  int64_t len = N;
  int ri = 0;
  for (const auto& it : d.net.order) {
    if (it.second == 0) {
      const wu::Res& r = d.net.res[it.first];
      buf("h" + std::to_string(ri), len, r.co);        // block1's output
      buf("o" + std::to_string(ri), len, r.co);        // the block's output
      ++ri;
    } else {
      const wu::Samp& q = d.net.samp[it.first];
      len = q.up ? len * 2 : len / 2;
      buf("r" + q.p, len, q.c);                        // raw conv output
      buf("y" + q.p, len, q.c);                        // ReLU(GN(raw))
    }
  }
  // statistics partials of the latest producer: stem 8 slots per 256 positions, convs 4 per 128, wu_act 1 per 64
  const int64_t max_slots = 8 * ((N + kWuStemTile - 1) / kWuStemTile) + 8;
  d.aoff["stats"] = A.reserve(sizeof(float) * (size_t)B * max_slots * 128 * 2);
  d.aoff["scale"] = A.reserve(sizeof(float) * (size_t)B * 128);
  d.aoff["shift"] = A.reserve(sizeof(float) * (size_t)B * 128);
  d.aoff["eps"] = A.reserve(sizeof(float) * (size_t)B * N);
  SDDM_HIP_CHECK(A.commit());
  d.B = (int)B;
  d.N = N;
  return SDDM_OK;
}

// the noise level the ResnetBlocks add: sqrt_alpha_bar[t] or t of the step counter (sampling,
// model.py:84-89) or the caller's [B] (a forward).  No launch
int WUState::begin(sddm_ctx* c, const float*, const float* noise_level, hipStream_t) {
  lv = wu_begin_level(c, noise_level, off_sp);
  return SDDM_OK;
}

// one forward (waveunet3.py:383-416): cond, x_t [B][N] fp32 -> clamp(output_conv) = eps [B][N] fp32 (aoff "eps")
int WUState::network(sddm_ctx* c, const float* cond, const float* x_t, int, int* t_dev, hipStream_t s) {
  WUState& d = *this;
  const Arena& W = c->warena;
  const int B = d.B;
  const int64_t N = d.N;
  const int dt = c->dtype;
  auto act = [&](const std::string& n) -> char* { return d.act.base + d.aoff.at(n); };
  auto wf = [&](const std::string& n) -> const float* { return W.at<float>(d.woff.at(n)); };
  float* stats = d.act.at<float>(d.aoff.at("stats"));
  float* scale = d.act.at<float>(d.aoff.at("scale"));
  float* shift = d.act.at<float>(d.aoff.at("shift"));
  int cur_slots = 0;                                   // partials in `stats`: of the latest producer
  // scale / shift of GroupNorm(G, C) with the named affine over the latest producer's [B][L][C]
  auto finalize = [&](int C, int G, int64_t L, const std::string& gamma, const std::string& beta) -> int {
    WUGnArgs g{stats, cur_slots, C, G, L, wf(gamma), wf(beta), 1e-5f, scale, shift, B};
    TRY_LAUNCH("wu_gn_finalize", launch_wu_gn_finalize(g, s));
    return SDDM_OK;
  };
  const char* x = nullptr;                             // the running activation [B][len][xc]
  int64_t len = N;
  int ri = 0;
  std::vector<std::string> shortcuts;
  for (const auto& it : d.net.order) {
    if (it.second == 0) {                              // ResnetBlock (waveunet3.py:73-89)
      const wu::Res& r = d.net.res[it.first];
      const std::string& p = r.p;
      const std::string hn = "h" + std::to_string(ri), on = "o" + std::to_string(ri);
      ++ri;
      const bool stem = r.ci == 2;
      const bool up_pre = p.find("upsampling") != std::string::npos && p.find("pre_shortcut") != std::string::npos;
      if (stem) {
        WUInStatsArgs ia{cond, x_t, B, (int)len, wf(p + "g1"), wf(p + "e1"), 1e-5f, scale, shift, t_dev};
        TRY_LAUNCH("wu_in_stats", launch_wu_in_stats(ia, s));
        WUStemArgs sa{cond, x_t, scale, shift, wf(p + "w1"), wf(p + "b1"), wf(p + "nw"), wf(p + "nb"), lv, act(hn), stats, B, (int)len, nullptr};
        TRY_LAUNCH("wu_stem", launch_wu_stem(dt, sa, s));
        cur_slots = 8 * (int)((len + kWuStemTile - 1) / kWuStemTile);
      } else {
        TRY(finalize(r.ci, r.g, len, p + "g1", p + "e1"));
        WUConvArgs a{};
        a.mode = WU_CONV5; a.src = x; a.Lin = (int)len; a.Cin = r.ci; a.scale = scale; a.shift = shift;
        a.w = W.base + d.woff.at(p + "w1"); a.bias = wf(p + "b1"); a.nw = wf(p + "nw"); a.nb = wf(p + "nb"); a.lv = lv;
        a.out = act(hn); a.Lout = (int)len; a.Cout = r.co; a.stats = stats; a.B = B;
        TRY_LAUNCH("wu_conv block1", launch_wu_conv(dt, a, s));
        cur_slots = wu_conv_slots((int)len);
      }
      TRY(finalize(r.co, r.g, len, p + "g2", p + "e2"));
      WUConvArgs a{};
      a.mode = WU_CONV5; a.src = act(hn); a.Lin = (int)len; a.Cin = r.co; a.scale = scale; a.shift = shift;
      a.w = W.base + d.woff.at(p + "w2"); a.bias = wf(p + "b2");
      if (stem) { a.res_mode = 3; a.cond = cond; a.x = x_t; a.rw2 = wf(p + "rw"); }
      else if (r.ci != r.co) { a.res_mode = 2; a.res = x; a.RC = r.ci; a.rw = W.base + d.woff.at(p + "rw"); }
      else { a.res_mode = 1; a.res = x; }
      if (up_pre) {                                    // combined = upsampled + shortcut (waveunet3.py:258)
        a.shortcut = act(shortcuts.back());
        shortcuts.pop_back();
      }
      a.out = act(on); a.Lout = (int)len; a.Cout = r.co; a.stats = stats; a.B = B;
      TRY_LAUNCH("wu_conv block2", launch_wu_conv(dt, a, s));
      cur_slots = wu_conv_slots((int)len);
      if (p.find("downsampling") != std::string::npos && p.find("pre_shortcut") != std::string::npos) shortcuts.push_back(on);
      x = act(on);
    } else {                                           // ConvLayer (waveunet3.py:140-179)
      const wu::Samp& q = d.net.samp[it.first];
      const int64_t lout = q.up ? len * 2 : len / 2;
      WUConvArgs a{};
      a.mode = q.up ? WU_UP4 : WU_DOWN4; a.src = x; a.Lin = (int)len; a.Cin = q.c;
      a.w = W.base + d.woff.at(q.p + "w"); a.bias = wf(q.p + "b");
      a.out = act("r" + q.p); a.Lout = (int)lout; a.Cout = q.c; a.stats = stats; a.B = B;
      TRY_LAUNCH("wu_conv resample", launch_wu_conv(dt, a, s));
      cur_slots = wu_conv_slots((int)lout);
      len = lout;
      TRY(finalize(q.c, q.c / 8, len, q.p + "g", q.p + "e"));
      WUActArgs aa{act("r" + q.p), scale, shift, act("y" + q.p), stats, B, (int)len, q.c};
      TRY_LAUNCH("wu_act", launch_wu_act(dt, aa, s));
      cur_slots = (int)((len + kWuActTile - 1) / kWuActTile);
      x = act("y" + q.p);
    }
  }
  WUHeadArgs ha{x, wf("out.w"), wf("out.b"), d.act.at<float>(d.aoff.at("eps")), B, (int)N};
  TRY_LAUNCH("wu_head", launch_wu_head(dt, ha, s));
  return SDDM_OK;
}
