// Waveunet path of the runtime (included by sddm_runtime.cpp after wu2_runtime.h): configuration
// check, weight packing, workspace and forward of reference model/waveunet.py:358-506 at the
// arguments of config_waveunet.json as a SeqNet; seq_sample runs SDDM.infer (model.py:50-124) over
// it.  Kernels: waveunet1.hip (the convs), waveunet2.hip (stem, head), waveunet.hip (finalize).
//
// Layers (C_i = 24 (i + 1), i = 0..11; L_i = N / 2^i; depth 1; a ConvLayer is filter ->
// GroupNorm(groups of 8) -> ReLU):
//   down i = 0..10  pre_shortcut  ConvLayer(k5, in -> C_i) at L_i (in = the 2 raw channels for i = 0):
//                                 the shortcut
//                   film_blocks.i FiLM on the shortcut: Conv3 C_i -> C_i, leaky_relu(0.2), + encoding
//                                 of the level, Conv3 C_i -> 2 C_i = (shift, scale)
//                   post_shortcut ConvLayer(k5, C_i -> C_i+1)
//                   downconv      ConvLayer(k4, stride 2, padding 1), to L_i+1
//   bottleneck      ConvLayer(k5, 288 -> 288) at L_11
//   up i = 11..1    upconv        ConvLayer(ConvTranspose k4, stride 2, padding 1, C_i -> C_i), to L_i-1
//                   pre_shortcut  ConvLayer(k5, C_i -> C_i-1)
//                   post_shortcut ConvLayer(k5, C_i-1 -> C_i-1) of scale * v + shift (FiLM of down i-1)
//   output_conv     Conv 1x1 24 -> 1, clamp
// The statistics scheme is Waveunet2's (wu2_runtime.h): raw conv outputs and partials are stored,
// a finalize launch makes scale / shift, the consumers normalise while they stage.
//
// Path per layer.  A layer runs wu_conv_kernel per batch row (launch_wu1_conv) and a finalize
// launch.  One whose output rows are shorter than a conv tile (128 positions) can instead run the
// batch-folded kernel (launch_wu1_fold), whose blocks own whole rows and write scale / shift
// themselves; wu1::fold_default says at which lengths it does by default (none: it measured
// slower).  Both launches of a layer's neighbours read one scale / shift pair while the folded
// kernel writes the next, so the two pairs alternate layer by layer.  Read from the environment when
// the context is configured: SDDM_WU_NO_FOLD=1 sends every layer down the per-row path,
// SDDM_WU_FOLD_ALL=1 every short layer down the folded one whatever wu1::fold_default says.
//
// Launches per reverse step: stem 1 (it steps t), 66 MFMA ConvLayer convs, 22 FiLM convs, head 1,
// transition 1, and one finalize per per-row ConvLayer: 67 on the per-row path -- 1 + 66 + 67 + 22
// + 1 + 1 = 158, the default.  At 16384 samples levels 8 to 11 are short (64 ... 8 positions): with
// SDDM_WU_FOLD_ALL the 20 ConvLayers from downconv 7 to the post_shortcut conv of upsampling block 2
// lose their finalize -- 138.
#pragma once
#include "wu1_kernels.h"
#include "wu_host.h"

namespace wu1 {
constexpr int kLevels = 12;
constexpr int kHop = 1 << (kLevels - 1);              // 2048: the length halves eleven times
inline int ch(int i) { return 24 * (i + 1); }
// the ConvLayers in forward order (wu2::Layer: film >= 0: the output is that level's shortcut, use
// >= 0: the input takes that level's FiLM).  The learned resampling convs sit directly under
// downconv / upconv here (waveunet.py:335, 278), not under .down / .up as in Waveunet2
static std::vector<wu2::Layer> build_net() {
  std::vector<wu2::Layer> n;
  for (int i = 0; i < kLevels - 1; ++i) {
    const std::string p = "waveunet.downsampling_blocks." + std::to_string(i) + ".";
    n.push_back({p + "pre_shortcut_convs.0.", sddm::WU_CONV5, i == 0 ? 2 : ch(i), ch(i), i, -1});
    n.push_back({p + "post_shortcut_convs.0.", sddm::WU_CONV5, ch(i), ch(i + 1), -1, -1});
    n.push_back({p + "downconv.", sddm::WU_DOWN4, ch(i + 1), ch(i + 1), -1, -1});
  }
  n.push_back({"waveunet.bottlenecks.0.", sddm::WU_CONV5, ch(kLevels - 1), ch(kLevels - 1), -1, -1});
  for (int j = 0; j < kLevels - 1; ++j) {
    const int i = kLevels - 1 - j;
    const std::string p = "waveunet.upsampling_blocks." + std::to_string(j) + ".";
    n.push_back({p + "upconv.", sddm::WU_UP4, ch(i), ch(i), -1, -1});
    n.push_back({p + "pre_shortcut_convs.0.", sddm::WU_CONV5, ch(i), ch(i - 1), -1, -1});
    n.push_back({p + "post_shortcut_convs.0.", sddm::WU_CONV5, ch(i - 1), ch(i - 1), -1, i - 1});
  }
  return n;
}
// whether a layer with output rows of `lout` < 128 positions takes the batch-folded kernel by
// default: only where the measurement of DESIGN 3f has its launches more than 5 % ahead of the
// per-row ones.  At B = 16 x 16384 in bf16 they are behind at every short length (kernel time per
// step, folded / per-row with its finalizes: L = 64 329 / 193 us, 32 360 / 199, 16 440 / 213,
// 8 145 / 54), so the per-row path is the default everywhere
inline bool fold_default(int) { return false; }
}  // namespace wu1

struct WU1State : SeqNet {
  std::vector<wu2::Layer> net = wu1::build_net();
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  WULevel lv{};                                       // the noise level of the current call (begin)
  // 0 never, 1 where wu1::fold_default says, 2 every short layer (configure).  fold_default folds
  // at no length today, so 0 and 1 run the same launches; 1 is where a per-length default would act
  int fold = 1;
  bool folded(int64_t lout) const { return lout < kWuTile && (fold == 2 || (fold == 1 && wu1::fold_default((int)lout))); }
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) override;
  int network(sddm_ctx* c, const float* cond, const float* x_t, int per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
};

// refuses everything the layer table is not built for (the arguments of config_waveunet.json are)
static int wu1_check_config(const Json& na) {
  std::vector<int> want;
  for (int i = 0; i < wu1::kLevels; ++i) want.push_back(wu1::ch(i));
  if (na.ints("num_channels", {}) != want) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet num_channels other than [24, 48, ..., 288] (twelve levels)");
  if ((int)na.number("num_inputs", 0) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet num_inputs %d (2: condition and y_t)", (int)na.number("num_inputs", 0));
  if ((int)na.number("kernel_size", 0) != 5) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet kernel_size %d (5)", (int)na.number("kernel_size", 0));
  if (na.string("res", "") != "learned") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet res '%s' ('learned': the fixed sinc resampler is not built)", na.string("res", "").c_str());
  if (na.string("conv_type", "") != "gn") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet conv_type '%s' ('gn')", na.string("conv_type", "").c_str());
  if ((int)na.number("depth", 1) != 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet depth %d (1)", (int)na.number("depth", 1));
  if ((int)na.number("resample_kernel_size", 4) != 4) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet resample_kernel_size %d (4)", (int)na.number("resample_kernel_size", 4));
  if ((int)na.number("resample_stride", 2) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet resample_stride %d (2)", (int)na.number("resample_stride", 2));
  return SDDM_OK;
}

// state-dict shapes (waveunet.py:379-394) without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> wu1_param_shapes(const std::vector<wu2::Layer>& n) {
  std::map<std::string, std::vector<int64_t>> s;
  for (const wu2::Layer& l : n) {
    const int k = wu2::taps(l.mode);
    if (l.mode == sddm::WU_UP4) s[l.p + "filter.weight"] = {l.ci, l.co, k};   // ConvTranspose1d: [ci][co][k]
    else s[l.p + "filter.weight"] = {l.co, l.ci, k};
    s[l.p + "filter.bias"] = {l.co};
    s[l.p + "norm.weight"] = {l.co}; s[l.p + "norm.bias"] = {l.co};
  }
  for (int i = 0; i < wu1::kLevels - 1; ++i) {
    const int c = wu1::ch(i);
    s[wu2::film(i) + "input_conv.weight"] = {c, c, 3}; s[wu2::film(i) + "input_conv.bias"] = {c};
    s[wu2::film(i) + "output_conv.weight"] = {2 * c, c, 3}; s[wu2::film(i) + "output_conv.bias"] = {2 * c};
  }
  s["waveunet.output_conv.weight"] = {1, wu1::ch(0), 1};
  s["waveunet.output_conv.bias"] = {1};
  return s;
}

size_t WU1State::pack(sddm_ctx* c, WeightPacker& pk) {
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  for (const wu2::Layer& l : net) {
    if (l.ci == 2) pk.f32(l.p + "w", P(l.p + "filter.weight"));                  // stem: fp32 [24][2][5], VALU kernel
    else wu_add_conv(c, pk, l.p + "w", l.co, l.ci, wu2::taps(l.mode), P(l.p + "filter.weight"), l.mode == sddm::WU_UP4);
    pk.f32(l.p + "b", P(l.p + "filter.bias"));
    pk.f32(l.p + "g", P(l.p + "norm.weight"));
    pk.f32(l.p + "e", P(l.p + "norm.bias"));
  }
  for (int i = 0; i < wu1::kLevels - 1; ++i) {
    const std::string f = wu2::film(i);
    wu_add_conv(c, pk, f + "iw", wu1::ch(i), wu1::ch(i), 3, P(f + "input_conv.weight"), false);
    pk.f32(f + "ib", P(f + "input_conv.bias"));
    wu_add_conv(c, pk, f + "ow", 2 * wu1::ch(i), wu1::ch(i), 3, P(f + "output_conv.weight"), false);
    pk.f32(f + "ob", P(f + "output_conv.bias"));
  }
  pk.f32("out.w", P("waveunet.output_conv.weight"));
  pk.f32("out.b", P("waveunet.output_conv.bias"));
  return 0;                                            // no table of its own: the level is one scalar per t
}

// activation buffers for (B, N): name -> [B][len][C] in the compute dtype
int WU1State::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  WU1State& d = *this;
  if (B < 1 || B > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)B);
  if (N < wu1::kHop || N % wu1::kHop)
    FAIL(SDDM_ERR_SHAPE, "%lld samples is not a positive multiple of %d (Waveunet halves the length eleven times)", (long long)N, wu1::kHop);
  if (N > (int64_t)1 << 30) FAIL(SDDM_ERR_SHAPE, "%lld samples: Waveunet positions are 32-bit", (long long)N);
  if (d.B == B && d.N == N) return SDDM_OK;
  const size_t es = dtype_size(c->dtype);
  Arena& A = d.act;
  A.reset();
  d.aoff.clear();
  auto buf = [&](const std::string& n, int64_t len, int C) { d.aoff[n] = A.reserve(es * (size_t)B * len * C); };
  // statistics partials of the latest producer, [slots][C][2] per row: stem 8 slots per 256
  // positions, convs 4 per 128
  size_t max_cells = (size_t)8 * ((N + kWuStemTile - 1) / kWuStemTile) * wu1::ch(0);
  int64_t len = N;
  for (size_t k = 0; k < d.net.size(); ++k) {
    const wu2::Layer& l = d.net[k];
    if (l.mode == sddm::WU_DOWN4) len /= 2;
    if (l.mode == sddm::WU_UP4) len *= 2;
    buf("r" + std::to_string(k), len, l.co);           // the layer's raw conv output
    if (l.film >= 0) {
      buf("fi" + std::to_string(l.film), len, l.co);   // FiLM input_conv's output
      buf("fo" + std::to_string(l.film), len, 2 * l.co);   // (shift, scale)
    }
    max_cells = std::max(max_cells, (size_t)wu_conv_slots((int)len) * l.co);
  }
  d.aoff["stats"] = A.reserve(sizeof(float) * (size_t)B * max_cells * 2);
  for (const char* n : {"scale0", "shift0", "scale1", "shift1"}) d.aoff[n] = A.reserve(sizeof(float) * (size_t)B * kWu1MaxC);
  d.aoff["eps"] = A.reserve(sizeof(float) * (size_t)B * N);
  SDDM_HIP_CHECK(A.commit());
  d.B = (int)B;
  d.N = N;
  return SDDM_OK;
}

// the noise level the FiLM encodings take (wu2_runtime.h).  No launch
int WU1State::begin(sddm_ctx* c, const float*, const float* noise_level, hipStream_t) {
  lv = wu_begin_level(c, noise_level, off_sp);
  return SDDM_OK;
}

// one forward (waveunet.py:475-506): cond, x_t [B][N] fp32 -> clamp(output_conv) = eps [B][N] fp32 (aoff "eps")
int WU1State::network(sddm_ctx* c, const float* cond, const float* x_t, int, int* t_dev, hipStream_t s) {
  WU1State& d = *this;
  const Arena& W = c->warena;
  const int B = d.B;
  const int dt = c->dtype;
  auto act = [&](const std::string& n) -> char* { return d.act.base + d.aoff.at(n); };
  auto wf = [&](const std::string& n) -> const float* { return W.at<float>(d.woff.at(n)); };
  float* stats = d.act.at<float>(d.aoff.at("stats"));
  float* const scales[2] = {d.act.at<float>(d.aoff.at("scale0")), d.act.at<float>(d.aoff.at("scale1"))};
  float* const shifts[2] = {d.act.at<float>(d.aoff.at("shift0")), d.act.at<float>(d.aoff.at("shift1"))};
  int cur = 0;                                         // the pair that holds the latest ConvLayer's norm
  float* scale = scales[0];
  float* shift = shifts[0];
  // one conv: folded when its rows are short; ol non-null: a ConvLayer, its norm goes to the other pair
  auto conv = [&](const char* what, const WU2ConvArgs& a, const wu2::Layer* ol) -> int {
    if (d.folded(a.Lout)) {
      WU1FoldArgs f{};
      static_cast<WU2ConvArgs&>(f) = a;
      f.stats = nullptr;
      if (ol) { f.gamma = wf(ol->p + "g"); f.beta = wf(ol->p + "e"); f.eps = 1e-5f; f.oscale = scales[cur ^ 1]; f.oshift = shifts[cur ^ 1]; }
      TRY_LAUNCH(what, launch_wu1_fold(dt, f, s));
    } else {
      TRY_LAUNCH(what, launch_wu1_conv(dt, a, s));
    }
    return SDDM_OK;
  };
  const char* x = nullptr;                             // the latest ConvLayer's raw output [B][len][C]; scale / shift are its norm
  int64_t len = d.N;
  for (size_t k = 0; k < d.net.size(); ++k) {
    const wu2::Layer& l = d.net[k];
    const int64_t lout = l.mode == sddm::WU_DOWN4 ? len / 2 : (l.mode == sddm::WU_UP4 ? len * 2 : len);
    char* out = act("r" + std::to_string(k));
    int slots;
    if (l.ci == 2) {
      WUStemArgs sa{};
      sa.cond = cond; sa.x = x_t; sa.w = wf(l.p + "w"); sa.bias = wf(l.p + "b");
      sa.out = out; sa.stats = stats; sa.B = B; sa.L = (int)len; sa.t_dev = t_dev;
      TRY_LAUNCH("wu2_stem", launch_wu2_stem(dt, sa, s));
      slots = 8 * (int)((len + kWuStemTile - 1) / kWuStemTile);
    } else {
      WU2ConvArgs a{};
      a.mode = l.mode; a.src = x; a.Lin = (int)len; a.Cin = l.ci; a.scale = scale; a.shift = shift;
      if (l.use >= 0) a.film = act("fo" + std::to_string(l.use));
      a.w = W.base + d.woff.at(l.p + "w"); a.bias = wf(l.p + "b");
      a.out = out; a.Lout = (int)lout; a.Cout = l.co; a.stats = stats; a.B = B;
      TRY(conv("wu1_conv ConvLayer", a, &l));
      slots = wu_conv_slots((int)lout);
    }
    len = lout;
    x = out;
    cur ^= 1;
    scale = scales[cur];
    shift = shifts[cur];
    if (l.ci == 2 || !d.folded(lout)) {
      WUGnArgs g{stats, slots, l.co, l.co / 8, len, wf(l.p + "g"), wf(l.p + "e"), 1e-5f, scale, shift, B};
      TRY_LAUNCH("wu_gn_finalize", launch_wu_gn_finalize(g, s));
    }
    if (l.film >= 0) {                                 // FiLM of the shortcut (waveunet.py:56-61)
      const std::string f = wu2::film(l.film), n = std::to_string(l.film);
      WU2ConvArgs a{};
      a.mode = WU_CONV3; a.src = x; a.Lin = (int)len; a.Cin = l.co; a.scale = scale; a.shift = shift;
      a.w = W.base + d.woff.at(f + "iw"); a.bias = wf(f + "ib"); a.enc_dim = l.co; a.lv = lv;
      a.out = act("fi" + n); a.Lout = (int)len; a.Cout = l.co; a.B = B;
      TRY(conv("wu1_conv FiLM input_conv", a, nullptr));
      WU2ConvArgs o{};
      o.mode = WU_CONV3; o.src = act("fi" + n); o.Lin = (int)len; o.Cin = l.co;
      o.w = W.base + d.woff.at(f + "ow"); o.bias = wf(f + "ob");
      o.out = act("fo" + n); o.Lout = (int)len; o.Cout = 2 * l.co; o.B = B;
      TRY(conv("wu1_conv FiLM output_conv", o, nullptr));
    }
  }
  WU2HeadArgs ha{x, scale, shift, wf("out.w"), wf("out.b"), d.act.at<float>(d.aoff.at("eps")), B, (int)d.N};
  TRY_LAUNCH("wu2_head", launch_wu2_head(dt, ha, s));
  return SDDM_OK;
}
