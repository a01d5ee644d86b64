// The FiLM Wave-U-Net path of the runtime (included by sddm_runtime.cpp after sddm_ctx and SeqNet):
// configuration check, weight packing, workspace and forward of the reference's two FiLM
// Wave-U-Nets as one SeqNet (WUFilmState) over a constant descriptor (wu2::Net); seq_sample runs
// SDDM.infer (model.py:50-124) over it.
//   Waveunet2  model/waveunet2.py:226-324 at the arguments of config_waveunet2.json: 4 levels
//   Waveunet   model/waveunet.py:358-506 at the arguments of config_waveunet.json: 12 levels
// They are the same network at two sizes and differ in the descriptor's fields only: the number of
// levels, the state-dict key of the learned resampling convs, and the conv launcher (Waveunet2's
// blocks hold the whole Cout, waveunet2.hip; Waveunet's a group of it, waveunet1.hip).  The stem, the
// head (waveunet2.hip) and the finalize (waveunet.hip) are shared.
//
// Layers (n levels, C_i = 24 (i + 1), L_i = N / 2^i, depth 1; a ConvLayer is filter ->
// GroupNorm(groups of 8) -> ReLU):
//   down i = 0..n-2 pre_shortcut  ConvLayer(k5, in -> C_i) at L_i (in = the 2 raw channels for i = 0):
//                                 the shortcut
//                   film_blocks.i FiLM on the shortcut: Conv3 C_i -> C_i, leaky_relu(0.2), + encoding
//                                 of the level, Conv3 C_i -> 2 C_i = (shift, scale)
//                   post_shortcut ConvLayer(k5, C_i -> C_i+1)
//                   downconv      ConvLayer(k4, stride 2, padding 1), to L_i+1
//   bottleneck      ConvLayer(k5, C_n-1 -> C_n-1) at L_n-1
//   up i = n-1..1   upconv        ConvLayer(ConvTranspose k4, stride 2, padding 1, C_i -> C_i), to L_i-1
//                   pre_shortcut  ConvLayer(k5, C_i -> C_i-1)
//                   post_shortcut ConvLayer(k5, C_i-1 -> C_i-1) of scale * v + shift (FiLM of down i-1)
//   output_conv     Conv 1x1 24 -> 1, clamp
//
// Statistics.  Every ConvLayer stores its raw conv output and leaves (sum, sum of squares) partials
// of it in the one statistics buffer; a finalize launch turns them into the per-(row, channel)
// scale / shift, and every consumer of the layer (the next conv; for a shortcut also the FiLM
// input_conv; for the last layer the head) applies ReLU(raw * scale + shift) while it stages its
// input.  No activated copy is stored and nothing is normalised twice.  There is one scale / shift
// pair: the finalize of layer k is stream-ordered behind the conv that read the pair of layer k - 1.
//
// Launches per reverse step: stem 1 (it steps t), 6 (n - 1) MFMA ConvLayer convs, one finalize per
// ConvLayer (6 (n - 1) + 1), 2 (n - 1) FiLM convs (the encoding is computed in the input_conv's
// epilogue), head 1, transition 1 -- Waveunet2 1 + 18 + 19 + 6 + 1 + 1 = 46, Waveunet
// 1 + 66 + 67 + 22 + 1 + 1 = 158, at any N.
#pragma once
#include "wu2_kernels.h"
#include "wu_host.h"

namespace wu2 {
// what the two networks differ in
struct Net {
  const char* name;                                   // for messages
  int levels;                                         // the length halves levels - 1 times: N is a multiple of 2^(levels - 1)
  const char* down; const char* up;                   // the learned resampling convs' keys in their blocks
  hipError_t (*conv)(int dtype, const sddm::WU2ConvArgs& a, hipStream_t s);
  int (*check_config)(const Json& args);              // refuses the arguments the table is not built for
};
constexpr int kLevels2 = 4, kLevels1 = 12;             // the levels of Waveunet2 and of Waveunet
inline int ch(int i) { return 24 * (i + 1); }
// the ConvLayers in forward order; film >= 0: the layer's output is the shortcut of that level (the
// FiLM block runs behind it), use >= 0: the layer's input takes the FiLM of that level
struct Layer { std::string p; int mode, ci, co, film, use; };
static std::vector<Layer> build_net(const Net& d) {
  std::vector<Layer> n;
  const int top = d.levels - 1;
  for (int i = 0; i < top; ++i) {
    const std::string p = "waveunet.downsampling_blocks." + std::to_string(i) + ".";
    n.push_back({p + "pre_shortcut_convs.0.", sddm::WU_CONV5, i == 0 ? 2 : ch(i), ch(i), i, -1});
    n.push_back({p + "post_shortcut_convs.0.", sddm::WU_CONV5, ch(i), ch(i + 1), -1, -1});
    n.push_back({p + d.down, sddm::WU_DOWN4, ch(i + 1), ch(i + 1), -1, -1});
  }
  n.push_back({"waveunet.bottlenecks.0.", sddm::WU_CONV5, ch(top), ch(top), -1, -1});
  for (int j = 0; j < top; ++j) {
    const int i = top - j;
    const std::string p = "waveunet.upsampling_blocks." + std::to_string(j) + ".";
    n.push_back({p + d.up, sddm::WU_UP4, ch(i), ch(i), -1, -1});
    n.push_back({p + "pre_shortcut_convs.0.", sddm::WU_CONV5, ch(i), ch(i - 1), -1, -1});
    n.push_back({p + "post_shortcut_convs.0.", sddm::WU_CONV5, ch(i - 1), ch(i - 1), -1, i - 1});
  }
  return n;
}
inline int taps(int mode) { return mode == sddm::WU_CONV5 ? 5 : (mode == sddm::WU_CONV3 ? 3 : 4); }
inline std::string film(int i) { return "waveunet.film_blocks." + std::to_string(i) + "."; }
}  // namespace wu2

struct WUFilmState : SeqNet {
  const wu2::Net& desc;
  std::vector<wu2::Layer> net;
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  WULevel lv{};                                       // the noise level of the current call (begin)
  explicit WUFilmState(const wu2::Net& d) : desc(d), net(wu2::build_net(d)) {}
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) override;
  int network(sddm_ctx* c, const float* cond, const float* x_t, int per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
};

// refuses everything the kernels are not instantiated for (the arguments of config_waveunet2.json are)
static int wu2_check_config(const Json& na) {
  const std::vector<int> ch = na.ints("num_channels", {});
  if (ch != std::vector<int>{24, 48, 72, 96}) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 num_channels other than [24, 48, 72, 96]");
  if ((int)na.number("num_inputs", 0) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 num_inputs %d (2: condition and y_t)", (int)na.number("num_inputs", 0));
  for (const char* k : {"downconv_kernel_size", "upconv_kernel_size", "bottleneck_kernel_size"})
    if ((int)na.number(k, 0) != 5) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 %s %d (5)", k, (int)na.number(k, 0));
  if ((int)na.number("conv_stride", 0) != 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 conv_stride %d (1)", (int)na.number("conv_stride", 0));
  if (na.string("conv_type", "") != "gn") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 conv_type '%s' ('gn')", na.string("conv_type", "").c_str());
  if ((int)na.number("depth", 1) != 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 depth %d (1)", (int)na.number("depth", 1));
  for (const char* k : {"downsample_kernel_size", "upsample_kernel_size"})
    if ((int)na.number(k, 4) != 4) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 %s %d (4)", k, (int)na.number(k, 4));
  if ((int)na.number("resample_stride", 2) != 2) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Waveunet2 resample_stride %d (2)", (int)na.number("resample_stride", 2));
  return SDDM_OK;
}

// refuses everything the layer table is not built for (the arguments of config_waveunet.json are)
static int wu1_check_config(const Json& na) {
  std::vector<int> want;
  for (int i = 0; i < wu2::kLevels1; ++i) want.push_back(wu2::ch(i));
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

namespace wu2 {
// waveunet2.py keeps the resampling convs under .down / .up, waveunet.py:335, 278 directly under
// downconv / upconv
static const Net kNets[] = {{"Waveunet2", kLevels2, "downconv.down.", "upconv.up.", sddm::launch_wu2_conv, wu2_check_config},
                            {"Waveunet", kLevels1, "downconv.", "upconv.", sddm::launch_wu1_conv, wu1_check_config}};
inline const Net* find_net(const std::string& type) {
  for (const Net& n : kNets)
    if (type == n.name) return &n;
  return nullptr;
}
}  // namespace wu2

// state-dict shapes (waveunet2.py:245-266, waveunet.py:379-394) without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> wu2_param_shapes(const WUFilmState& d) {
  std::map<std::string, std::vector<int64_t>> s;
  for (const wu2::Layer& l : d.net) {
    const int k = wu2::taps(l.mode);
    if (l.mode == sddm::WU_UP4) s[l.p + "filter.weight"] = {l.ci, l.co, k};   // ConvTranspose1d: [ci][co][k]
    else s[l.p + "filter.weight"] = {l.co, l.ci, k};
    s[l.p + "filter.bias"] = {l.co};
    s[l.p + "norm.weight"] = {l.co}; s[l.p + "norm.bias"] = {l.co};
  }
  for (int i = 0; i < d.desc.levels - 1; ++i) {
    const int c = wu2::ch(i);
    s[wu2::film(i) + "input_conv.weight"] = {c, c, 3}; s[wu2::film(i) + "input_conv.bias"] = {c};
    s[wu2::film(i) + "output_conv.weight"] = {2 * c, c, 3}; s[wu2::film(i) + "output_conv.bias"] = {2 * c};
  }
  s["waveunet.output_conv.weight"] = {1, wu2::ch(0), 1};
  s["waveunet.output_conv.bias"] = {1};
  return s;
}

size_t WUFilmState::pack(sddm_ctx* c, WeightPacker& pk) {
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  for (const wu2::Layer& l : net) {
    if (l.ci == 2) pk.f32(l.p + "w", P(l.p + "filter.weight"));                  // stem: fp32 [24][2][5], VALU kernel
    else wu_add_conv(c, pk, l.p + "w", l.co, l.ci, wu2::taps(l.mode), P(l.p + "filter.weight"), l.mode == sddm::WU_UP4);
    pk.f32(l.p + "b", P(l.p + "filter.bias"));
    pk.f32(l.p + "g", P(l.p + "norm.weight"));
    pk.f32(l.p + "e", P(l.p + "norm.bias"));
  }
  for (int i = 0; i < desc.levels - 1; ++i) {
    const std::string f = wu2::film(i);
    wu_add_conv(c, pk, f + "iw", wu2::ch(i), wu2::ch(i), 3, P(f + "input_conv.weight"), false);
    pk.f32(f + "ib", P(f + "input_conv.bias"));
    wu_add_conv(c, pk, f + "ow", 2 * wu2::ch(i), wu2::ch(i), 3, P(f + "output_conv.weight"), false);
    pk.f32(f + "ob", P(f + "output_conv.bias"));
  }
  pk.f32("out.w", P("waveunet.output_conv.weight"));
  pk.f32("out.b", P("waveunet.output_conv.bias"));
  return 0;                                            // no table of its own: the level is one scalar per t
}

// activation buffers for (B, N): name -> [B][len][C] in the compute dtype
int WUFilmState::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  WUFilmState& d = *this;
  TRY(wu_check_shape(desc.name, B, N, desc.levels - 1));
  if (d.B == B && d.N == N) return SDDM_OK;
  const size_t es = dtype_size(c->dtype);
  Arena& A = d.act;
  A.reset();
  d.aoff.clear();
  auto buf = [&](const std::string& n, int64_t len, int C) { d.aoff[n] = A.reserve(es * (size_t)B * len * C); };
  // statistics partials of the latest producer, [slots][C][2] per row: stem 8 slots per 256
  // positions, convs 4 per 128
  size_t max_cells = (size_t)8 * ((N + kWuStemTile - 1) / kWuStemTile) * wu2::ch(0);
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
  const int max_c = wu2::ch(desc.levels - 1);
  d.aoff["scale"] = A.reserve(sizeof(float) * (size_t)B * max_c);
  d.aoff["shift"] = A.reserve(sizeof(float) * (size_t)B * max_c);
  d.aoff["eps"] = A.reserve(sizeof(float) * (size_t)B * N);
  SDDM_HIP_CHECK(A.commit());
  d.B = (int)B;
  d.N = N;
  return SDDM_OK;
}

// the noise level the FiLM encodings take: sqrt_alpha_bar[t] or t of the step counter (sampling,
// model.py:84-89) or the caller's [B] (a forward).  No launch
int WUFilmState::begin(sddm_ctx* c, const float*, const float* noise_level, hipStream_t) {
  lv = wu_begin_level(c, noise_level, off_sp);
  return SDDM_OK;
}

// one forward (waveunet2.py:293-324, waveunet.py:475-506): cond, x_t [B][N] fp32 ->
// clamp(output_conv) = eps [B][N] fp32 (aoff "eps")
int WUFilmState::network(sddm_ctx* c, const float* cond, const float* x_t, int, int* t_dev, hipStream_t s) {
  WUFilmState& d = *this;
  const Arena& W = c->warena;
  const int B = d.B;
  const int dt = c->dtype;
  auto act = [&](const std::string& n) -> char* { return d.act.base + d.aoff.at(n); };
  auto wf = [&](const std::string& n) -> const float* { return W.at<float>(d.woff.at(n)); };
  float* stats = d.act.at<float>(d.aoff.at("stats"));
  float* scale = d.act.at<float>(d.aoff.at("scale"));
  float* shift = d.act.at<float>(d.aoff.at("shift"));
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
      TRY_LAUNCH("wu_conv ConvLayer", desc.conv(dt, a, s));
      slots = wu_conv_slots((int)lout);
    }
    len = lout;
    x = out;
    WUGnArgs g{stats, slots, l.co, l.co / 8, len, wf(l.p + "g"), wf(l.p + "e"), 1e-5f, scale, shift, B};
    TRY_LAUNCH("wu_gn_finalize", launch_wu_gn_finalize(g, s));
    if (l.film >= 0) {                                 // FiLM of the shortcut (waveunet2.py:56-61, waveunet.py:56-61)
      const std::string f = wu2::film(l.film), n = std::to_string(l.film);
      WU2ConvArgs a{};
      a.mode = WU_CONV3; a.src = x; a.Lin = (int)len; a.Cin = l.co; a.scale = scale; a.shift = shift;
      a.w = W.base + d.woff.at(f + "iw"); a.bias = wf(f + "ib"); a.enc_dim = l.co; a.lv = lv;
      a.out = act("fi" + n); a.Lout = (int)len; a.Cout = l.co; a.B = B;
      TRY_LAUNCH("wu_conv FiLM input_conv", desc.conv(dt, a, s));
      WU2ConvArgs o{};
      o.mode = WU_CONV3; o.src = act("fi" + n); o.Lin = (int)len; o.Cin = l.co;
      o.w = W.base + d.woff.at(f + "ow"); o.bias = wf(f + "ob");
      o.out = act("fo" + n); o.Lout = (int)len; o.Cout = 2 * l.co; o.B = B;
      TRY_LAUNCH("wu_conv FiLM output_conv", desc.conv(dt, o, s));
    }
  }
  WU2HeadArgs ha{x, scale, shift, wf("out.w"), wf("out.b"), d.act.at<float>(d.aoff.at("eps")), B, (int)d.N};
  TRY_LAUNCH("wu2_head", launch_wu2_head(dt, ha, s));
  return SDDM_OK;
}
