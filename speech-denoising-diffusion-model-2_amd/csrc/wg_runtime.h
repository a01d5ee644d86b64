// WaveGrad-family path of the runtime (included by sddm_runtime.cpp after sddm_ctx and SeqNet):
// weight packing, workspace and forward of three networks of reference model/wavegrad.py as one
// SeqNet, described by one table each (wg::Variant) and run by the same kernels (wavegrad.hip);
// seq_sample runs the reverse loop over them:
//
//   WaveGrad          (wavegrad.py:140-179) under SDDM_spectrogram.infer (model.py:212-257)
//   DenoiseWaveGrad1  (wavegrad.py:184-242) under SDDM.infer (model.py:50-124), waveform condition
//   DenoiseWaveGrad3  (wavegrad.py:307-353) under SDDM.infer, waveform condition
//
// WaveGrad.  The reference wiring of SDDM_spectrogram + WaveGrad fails (x_t [B,1,N]
// reaches a Conv1d as 4-D, and the squeezed [B,N] output broadcasts against x_t); the library
// applies the adapter: audio = x_t[:, 0], noise level [B], eps -> [B,1,N].
// Step-invariant per sampling call (the spectrogram does not change across steps): the spectrogram
// transpose, first_conv, and upsample.0's block1 and block2[0] (no FiLM reaches them).  The
// PositionalEncoding rows of all t are one launch.  Per reverse step: downsample.0, 5 FiLMs
// (2 convs each), 4 DBlocks (4 convs), upsample.0 (3 convs), upsample.1-4 (5 convs), last_conv,
// transition -- 52 launches.
//
// DenoiseWaveGrad1.  The condition is constant across steps, so the whole downsample_x encoder
// (stem + 5 DBlocks, 21 launches) and upsample.0's block1 / block2[0] run once per sampling call;
// the per-step launches are WaveGrad's 52 (y_t branch, FiLMs, the rest of the UBlocks, last_conv,
// transition).
//
// DenoiseWaveGrad3.  cat([y_t, x]) feeds downsample.0, so nothing hoists: per step the two-source
// stem, 4 DBlocks, 5 FiLMs, the bottleneck DBlock (4 convs), all five UBlocks in full (5 convs
// each), last_conv, transition -- 58 launches.
#pragma once
#include "wg_kernels.h"

namespace wg {
struct Down { int ci, co, f; };
struct Film { int ci, co; };
struct Up { int ci, h, f; int dil[4]; };
enum { kWaveGrad = 0, kDenoise1 = 1, kDenoise3 = 2 };
// One network of the family.  `bottom` is the extra DBlock whose output feeds upsample.0
// (downsample_x.5 of DenoiseWaveGrad1, bottleneck of DenoiseWaveGrad3; f = 0: none, WaveGrad's
// upsample.0 reads first_conv(spectrogram)).  `hoist`: upsample.0's input does not depend on the
// step, so it and upsample.0's block1 / block2[0] are computed once per sampling call.
struct Variant {
  int kind; const char* name; int hop; int stem_ci;
  Down down[5]; Film film[5]; Up up[5];
  int enc_off[5]; int enc_n;
  Down bottom; const char* bottom_key; bool hoist;
};
static const Variant kVariants[3] = {
    {kWaveGrad, "WaveGrad", 300, 1,                                                                 // 5 * 5 * 3 * 2 * 2
     {{1, 32, 1}, {32, 128, 2}, {128, 128, 2}, {128, 256, 3}, {256, 512, 5}},                        // wavegrad.py:143-149
     {{32, 128}, {128, 128}, {128, 256}, {256, 512}, {512, 512}},                                    // wavegrad.py:150-156
     {{768, 512, 5, {1, 2, 1, 2}}, {512, 512, 5, {1, 2, 1, 2}}, {512, 256, 3, {1, 2, 4, 8}},
      {256, 128, 2, {1, 2, 4, 8}}, {128, 128, 2, {1, 2, 4, 8}}},                                     // wavegrad.py:157-163
     {0, 32, 160, 288, 544}, 1056,                                                                   // 32 + 128 + 128 + 256 + 512
     {0, 0, 0}, "", true},
    {kDenoise1, "DenoiseWaveGrad1", 400, 1,                                                         // 5 * 5 * 4 * 2 * 2
     {{1, 32, 1}, {32, 128, 2}, {128, 128, 2}, {128, 256, 4}, {256, 512, 5}},                        // wavegrad.py:191-198
     {{32, 128}, {128, 128}, {128, 256}, {256, 512}, {512, 512}},                                    // wavegrad.py:210-216
     {{512, 512, 5, {1, 2, 1, 2}}, {512, 512, 5, {1, 2, 1, 2}}, {512, 256, 4, {1, 2, 4, 8}},
      {256, 128, 2, {1, 2, 4, 8}}, {128, 128, 2, {1, 2, 4, 8}}},                                     // wavegrad.py:217-223
     {0, 32, 160, 288, 544}, 1056,
     {512, 512, 5}, "downsample_x.5.", true},                                                        // wavegrad.py:207
    {kDenoise3, "DenoiseWaveGrad3", 300, 2,                                                         // 5 * 5 * 3 * 2 * 2
     {{2, 32, 1}, {32, 128, 2}, {128, 128, 2}, {128, 256, 3}, {256, 512, 5}},                        // wavegrad.py:314-321
     {{32, 128}, {128, 128}, {128, 256}, {256, 512}, {512, 512}},                                    // wavegrad.py:325-331
     {{512, 512, 5, {1, 2, 1, 2}}, {512, 512, 5, {1, 2, 1, 2}}, {512, 256, 3, {1, 2, 4, 8}},
      {256, 128, 2, {1, 2, 4, 8}}, {128, 128, 2, {1, 2, 4, 8}}},                                     // wavegrad.py:332-338
     {0, 32, 160, 288, 544}, 1056,
     {512, 512, 5}, "bottleneck.", false},                                                           // wavegrad.py:323
};
static const Variant* find_variant(const std::string& name) {
  for (const Variant& v : kVariants)
    if (name == v.name) return &v;
  return nullptr;
}
}  // namespace wg

struct WGConvSpec;
struct WGState : SeqNet {                             // shapes: wg_param_shapes of the variant
  static constexpr int kSpecC = 128;                  // WaveGrad's first_conv input channels
  const wg::Variant* v = &wg::kVariants[0];           // the context's network (set by sddm_configure)
  std::map<std::string, size_t> aoff;                 // activation buffers in act
  int F = -1;                                         // bottom positions of the current (B, N): N = hop F
  const float* enc = nullptr;                         // the encoding rows of the current call (begin)
  size_t pack(sddm_ctx* c, WeightPacker& pk) override;
  int prepare(sddm_ctx* c, int64_t B, int64_t N) override;
  int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) override;
  int network(sddm_ctx* c, const float* cond, const float* audio, int enc_per_b, int* t_dev, hipStream_t s) override;
  float* eps() override { return act.at<float>(aoff.at("eps")); }
  int conv(sddm_ctx* c, WGConvSpec q, int B, const float* enc, int enc_per_b, const int* t_dev, hipStream_t s);
  int dblock(sddm_ctx* c, const std::string& p, const char* xs, int64_t lin, const wg::Down& dn, int64_t lout,
             const std::string& o, const char* out, int B, hipStream_t s);
  int up0_head(sddm_ctx* c, int B, const int64_t* L, hipStream_t s);
};

// state-dict shapes of a variant (wavegrad.py:140-165, 189-224, 312-339) without the
// noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> wg_param_shapes(const wg::Variant& v) {
  std::map<std::string, std::vector<int64_t>> s;
  auto conv = [&](const std::string& p, int co, int ci, int k) {
    s[p + ".weight"] = {co, ci, k};
    s[p + ".bias"] = {co};
  };
  auto dblock = [&](const std::string& p, const wg::Down& d) {
    conv(p + "residual_dense", d.co, d.ci, 1);
    conv(p + "conv.0", d.co, d.ci, 3);
    conv(p + "conv.1", d.co, d.co, 3);
    conv(p + "conv.2", d.co, d.co, 3);
  };
  conv("downsample.0", 32, v.stem_ci, 5);
  for (int i = 1; i < 5; ++i) dblock("downsample." + std::to_string(i) + ".", v.down[i]);
  if (v.kind == wg::kDenoise1) {                     // downsample_x: the same ladder plus the bottom DBlock
    conv("downsample_x.0", 32, 1, 5);
    for (int i = 1; i < 5; ++i) dblock("downsample_x." + std::to_string(i) + ".", v.down[i]);
  }
  if (v.bottom.f) dblock(v.bottom_key, v.bottom);
  for (int i = 0; i < 5; ++i) {
    const std::string p = "film." + std::to_string(i) + ".";
    conv(p + "input_conv", v.film[i].ci, v.film[i].ci, 3);
    conv(p + "output_conv", 2 * v.film[i].co, v.film[i].ci, 3);
  }
  for (int i = 0; i < 5; ++i) {
    const wg::Up& u = v.up[i];
    const std::string p = "upsample." + std::to_string(i) + ".";
    conv(p + "block1", u.h, u.ci, 1);
    conv(p + "block2.0", u.h, u.ci, 3);
    conv(p + "block2.1", u.h, u.h, 3);
    conv(p + "block3.0", u.h, u.h, 3);
    conv(p + "block3.1", u.h, u.h, 3);
  }
  if (v.kind == wg::kWaveGrad) conv("first_conv", v.up[0].ci, WGState::kSpecC, 3);
  conv("last_conv", 1, v.up[4].h, 3);
  return s;
}

size_t WGState::pack(sddm_ctx* c, WeightPacker& pk) {
  const WGState& d = *this;
  const int dt = c->dtype;
  const size_t es = dtype_size(dt);
  auto add_f32 = [&](const std::string& name, const std::vector<float>& v) { pk.f32(name, v); };
  // Conv1d weight [Cout][Cin][K] -> [Cout_pad64][K][Cin] in the compute dtype (zero pad rows)
  const wg::Variant& v = *d.v;
  for (const auto& kv : d.shapes) {
    const std::string& key = kv.first;
    if (key.size() < 7 || key.compare(key.size() - 7, 7, ".weight")) continue;
    const std::string base = key.substr(0, key.size() - 7);
    const std::vector<float>& w = c->params.at(key).data;
    const int co = (int)kv.second[0], ci = (int)kv.second[1], k = (int)kv.second[2];
    add_f32(base + ".b", c->params.at(base + ".bias").data);
    if (base == "downsample.0" || base == "downsample_x.0") { add_f32(base + ".w", w); continue; }   // fp32 [32][1 | 2][5], VALU kernels
    const int cop = (co + 63) / 64 * 64;
    char* b = pk.raw(base + ".w", (size_t)cop * k * ci * es);
    for (int o = 0; o < co; ++o)
      for (int i = 0; i < ci; ++i)
        for (int t = 0; t < k; ++t) store_elem(b, ((size_t)o * k + t) * ci + i, w[((size_t)o * ci + i) * k + t], dt);
  }
  {  // PositionalEncoding exp vectors, torch fp32 op order (wavegrad.py:45-47)
    std::vector<float> ev;
    for (int i = 0; i < 5; ++i) {
      const int cnt = v.film[i].ci / 2;
      for (int k = 0; k < cnt; ++k) {
        const float step = (float)k / (float)cnt;
        ev.push_back(std::exp((float)(-std::log(1e4)) * step));
      }
    }
    add_f32("enc.ev", ev);
  }
  return sizeof(float) * (size_t)(c->T + 1) * v.enc_n;   // every t's encoding rows
}

// lengths of the levels for F bottom positions: L[0] = hop F samples .. L[4]; L[5] = F (upsample.0's input)
static void wg_lengths(const wg::Variant& v, int F, int64_t* L) {
  L[0] = (int64_t)v.hop * F;
  for (int i = 1; i < 5; ++i) L[i] = L[i - 1] / v.down[i].f;
  L[5] = F;
}

// activation buffers for (B, N): name -> [B][len][C] in the compute dtype
int WGState::prepare(sddm_ctx* c, int64_t B, int64_t N) {
  WGState& d = *this;
  const wg::Variant& v = *d.v;
  if (B < 1 || B > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)B);
  if (c->hop_samples != v.hop)
    FAIL(SDDM_ERR_SHAPE, "hop_samples %d: %s resamples x%d (wavegrad.py:157-163, 217-223, 332-338)", c->hop_samples, v.name, v.hop);
  if (N < v.hop || N % v.hop)
    FAIL(SDDM_ERR_SHAPE, "%lld samples is not a positive multiple of %s's hop (%d)", (long long)N, v.name, v.hop);
  if (d.B == B && d.N == N) return SDDM_OK;
  const int F = (int)(N / v.hop);
  const size_t es = dtype_size(c->dtype);
  Arena& A = d.act;
  A.reset();
  d.aoff.clear();
  auto buf = [&](const std::string& n, int64_t len, int C) { d.aoff[n] = A.reserve(es * (size_t)B * len * C); };
  int64_t L[6];
  wg_lengths(v, F, L);
  buf("d0", L[0], 32);
  for (int i = 0; i < 5; ++i) {
    const std::string s = std::to_string(i);
    if (i > 0) for (const char* n : {"r", "a", "b", ""}) buf("d" + s + n, L[i], v.down[i].co);
    buf("f" + s + "a", L[i], v.film[i].ci);
    buf("f" + s, L[i], 2 * v.film[i].co);
  }
  if (v.kind == wg::kWaveGrad) buf("spec", L[5], WGState::kSpecC);
  if (v.bottom.f) for (const char* n : {"r", "a", "b"}) buf(std::string("bn") + n, L[5], v.bottom.co);   // bottom DBlock scratch
  buf("uin", L[5], v.up[0].ci);
  for (int i = 0; i < 5; ++i) {
    const std::string s = std::to_string(i);
    const int64_t lin = L[5 - i], lout = L[4 - i];
    buf("u" + s + "b1", lin, v.up[i].h);
    for (const char* n : {"y0", "x", "z", "", "m", "p"}) buf("u" + s + n, lout, v.up[i].h);   // m: leaky(film(x)); p: pre-2 fallback scratch
  }
  d.aoff["eps"] = A.reserve(sizeof(float) * (size_t)B * L[0]);
  d.aoff["encb"] = A.reserve(sizeof(float) * (size_t)B * v.enc_n);
  SDDM_HIP_CHECK(A.commit());
  d.B = (int)B;
  d.N = N;
  d.F = F;
  return SDDM_OK;
}

struct WGConvSpec {
  const char* src; int64_t src_T; int src_C; int map, f; int64_t Tc; int Cin;
  std::string w; int Cout, K, dil, pre; const char* film;
  int post, enc_off; const char* res; int res_map, res_f; int64_t res_T;
  const char* out;
  const char* efilm = nullptr; int post_film = 0; const char* out2 = nullptr;   // WGConvArgs::post_film
};

int WGState::conv(sddm_ctx* c, WGConvSpec q, int B, const float* enc, int enc_per_b, const int* t_dev, hipStream_t s) {
  WGState& d = *this;
  const Arena& W = c->warena;
  std::string mod;
  WGConvArgs probe{};
  probe.Cout = q.Cout; probe.K = q.K; probe.dil = q.dil; probe.pre = q.pre; probe.out_f32 = 0;
  if (q.pre == 2 && !wg_conv_uses_lds(probe)) {   // modulate once into the UBlock's scratch, then a plain conv
    mod = std::string(q.out).substr(0, 2) + "p";
    WGFilmArgs fa{d.act.base + d.aoff.at(q.src), d.act.base + d.aoff.at(q.film), d.act.base + d.aoff.at(mod),
                  (int64_t)B * q.Tc, q.Cin};
    SDDM_HIP_CHECK(launch_wg_film(c->dtype, fa, s));
    q.src = mod.c_str();
    q.pre = 0;
    q.film = nullptr;
  }
  WGConvArgs a{};
  a.src = d.act.base + d.aoff.at(q.src); a.src_T = (int)q.src_T; a.src_C = q.src_C; a.map = q.map; a.f = q.f;
  a.Tc = (int)q.Tc; a.Cin = q.Cin; a.K = q.K; a.dil = q.dil; a.pre = q.pre;
  a.film = q.film ? d.act.base + d.aoff.at(q.film) : nullptr;
  a.w = W.base + d.woff.at(q.w + ".w"); a.bias = W.at<float>(d.woff.at(q.w + ".b")); a.Cout = q.Cout;
  a.post = q.post; a.enc = enc; a.enc_stride = d.v->enc_n; a.enc_off = q.enc_off; a.enc_per_b = enc_per_b;
  a.t_dev = t_dev;
  a.res = q.res ? d.act.base + d.aoff.at(q.res) : nullptr; a.res_map = q.res_map; a.res_f = q.res_f;
  a.res_T = (int)q.res_T;
  a.out = d.act.base + d.aoff.at(q.out); a.out_f32 = std::strcmp(q.out, "eps") == 0;
  a.B = B;
  a.post_film = q.post_film;
  a.efilm = q.efilm ? d.act.base + d.aoff.at(q.efilm) : nullptr;
  a.out2 = q.out2 ? d.act.base + d.aoff.at(q.out2) : nullptr;
  TRY_LAUNCH(("wg_conv " + q.w).c_str(), launch_wg_conv(c->dtype, a, s));
  return SDDM_OK;
}

// DBlock (wavegrad.py:126-137): weights p + {residual_dense, conv.0-2}, input xs [B][lin][dn.ci] ->
// out [B][lout][dn.co]; scratch buffers o + {r, a, b}
int WGState::dblock(sddm_ctx* c, const std::string& p, const char* xs, int64_t lin, const wg::Down& dn, int64_t lout,
                    const std::string& o, const char* out, int B, hipStream_t s) {
  TRY(conv(c, {xs, lin, dn.ci, WG_MAP_DOWN, dn.f, lout, dn.ci, p + "residual_dense", dn.co, 1, 1, 0, nullptr, 0, 0,
               nullptr, 0, 1, 0, (o + "r").c_str()}, B, nullptr, 0, nullptr, s));
  TRY(conv(c, {xs, lin, dn.ci, WG_MAP_DOWN, dn.f, lout, dn.ci, p + "conv.0", dn.co, 3, 1, 1, nullptr, 0, 0,
               nullptr, 0, 1, 0, (o + "a").c_str()}, B, nullptr, 0, nullptr, s));
  TRY(conv(c, {(o + "a").c_str(), lout, dn.co, WG_MAP_ID, 1, lout, dn.co, p + "conv.1", dn.co, 3, 2, 1, nullptr, 0, 0,
               nullptr, 0, 1, 0, (o + "b").c_str()}, B, nullptr, 0, nullptr, s));
  TRY(conv(c, {(o + "b").c_str(), lout, dn.co, WG_MAP_ID, 1, lout, dn.co, p + "conv.2", dn.co, 3, 4, 1, nullptr, 0, 0,
               (o + "r").c_str(), WG_MAP_ID, 1, lout, out}, B, nullptr, 0, nullptr, s));
  return SDDM_OK;
}

// upsample.0's block1 / block2[0] from "uin" (wavegrad.py:92-97): no FiLM reaches them
int WGState::up0_head(sddm_ctx* c, int B, const int64_t* L, hipStream_t s) {
  const wg::Up& u = v->up[0];
  TRY(conv(c, {"uin", L[5], u.ci, WG_MAP_ID, 1, L[5], u.ci, "upsample.0.block1", u.h, 1, 1, 0, nullptr, 0, 0, nullptr, 0, 1, 0, "u0b1"},
           B, nullptr, 0, nullptr, s));
  TRY(conv(c, {"uin", L[5], u.ci, WG_MAP_UP, u.f, L[4], u.ci, "upsample.0.block2.0", u.h, 3, u.dil[0], 1, nullptr, 0, 0,
               nullptr, 0, 1, 0, "u0y0"}, B, nullptr, 0, nullptr, s));
  return SDDM_OK;
}

// step-invariant work of one call.  All: the PositionalEncoding rows, of every t (sampling) or one
// per batch item (a forward).  WaveGrad: cond = spectrogram [B][128][F] -> first_conv
// (wavegrad.py:175).  DenoiseWaveGrad1: cond = waveform [B][N] -> downsample_x (wavegrad.py:234-236;
// its levels 1-4 borrow the y_t branch's buffers, which the steps overwrite afterwards).  Both then
// run upsample.0's block1 / block2[0].  DenoiseWaveGrad3 has no more step-invariant work
int WGState::begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) {
  WGState& d = *this;
  const wg::Variant& v = *d.v;
  float* rows = noise_level ? d.act.at<float>(d.aoff.at("encb")) : c->warena.at<float>(d.off_rows);
  WGEncArgs e{};
  e.noise_levels = noise_level; e.table = c->dtab(3);
  e.time_step_mode = c->noise_time_step; e.R = noise_level ? d.B : c->T + 1;
  e.ev = c->warena.at<float>(d.woff.at("enc.ev")); e.stride = v.enc_n; e.n = v.enc_n;
  for (int i = 0; i < 5; ++i) { e.dims[i] = v.film[i].ci; e.offs[i] = v.enc_off[i]; }
  e.out = rows;
  SDDM_HIP_CHECK(launch_wg_enc(e, s));
  d.enc = rows;
  if (!v.hoist) return SDDM_OK;
  const int B = d.B, F = d.F;
  int64_t L[6];
  wg_lengths(v, F, L);
  if (v.kind == wg::kWaveGrad) {
    WGSpecArgs sa{cond, d.act.base + d.aoff.at("spec"), B, WGState::kSpecC, F};
    SDDM_HIP_CHECK(launch_wg_spec(c->dtype, sa, s));
    TRY(conv(c, {"spec", L[5], 128, WG_MAP_ID, 1, L[5], 128, "first_conv", v.up[0].ci, 3, 1, 0, nullptr, 0, 0, nullptr, 0, 1, 0, "uin"},
             B, nullptr, 0, nullptr, s));
  } else {
    const Arena& W = c->warena;
    WGFirstArgs fa{cond, W.at<float>(d.woff.at("downsample_x.0.w")), W.at<float>(d.woff.at("downsample_x.0.b")),
                   d.act.base + d.aoff.at("d0"), B, (int)L[0], nullptr};
    SDDM_HIP_CHECK(launch_wg_first(c->dtype, fa, s));
    std::string x = "d0";
    for (int i = 1; i < 5; ++i) {
      const std::string si = std::to_string(i), o = "d" + si;
      TRY(dblock(c, "downsample_x." + si + ".", x.c_str(), L[i - 1], v.down[i], L[i], o, o.c_str(), B, s));
      x = o;
    }
    TRY(dblock(c, v.bottom_key, x.c_str(), L[4], v.bottom, L[5], "bn", "uin", B, s));
  }
  return up0_head(c, B, L, s);
}

// one forward of the y_t branch and the decoder (wavegrad.py:167-179, 226-242, 341-353): audio
// [B][N] fp32 (and, for DenoiseWaveGrad3, the condition waveform [B][N]) -> eps [B][N] fp32 (aoff "eps")
int WGState::network(sddm_ctx* c, const float* cond, const float* audio, int enc_per_b, int* t_dev, hipStream_t s) {
  WGState& d = *this;
  const wg::Variant& v = *d.v;
  const int B = d.B, F = d.F;
  const Arena& W = c->warena;
  int64_t L[6];
  wg_lengths(v, F, L);
  if (v.stem_ci == 2) {                                  // cat([y_t, x]) (wavegrad.py:343)
    WGFirst2Args fa{audio, cond, W.at<float>(d.woff.at("downsample.0.w")), W.at<float>(d.woff.at("downsample.0.b")),
                    d.act.base + d.aoff.at("d0"), B, (int)L[0], t_dev};
    SDDM_HIP_CHECK(launch_wg_first2(c->dtype, fa, s));
  } else {
    WGFirstArgs fa{audio, W.at<float>(d.woff.at("downsample.0.w")), W.at<float>(d.woff.at("downsample.0.b")),
                   d.act.base + d.aoff.at("d0"), B, (int)L[0], t_dev};
    SDDM_HIP_CHECK(launch_wg_first(c->dtype, fa, s));
  }
  std::string x = "d0";
  for (int i = 0; i < 5; ++i) {
    const std::string si = std::to_string(i);
    if (i > 0) {
      const std::string o = "d" + si;
      TRY(dblock(c, "downsample." + si + ".", x.c_str(), L[i - 1], v.down[i], L[i], o, o.c_str(), B, s));
      x = o;
    }
    const wg::Film& fm = v.film[i];                      // FiLM (wavegrad.py:66-71)
    const std::string p = "film." + si + ".", o = "f" + si;
    TRY(conv(c, {x.c_str(), L[i], fm.ci, WG_MAP_ID, 1, L[i], fm.ci, p + "input_conv", fm.ci, 3, 1, 0, nullptr, 1,
                 v.enc_off[i], nullptr, 0, 1, 0, (o + "a").c_str()}, B, enc, enc_per_b, t_dev, s));
    TRY(conv(c, {(o + "a").c_str(), L[i], fm.ci, WG_MAP_ID, 1, L[i], fm.ci, p + "output_conv", 2 * fm.co, 3, 1, 0, nullptr,
                 0, 0, nullptr, 0, 1, 0, o.c_str()}, B, enc, enc_per_b, t_dev, s));
  }
  if (!v.hoist) {                                        // bottleneck (wavegrad.py:349), then upsample.0 in full
    TRY(dblock(c, v.bottom_key, x.c_str(), L[4], v.bottom, L[5], "bn", "uin", B, s));
  }
  x = "uin";
  for (int i = 0; i < 5; ++i) {                           // UBlock (wavegrad.py:91-112)
    const wg::Up& u = v.up[i];
    const std::string si = std::to_string(i), p = "upsample." + si + ".", o = "u" + si;
    const std::string film = "f" + std::to_string(4 - i);
    const int64_t lin = L[5 - i], lout = L[4 - i];
    // FiLM placement.  512-channel UBlocks (upsample.0-1): the FiLM of block2.1 / block3.0 /
    // block3.1's inputs runs in their producers' epilogues (post_film: y0 holds leaky(film(block2.0
    // out)), m holds leaky(film(x)), z holds leaky(film(block3.0 out))), so shift / scale are read
    // once per element instead of once per 128-channel block of the consumer (upsample.1: 1137 ->
    // 962 us per step at B=64).  Where upsample.0's block2.0 is step-invariant (begin: WaveGrad,
    // DenoiseWaveGrad1), its block2.1 keeps the FiLM in the staging (pre 2).  The 128 / 256-channel UBlocks keep the
    // staged FiLM: there the epilogue loads are exposed (all blocks reach their epilogues
    // together) and cost more than the re-reads save (upsample.4: 1324 -> 1675 us)
    const std::string ym = o + "y0", xm = o + "m", xo = o + "x", zo = o + "z", b1 = o + "b1";
    static const int epi_min_h = std::getenv("SDDM_WG_EPI_MIN_H") ? std::atoi(std::getenv("SDDM_WG_EPI_MIN_H")) : 512;
    const bool epi = u.h >= epi_min_h;
    const bool head_done = i == 0 && v.hoist;            // begin ran block1 / block2[0] (plain, no epilogue FiLM)
    if (!head_done) {
      TRY(conv(c, {x.c_str(), lin, u.ci, WG_MAP_ID, 1, lin, u.ci, p + "block1", u.h, 1, 1, 0, nullptr, 0, 0, nullptr, 0, 1, 0,
                   b1.c_str()}, B, enc, enc_per_b, t_dev, s));
      TRY(conv(c, {x.c_str(), lin, u.ci, WG_MAP_UP, u.f, lout, u.ci, p + "block2.0", u.h, 3, u.dil[0], 1, nullptr, 0, 0,
                   nullptr, 0, 1, 0, ym.c_str(), epi ? film.c_str() : nullptr, epi ? 1 : 0}, B, enc, enc_per_b, t_dev, s));
    }
    const bool pre21 = !epi || head_done;
    TRY(conv(c, {ym.c_str(), lout, u.h, WG_MAP_ID, 1, lout, u.h, p + "block2.1", u.h, 3, u.dil[1], pre21 ? 2 : 0,
                 pre21 ? film.c_str() : nullptr, 0, 0, b1.c_str(), WG_MAP_UP, u.f, lin, xo.c_str(),
                 epi ? film.c_str() : nullptr, epi ? 2 : 0, epi ? xm.c_str() : nullptr}, B, enc, enc_per_b, t_dev, s));
    TRY(conv(c, {epi ? xm.c_str() : xo.c_str(), lout, u.h, WG_MAP_ID, 1, lout, u.h, p + "block3.0", u.h, 3, u.dil[2],
                 epi ? 0 : 2, epi ? nullptr : film.c_str(), 0, 0, nullptr, 0, 1, 0, zo.c_str(), epi ? film.c_str() : nullptr,
                 epi ? 1 : 0}, B, enc, enc_per_b, t_dev, s));
    TRY(conv(c, {zo.c_str(), lout, u.h, WG_MAP_ID, 1, lout, u.h, p + "block3.1", u.h, 3, u.dil[3], epi ? 0 : 2,
                 epi ? nullptr : film.c_str(), 0, 0, xo.c_str(), WG_MAP_ID, 1, lout, o.c_str()}, B, enc, enc_per_b, t_dev, s));
    x = o;
  }
  const int cl = v.up[4].h;
  TRY(conv(c, {x.c_str(), L[0], cl, WG_MAP_ID, 1, L[0], cl, "last_conv", 1, 3, 1, 0, nullptr, 0, 0, nullptr, 0, 1, 0, "eps"},
           B, enc, enc_per_b, t_dev, s));
  return SDDM_OK;
}
