// UNetModified2 / UNetTST path of the runtime (included by sddm_runtime.cpp after sddm_ctx, Net and the
// weight packers): configuration check, weight packing, the per-batch plan of one reverse step and its
// run, of reference model/UNetModified2.py:146-269 and model/UNetTST.py:270-392 as a Net.  Unlike the
// sequential networks it runs in lanes whose step graphs replay concurrently.
// Kernels: kernels.hip (conv_in, final, embed, concat), conv_strip / conv_tile / conv_deep / conv_chain
// .hip (the 3x3 convs), dual_transformer.hip.
//
// Layers (channels inner * mult per level; F frames of segment_len positions, halved per level):
//   downs.0         conv_in: the frames of (cond, x_t) -> inner channels
//   downs           per level res_blocks ResnetBlocks, then Downsample (3x3, stride 2)
//   mid             ResnetBlock mid.0; UNetTST: Dual_Transformer(C, C, 0, n_TSTB) in its place
//   ups             per level ResnetBlock over cat(x, skip), Upsample (nearest x2, 3x3), then
//                   res_blocks ResnetBlocks over cat(x, skip)
//   final_conv      GroupNorm, Swish, 3x3 conv to one channel, overlap-add and the transition
// A ResnetBlock is two 3x3 convs; each conv applies the GroupNorm + Swish of its input as it loads it
// (the producer leaves per-tile statistics), block1 adds the noise embedding's projection, block2 the
// residual (the 1x1 res_conv where the channels change).
//
// Launches per reverse step at res_blocks 1 and five levels: conv_in 1, 11 ResnetBlocks x 2, 5
// Downsamples, 5 Upsamples, final 1 -- 44 for UNetModified2 (40 where a tuning table marks the
// bottom-level chain), 43 for UNetTST.  Where a GroupNorm group would straddle cat(x, skip)
// (res_blocks >= 2) one concat launch precedes the block.  The noise embeddings of every t are one
// launch per sampling call.
#pragma once
#include "kernels.h"
#include "dual_transformer.h"

// ---------------------------------------------------------------------------------------------
// UNetModified2 architecture (UNetModified2.py:146-235)
// ---------------------------------------------------------------------------------------------
struct UNetCfg {
  int in_channel = 2, out_channel = 1, inner = 32, groups = 32, res_blocks = 3;
  std::vector<int> mults{1, 2, 3, 4, 5};
  int seg = 128, stride = 64;
  double dropout = 0.0;
  int mid_tst = 0;   // 1: UNetTST -- mid is Dual_Transformer(C, C, 0, n_tstb) (UNetTST.py:324), and the
  int n_tstb = 6;    //    noise MLP has no final Swish (UNetTST.py:293-298)
};
struct LayerDesc { int kind; std::string name; int cin, cout; };  // kind 0 conv,1 res,2 down,3 up,4 final,5 dual transformer
static std::vector<LayerDesc> unet_layers(const UNetCfg& c, std::vector<LayerDesc>* downs_out,
                                          std::vector<LayerDesc>* mid_out, std::vector<LayerDesc>* ups_out) {
  std::vector<LayerDesc> downs, mid, ups;
  downs.push_back({0, "downs.0", c.in_channel, c.inner});
  std::vector<int> feat{c.inner};
  int cin = c.inner, idx = 1, cout = c.inner;
  for (size_t ind = 0; ind < c.mults.size(); ++ind) {
    cout = c.inner * c.mults[ind];
    for (int r = 0; r < c.res_blocks; ++r) {
      downs.push_back({1, "downs." + std::to_string(idx++), cin, cout});
      feat.push_back(cout);
      cin = cout;
    }
    downs.push_back({2, "downs." + std::to_string(idx++), cout, cout});
    feat.push_back(cout);
  }
  if (c.mid_tst) mid.push_back({5, "mid", cin, cin});
  else mid.push_back({1, "mid.0", cin, cin});
  idx = 0;
  for (int ind = (int)c.mults.size() - 1; ind >= 0; --ind) {
    cin = c.inner * c.mults[ind];
    cout = cin;
    ups.push_back({1, "ups." + std::to_string(idx++), cin + feat.back(), cout});
    feat.pop_back();
    ups.push_back({3, "ups." + std::to_string(idx++), cout, cout});
    cout = ind == 0 ? c.inner : c.inner * c.mults[ind - 1];
    for (int r = 0; r < c.res_blocks; ++r) {
      ups.push_back({1, "ups." + std::to_string(idx++), cin + feat.back(), cout});
      feat.pop_back();
      cin = cout;
    }
  }
  std::vector<LayerDesc> all;
  all.insert(all.end(), downs.begin(), downs.end());
  all.insert(all.end(), mid.begin(), mid.end());
  all.insert(all.end(), ups.begin(), ups.end());
  all.push_back({4, "final_conv", cout, c.out_channel});
  if (downs_out) *downs_out = downs;
  if (mid_out) *mid_out = mid;
  if (ups_out) *ups_out = ups;
  return all;
}

// the network's arguments (`na`; num_samples may also stand at the config's top level) -> `u` and the
// length the network is built for.  tst: UNetTST (UNetTST.py:270-392), i.e. UNetModified2 with mid =
// Dual_Transformer and no final Swish in the noise MLP
static int unet_configure(const Json& cfg, const Json& na, bool tst, UNetCfg& u, int* num_samples) {
  u.in_channel = (int)na.number("in_channel", 2);
  u.out_channel = (int)na.number("out_channel", 1);
  u.inner = (int)na.number("inner_channel", 32);
  u.groups = (int)na.number("norm_groups", 32);
  u.mults = na.ints("channel_mults", {1, 2, 3, 4, 5});
  u.res_blocks = (int)na.number("res_blocks", 3);
  u.dropout = na.number("dropout", 0.0);
  u.seg = (int)na.number("segment_len", 128);
  u.stride = (int)na.number("segment_stride", 64);
  const int Ns = (int)cfg.number("num_samples", (double)na.number("num_samples", -1));
  if (u.in_channel != 2 || u.out_channel != 1)
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "UNetModified2 with in_channel %d / out_channel %d", u.in_channel, u.out_channel);
  if (u.inner > 128 || u.inner % 32) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "inner_channel %d (multiples of 32 up to 128)", u.inner);
  if (Ns <= u.seg || (Ns - u.seg) % u.stride) FAIL(SDDM_ERR_SHAPE, "num_samples %d: (n - %d) %% %d != 0 (UNetModified2.py:13)", Ns, u.seg, u.stride);
  const int F = (Ns - u.seg) / u.stride + 1;
  const int div = 1 << (int)u.mults.size();
  if (F % div || u.seg % div) FAIL(SDDM_ERR_SHAPE, "n_frames %d and segment_len %d must be multiples of %d", F, u.seg, div);
  if (u.seg % u.stride) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "segment_len %% segment_stride != 0");
  if (tst) {   // everything the plan or the Dual_Transformer kernel would refuse later is refused here
    u.mid_tst = 1;
    u.n_tstb = (int)na.number("n_TSTB", 6);
    if (u.n_tstb < 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "n_TSTB %d: at least one transformer block", u.n_tstb);
    if (u.res_blocks < 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "res_blocks %d: at least one", u.res_blocks);
    if (u.inner != 32 || 512 % u.seg)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "inner_channel %d / segment_len %d: conv_in needs 32 and a divisor of 512", u.inner, u.seg);
    const int Cb = u.mults.empty() ? 0 : u.inner * u.mults.back();
    if (Cb != kTstC)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "channel_mults: the bottom level has %d channels, the Dual_Transformer kernel is built for %d",
           Cb, kTstC);
    if ((Cb / 2) % kTstHeads) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "channel_mults: %d heads do not divide d_model %d", kTstHeads, Cb / 2);
    if (u.groups < 1 || 256 % u.groups)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "norm_groups %d: the GroupNorm finalize needs a divisor of 256", u.groups);
    for (int m : u.mults)
      if (m < 1 || (u.inner * m) % u.groups)
        FAIL(SDDM_ERR_NOT_IMPLEMENTED, "channel_mults / norm_groups: %d channels in groups of %d", u.inner * m, u.groups);
    const int tok = (F / div) * (u.seg / div);
    if (tok > kTstMaxTokens)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "num_samples %d: the bottom level has %d x %d = %d tokens, the Dual_Transformer kernel holds %d",
           Ns, F / div, u.seg / div, tok, kTstMaxTokens);
  }
  *num_samples = Ns;
  return SDDM_OK;
}

// state-dict shapes without the noise_estimate_model. prefix
static std::map<std::string, std::vector<int64_t>> unet_param_shapes(const UNetCfg& c) {
  std::map<std::string, std::vector<int64_t>> s;
  const int64_t inner = c.inner;
  s["noise_level_mlp.1.weight"] = {inner * 4, inner};
  s["noise_level_mlp.1.bias"] = {inner * 4};
  s["noise_level_mlp.3.weight"] = {inner, inner * 4};
  s["noise_level_mlp.3.bias"] = {inner};
  for (const auto& L : unet_layers(c, nullptr, nullptr, nullptr)) {
    const std::string& n = L.name;
    if (L.kind == 1) {
      s[n + ".noise_func.noise_func.0.weight"] = {L.cout, inner};
      s[n + ".noise_func.noise_func.0.bias"] = {L.cout};
      s[n + ".block1.block.0.weight"] = {L.cin};
      s[n + ".block1.block.0.bias"] = {L.cin};
      s[n + ".block1.block.3.weight"] = {L.cout, L.cin, 3, 3};
      s[n + ".block1.block.3.bias"] = {L.cout};
      s[n + ".block2.block.0.weight"] = {L.cout};
      s[n + ".block2.block.0.bias"] = {L.cout};
      s[n + ".block2.block.3.weight"] = {L.cout, L.cout, 3, 3};
      s[n + ".block2.block.3.bias"] = {L.cout};
      if (L.cin != L.cout) {
        s[n + ".res_conv.weight"] = {L.cout, L.cin, 1, 1};
        s[n + ".res_conv.bias"] = {L.cout};
      }
    } else if (L.kind == 2 || L.kind == 3) {
      s[n + ".conv.weight"] = {L.cout, L.cin, 3, 3};
      s[n + ".conv.bias"] = {L.cout};
    } else if (L.kind == 0) {
      s[n + ".weight"] = {L.cout, L.cin, 3, 3};
      s[n + ".bias"] = {L.cout};
    } else if (L.kind == 5) {   // Dual_Transformer (UNetTST.py:184-210): one-element PReLUs
      dt_param_shapes(s, n, L.cin, c.n_tstb, kDtPreluShared);
    } else {
      s[n + ".block.0.weight"] = {L.cin};
      s[n + ".block.0.bias"] = {L.cin};
      s[n + ".block.3.weight"] = {L.cout, L.cin, 3, 3};
      s[n + ".block.3.bias"] = {L.cout};
    }
  }
  return s;
}

// ---------------------------------------------------------------------------------------------
// state: the packed weights and the plan, in lanes
// ---------------------------------------------------------------------------------------------
// an activation of the plan and its per-tile GroupNorm statistics; `off`, `st_off`: where in the lane's arena
struct Tensor { void* p = nullptr; int C = 0, H = 0, W = 0; float* stats = nullptr; int tiles = 0, n_tile = 0; size_t off = 0, st_off = 0; };

struct RunState {  // fields patched into the plan's kernel arguments at launch time
  const float* cond = nullptr;
  float* x = nullptr;
  const float* temb = nullptr;
  int temb_per_b = 0;
  int* t_dev = nullptr;
  int final_mode = 0;
  float* eps_out = nullptr;
  uint64_t seed = 0;
  int64_t row_offset = 0;
  const float* noise = nullptr;   // caller-supplied draws of this lane's rows (sddm_sample_noise), or null
  int64_t noise_ld = 0;
};

static constexpr int kStreams = 4;    // concurrent lane streams (GPU_MAX_HW_QUEUES is 4)
static constexpr int kMaxLanes = 64;  // step counters reserved in the weight arena

struct Lane {                         // one row block of the batch: plan + activations + graph
  int B = 0, row0 = 0, idx = 0;
  Arena arena;
  std::vector<Op> ops;
  RunState rs;
  size_t off_temb_fwd = 0, off_cond = 0, off_x = 0;
  hipGraphExec_t gexec = nullptr;
  hipGraph_t graph = nullptr;
  int g_K = 0, g_gen = -1;
  ~Lane() {
    if (gexec) (void)hipGraphExecDestroy(gexec);
    if (graph) (void)hipGraphDestroy(graph);
    arena.reset();
  }
};

struct UNetState : Net {
  UNetCfg u;
  std::map<std::string, size_t> woff;   // packed weight offsets in ctx->warena
  size_t off_tdev = 0, off_temb_tab = 0;  // the lanes' StepParams; the projected embeddings of every t
  int SC = 0;                            // length of the projection vector (the ResnetBlocks' channels, summed)
  std::map<std::string, int> temb_off;  // per ResnetBlock offset in the projection vector
  // the batch is split into lanes of at most ctx->lane_rows rows; each lane has its own plan,
  // activations and step counter, and the lanes' step graphs are replayed concurrently on
  // kStreams streams (the deep UNet levels are latency-bound: independent lanes fill the chip)
  std::vector<std::unique_ptr<Lane>> lanes;
  int plan_B = -1;
  int plan_gen = 0;
  hipStream_t work[kStreams] = {};
  hipEvent_t ev_in = nullptr;
  hipEvent_t ev_done[kStreams] = {};

  ~UNetState() override {
    for (int k = 0; k < kStreams; ++k) {
      if (work[k]) { (void)hipStreamSynchronize(work[k]); (void)hipStreamDestroy(work[k]); }
      if (ev_done[k]) (void)hipEventDestroy(ev_done[k]);
    }
    lanes.clear();
    if (ev_in) (void)hipEventDestroy(ev_in);
  }
  int upload_weights(sddm_ctx* c) override;
  int sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset, float* out,
             float* record, int sample_inter, const float* noise, hipStream_t user) override;
  int forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B, int64_t N,
              float* eps_out, hipStream_t s) override;
  const std::vector<Op>& ops() const override { return lanes.empty() ? Net::ops() : lanes[0]->ops; }   // the same in every lane
  void replan() override { plan_B = -1; lanes.clear(); }

  EmbedArgs embed_args(const sddm_ctx* c) const;
  int build_lane(sddm_ctx* c, Lane& L);
  int prepare_plan(sddm_ctx* c, int64_t B, int64_t N);
  int run_ops(sddm_ctx* c, Lane& L, hipStream_t s);
  int prof_drain(sddm_ctx* c, const Lane& L);
};

// ---------------------------------------------------------------------------------------------
// weight upload: pack every layer into the kernels' layouts in the compute dtype
// ---------------------------------------------------------------------------------------------
int UNetState::upload_weights(sddm_ctx* c) {
  const int dt = c->dtype;
  const size_t es = dtype_size(dt);
  auto P = [&](const std::string& k) -> const Param& { return c->params.at(k); };
  temb_off.clear();
  WeightPacker pk(c, woff);
  // conv weight [co][ci][taps] (3x3: 9 taps, 1x1: 1) as W'[co][k'], k' = (ci / 32 * taps + tap) * 32 + ci % 32
  // (the 32 input channels of one tap side by side), in three images
  auto add_conv = [&](const std::string& name, const Param& w, int taps) {
    const int co = (int)w.shape[0], ci = (int)w.shape[1];
    const int cop = (co + 63) / 64 * 64, K = ci * taps;
    std::vector<float> m((size_t)co * K);
    for (int o = 0; o < co; ++o)
      for (int i = 0; i < ci; ++i)
        for (int tap = 0; tap < taps; ++tap)
          m[(size_t)o * K + ((i / 32) * taps + tap) * 32 + i % 32] = w.data[((size_t)o * ci + i) * taps + tap];
    char* b = pk.raw(name, (size_t)cop * K * es);   // W' itself: [co_pad64][ci/32][taps][32] (T)
    for (size_t j = 0; j < m.size(); ++j) store_elem(b, j, m[j], dt);
    // conv_deep fragment image [co/16][ci/32 * taps][64 lanes][8]: lane l of step s holds
    // W[16 cb + (l & 15)][32 (s / taps) + 8 (l >> 4) + j][tap s % taps]
    store_frags(pk.raw(name + "_f", (size_t)co * K * es), 0, m.data(), co, K, dt);
    if (dt != DT_F32) {  // conv_tile image [ci/32][taps][4][co][8]: one 16-byte unit = 8 input channels
      char* bt = pk.raw(name + "_t", (size_t)co * K * es);
      for (int o = 0; o < co; ++o)
        for (int k = 0; k < K; ++k)
          store_elem(bt, (((size_t)(k / 32) * 4 + (k % 32) / 8) * co + o) * 8 + k % 8, m[(size_t)o * K + k], dt);
    }
  };
  std::vector<float> pw, pb;
  int sc = 0;
  for (const auto& L : unet_layers(u, nullptr, nullptr, nullptr)) {
    const std::string& n = L.name;
    if (L.kind == 0) {
      pk.f32(n + ".weight", P(n + ".weight").data);
      pk.f32(n + ".bias", P(n + ".bias").data);
    } else if (L.kind == 1) {
      pk.f32(n + ".block1.gamma", P(n + ".block1.block.0.weight").data);
      pk.f32(n + ".block1.beta", P(n + ".block1.block.0.bias").data);
      add_conv(n + ".block1.w", P(n + ".block1.block.3.weight"), 9);
      pk.f32(n + ".block1.b", P(n + ".block1.block.3.bias").data);
      pk.f32(n + ".block2.gamma", P(n + ".block2.block.0.weight").data);
      pk.f32(n + ".block2.beta", P(n + ".block2.block.0.bias").data);
      add_conv(n + ".block2.w", P(n + ".block2.block.3.weight"), 9);
      std::vector<float> b2 = P(n + ".block2.block.3.bias").data;
      if (L.cin != L.cout) {
        add_conv(n + ".res.w", P(n + ".res_conv.weight"), 1);
        const auto& rb = P(n + ".res_conv.bias").data;
        for (int i = 0; i < L.cout; ++i) b2[i] = b2[i] + rb[i];
      }
      pk.f32(n + ".block2.b", b2);
      const auto& fw = P(n + ".noise_func.noise_func.0.weight").data;
      const auto& fb = P(n + ".noise_func.noise_func.0.bias").data;
      pw.insert(pw.end(), fw.begin(), fw.end());
      pb.insert(pb.end(), fb.begin(), fb.end());
      temb_off[n] = sc;
      sc += L.cout;
    } else if (L.kind == 2 || L.kind == 3) {
      add_conv(n + ".w", P(n + ".conv.weight"), 9);
      pk.f32(n + ".b", P(n + ".conv.bias").data);
    } else if (L.kind == 5) {
      dt_pack(c, pk, n, kTstLayout, u.n_tstb, kDtPreluShared);   // at the offsets of dual_transformer.h
    } else {
      pk.f32(n + ".gamma", P(n + ".block.0.weight").data);
      pk.f32(n + ".beta", P(n + ".block.0.bias").data);
      pk.f32(n + ".w", P(n + ".block.3.weight").data);  // [1][C][3][3]
      pk.f32(n + ".b", P(n + ".block.3.bias").data);
    }
  }
  pk.f32("mlp.w1", P("noise_level_mlp.1.weight").data);
  pk.f32("mlp.b1", P("noise_level_mlp.1.bias").data);
  pk.f32("mlp.w2", P("noise_level_mlp.3.weight").data);
  pk.f32("mlp.b2", P("noise_level_mlp.3.bias").data);
  pk.f32("proj.w", pw);
  pk.f32("proj.b", pb);
  {  // PositionalEncoding.embedding_vector (UNetModified2.py:53-55), fp32 ops as torch
    const int half = u.inner / 2;
    std::vector<float> ev(half);
    for (int k = 0; k < half; ++k) {
      const float e = (-(float)k * 4.0f) / (float)half;
      ev[k] = 1e4f * std::pow(10.0f, e);
    }
    pk.f32("emb_vec", ev);
  }
  SC = sc;
  plan_B = -1;  // plans hold weight pointers
  return pk.finish(64 * kMaxLanes, &off_tdev, sizeof(float) * (size_t)(c->T + 1) * sc, &off_temb_tab);
}

// the noise MLP and the ResnetBlocks' projections (embed kernel): the caller adds the levels, the
// row count and the output
EmbedArgs UNetState::embed_args(const sddm_ctx* c) const {
  auto wf = [&](const char* k) { return c->warena.at<float>(woff.at(k)); };
  EmbedArgs e{};
  e.dim = u.inner;
  e.emb_vec = wf("emb_vec");
  e.w1 = wf("mlp.w1"); e.b1 = wf("mlp.b1");
  e.w2 = wf("mlp.w2"); e.b2 = wf("mlp.b2");
  e.pw = wf("proj.w"); e.pb = wf("proj.b");
  e.SC = SC; e.no_final_swish = u.mid_tst;
  return e;
}

// ---------------------------------------------------------------------------------------------
// plan: the launch sequence of one UNetModified2 step for batch B
// ---------------------------------------------------------------------------------------------
struct ConvChoice {
  int strip = 0;      // 1: row-streaming kernel (conv_strip.hip), 0: whole-K tile kernel (conv_deep.hip)
  int nblk = 32, SR = 0, mpi = 128;
  int mt = 0, nw = 4, nb = 32;                    // conv_deep: pixels per block, waves, channels
  int tile = -1;                                  // conv_tile configuration (16-bit dtypes), -1: none
  int TR = 0, TW = 0, tiles_x = 0, n_tiles = 0;  // stats tiling of the output
  int chain = 0;                                  // 1: part of the bottom-level chain launch (conv_chain.hip)
};

// conv_deep tile (pixels per block) and waves per block.  A block's time is dominated by its
// one memory round trip, so the grid should need as few rounds of resident blocks as possible
// (256 CUs x 2 blocks at 4 waves, x 1 block at 8 waves); among equal round counts 8 waves (the
// K split 8 ways, weights resident) and then the smaller tile (less work per block) win.
// SDDM_DEEP_CFG=mt:nw forces one configuration wherever it fits (experiments).
static bool choose_deep(int dt, int B, ConvArgs a, bool s2, ConvChoice& ch, int want_mt = 0, int want_nw = 0,
                        int want_nb = 0) {
  static int force_mt = -1, force_nw = -1, force_nb = 0;
  if (force_mt < 0) {
    force_mt = force_nw = 0;
    if (const char* e = std::getenv("SDDM_DEEP_CFG")) std::sscanf(e, "%d:%d:%d", &force_mt, &force_nw, &force_nb);
  }
  // 16-channel blocks only where asked for (tuning table or SDDM_DEEP_CFG): twice the blocks, each
  // with half the weight bytes (the per-CU load volume bounds these layers) but the input halo
  // transformed twice as often
  // (a forced block width that does not divide a layer's channels leaves that layer at 32)
  const int nb = want_mt ? (want_nb ? want_nb : 32) : (force_nb && a.Cout % force_nb == 0 ? force_nb : 32);
  if (a.Cout % nb) return false;
  const int nz = a.Cout / nb;
  a.deep_nb = nb;
  struct Cand { int mt, nw, TR, TW, tiles_x, n_tiles, blocks, rounds; };
  std::vector<Cand> cs;
  // second pass, only when the first finds nothing (frame counts such as 96, whose 6 x 8 level no
  // full tile divides): partly filled tiles of the most rows that divide the image
  for (int pass = 0; pass < 2 && cs.empty(); ++pass)
  for (int mt : {128, 64, 32, 16}) {
    if (mt == 16 && nb != 16) continue;
    const int TW = std::min(a.Wo, mt);
    if (mt % TW || a.Wo % TW) continue;
    int TR = std::min(mt / TW, a.Ho);
    while (pass == 1 && a.Ho % TR) --TR;
    if (a.Ho % TR) continue;
    if (TR * TW < mt && mt > 32 && pass == 0) continue;   // partial tiles only at the smallest size
    a.TR = TR; a.TW = TW; a.tiles_x = a.Wo / TW; a.n_tiles = a.tiles_x * (a.Ho / TR);
    for (int nw : {8, 4}) {
      a.deep_nw = nw;
      if (conv_deep_lds_bytes(dt, mt, s2, a) > kLdsBytes) continue;
      const int blocks = a.n_tiles * B * nz, per_round = 256 * (nw == 4 ? 2 : 1);
      cs.push_back({mt, nw, TR, TW, a.tiles_x, a.n_tiles, blocks, (blocks + per_round - 1) / per_round});
    }
  }
  if (cs.empty()) return false;
  const Cand* pick = nullptr;
  const int fm = want_mt ? want_mt : force_mt, fn = want_mt ? want_nw : force_nw;
  for (const Cand& c : cs)
    if (c.mt == fm && c.nw == fn) pick = &c;
  if (!pick) {
    pick = &cs[0];
    for (const Cand& c : cs) {
      if (c.rounds != pick->rounds) { if (c.rounds < pick->rounds) pick = &c; continue; }
      if (c.nw != pick->nw) { if (c.nw > pick->nw) pick = &c; continue; }
      if (c.mt < pick->mt) pick = &c;
    }
  }
  ch.strip = 0; ch.mt = pick->mt; ch.nw = pick->nw; ch.nb = nb;
  ch.TR = pick->TR; ch.TW = pick->TW; ch.tiles_x = pick->tiles_x; ch.n_tiles = pick->n_tiles;
  return true;
}

// conv_tile configuration: the largest pixel x channel tile (most reuse of each transformed input
// element and weight) among those whose grid still fills the chip; when no tile reaches 256
// blocks, the one with the most blocks.  SDDM_TILE_CFG=<i> forces configuration i wherever it
// fits; SDDM_NO_TILE=1 keeps every 16-bit layer on conv_deep (experiments).
// conv_deep block order: a tile's channel blocks on one XCD (the input halo read once per XCD,
// every XCD reading every weight slice) when the layer's input is at least its weights, else
// z-major (each XCD its own weight slices; the 8x4 / 16x8 levels, where weights dominate).  PMC:
// deep-level traffic 200.6 MB (z-major everywhere) -> 138.6 (channel-inner everywhere) -> ~130 MB
// per step.  SDDM_DEEP_ZIN=0/1 forces one order (A/B runs).
static int deep_zin(const ConvArgs& a, int B, size_t es) {
  static const int force = std::getenv("SDDM_DEEP_ZIN") ? std::atoi(std::getenv("SDDM_DEEP_ZIN")) : -1;
  if (force >= 0) return force;
  const double in = (double)B * a.Hi * a.Wi * (a.CA + a.CB) * es;
  const double w = (double)a.Cout * ((a.CA + a.CB) * 9 + (a.res_mode == 2 ? a.RCA + a.RCB : 0)) * es;
  return in >= w ? 1 : 0;
}

static bool choose_tile(int dt, int B, ConvArgs a, bool s2, ConvChoice& ch, int want = -1) {
  if (dt == DT_F32) return false;
  static const int force = std::getenv("SDDM_TILE_CFG") ? std::atoi(std::getenv("SDDM_TILE_CFG")) : -1;
  static const bool off = std::getenv("SDDM_NO_TILE") != nullptr;
  if (off) return false;
  const int fw = want >= 0 ? want : force;
  struct Cand { int cfg, TR, TW, tiles_x, n_tiles, blocks, area; };
  std::vector<Cand> cs;
  for (int cfg = 0; cfg < conv_tile_ncfg(); ++cfg) {
    const TileCfg t = conv_tile_cfg(cfg);
    const int MT = t.wpx * t.fp * 16, NB = t.wco * t.fc * 16;
    if (a.Cout % NB) continue;
    const int TW = std::min(a.Wo, MT);
    if (MT % TW || a.Wo % TW) continue;
    const int TR = std::min(MT / TW, a.Ho);
    if (a.Ho % TR) continue;
    if (TR * TW < MT && (TR != a.Ho || TW != a.Wo)) continue;   // partial tiles: whole small images only
    a.TR = TR; a.TW = TW; a.tiles_x = a.Wo / TW; a.n_tiles = a.tiles_x * (a.Ho / TR);
    if (conv_tile_lds_bytes(cfg, s2, a) > kLdsBytes) continue;
    cs.push_back({cfg, TR, TW, a.tiles_x, a.n_tiles, a.n_tiles * B * (a.Cout / NB), TR * TW * NB});
  }
  if (cs.empty()) return false;
  const Cand* pick = nullptr;
  for (const Cand& c : cs)
    if (c.cfg == fw) pick = &c;
  if (!pick) {
    for (const Cand& c : cs) {
      if (!pick) { pick = &c; continue; }
      const bool cf = c.blocks >= 256, pf = pick->blocks >= 256;
      if (cf != pf) { if (cf) pick = &c; continue; }
      if (!cf) { if (c.blocks != pick->blocks) { if (c.blocks > pick->blocks) pick = &c; continue; } }
      if (c.area > pick->area) pick = &c;
    }
  }
  ch.strip = 0; ch.tile = pick->cfg;
  ch.TR = pick->TR; ch.TW = pick->TW; ch.tiles_x = pick->tiles_x; ch.n_tiles = pick->n_tiles;
  return true;
}

static bool choose_conv(int dt, int B, int Cin, int RC, int res_mode, int Ho, int Wo, int Cout, bool s2, bool up,
                        ConvChoice& ch, int want_mt = 0, int want_nw = 0, int kind = 0, int ka = 0, int want_nb = 0) {
  ConvArgs a{};
  a.CA = Cin; a.CB = 0; a.RCA = RC; a.RCB = 0; a.res_mode = res_mode; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
  a.upsample = up ? 1 : 0;
  a.Hi = up ? Ho / 2 : (s2 ? Ho * 2 : Ho); a.Wi = up ? Wo / 2 : (s2 ? Wo * 2 : Wo);
  // tuning knobs for experiments (unset = defaults): SDDM_STRIP_MPI=128|256, SDDM_STRIP_BLOCKS=target grid
  static const int env_mpi = std::getenv("SDDM_STRIP_MPI") ? std::atoi(std::getenv("SDDM_STRIP_MPI")) : 0;
  static const int env_blocks = std::getenv("SDDM_STRIP_BLOCKS") ? std::atoi(std::getenv("SDDM_STRIP_BLOCKS")) : 0;
  if (kind == 2) {
    ConvChoice t = ch;
    if (choose_tile(dt, B, a, s2, t, ka) && t.tile == ka) { ch = t; return true; }
  }
  if (!s2 && (Wo == 128 || Wo == 64) && std::getenv("SDDM_NO_STRIP") == nullptr && (kind == 0 || kind == 1)) {
    const int nbs[2] = {(Cout % 64 == 0) ? 64 : 32, 32};
    for (int mpi : {256, 128}) {
      if (env_mpi && mpi != env_mpi) continue;
      const int TRs = mpi / Wo;
      if (Ho % TRs) continue;
      for (int ni = 0; ni < 2; ++ni) {
        const int nb = nbs[ni];
        if (conv_strip_lds_bytes(dt, nb, mpi, a) > kLdsBytes) continue;
        const int nz = (Cout + nb - 1) / nb;
        int SR = 0;
        const int target = env_blocks ? env_blocks : 256;
        for (int m = 32; m >= 2; m /= 2) {   // longest strip that still gives >= target blocks
          const int sr = TRs * m;
          if (Ho % sr) continue;
          SR = sr;
          if ((Ho / sr) * B * nz >= target) break;
        }
        if (SR == 0) continue;
        ch.strip = 1; ch.nblk = nb; ch.SR = SR; ch.mpi = mpi;
        ch.TR = SR; ch.TW = Wo; ch.tiles_x = 1; ch.n_tiles = Ho / SR;
        return true;
      }
    }
  }
  if (want_mt == 0 && kind != 3 && choose_tile(dt, B, a, s2, ch)) return true;
  return choose_deep(dt, B, a, s2, ch, want_mt, want_nw, want_nb);
}

// One conv step as it is launched: the planned arguments, the lane's embedding rows and step counter
// patched in.  flags 0: the step itself; otherwise the timing ablations of SDDM_REPEAT_FLAGS:
// 1 no stats, 2 no GroupNorm transform, 4 no residual / embedding, 8 skip the K loop
struct ConvLaunch {
  ConvArgs a; ConvChoice ch; int dt, B;
  bool s2, temb; int toff;              // temb: block1 of a ResnetBlock, whose projection starts at toff
  const Lane* lane; const UNetState* net;
};
static hipError_t launch_conv(const ConvLaunch& p, int flags, hipStream_t s) {
  ConvArgs x = p.a;
  const ConvChoice& ch = p.ch;
  if (p.temb && !(flags & 4)) {
    x.temb = p.lane->rs.temb + p.toff;
    x.temb_ld = p.net->SC;
    x.temb_per_b = p.lane->rs.temb_per_b;
    x.t_dev = p.lane->rs.t_dev;
  }
  if (flags & 1) x.stats = nullptr;
  if (flags & 2) x.gamma = nullptr;
  if (flags & 4) x.res_mode = 0;
  if (flags) x.dbg = flags;
  if (ch.strip) return launch_conv_strip(p.dt, ch.nblk, ch.mpi, ch.SR, x, p.B, s);
  if (ch.tile >= 0) return launch_conv_tile(p.dt, ch.tile, p.s2, x, p.B, s);
  x.deep_zin = deep_zin(x, p.B, dtype_size(p.dt)); x.deep_nw = ch.nw; x.deep_nb = ch.nb;
  return launch_conv_deep(p.dt, ch.mt, p.s2, x, p.B, s);
}

int UNetState::build_lane(sddm_ctx* c, Lane& L) {
  const int B = L.B;
  Lane* lp = &L;
  const int dt = c->dtype;
  const size_t es = dtype_size(dt);
  const int N = c->num_samples, W = u.seg, S = u.stride;
  const int F = (N - W) / S + 1;
  Arena& A = L.arena;                   // of a new lane: empty

  // ---- pass 1: symbolic program + buffer reservations ----
  std::vector<Tensor> tres;
  auto new_tensor = [&](int C, int H, int Wd, int tiles, int n_tile) -> int {
    Tensor t;
    t.off = A.reserve((size_t)B * H * Wd * C * es);
    t.st_off = A.reserve(sizeof(float) * (size_t)B * tiles * C * 2);
    t.C = C; t.H = H; t.W = Wd; t.tiles = tiles; t.n_tile = n_tile;
    tres.push_back(t);
    return (int)tres.size() - 1;
  };
  struct GNRes { int a, b; std::string w; };   // GroupNorm sources (finalized in the consumer)
  std::vector<GNRes> gres;
  auto new_gn = [&](int xa, int xb, const std::string& w) -> int {
    gres.push_back({xa, xb, w});
    return (int)gres.size() - 1;
  };
  L.off_temb_fwd = A.reserve(sizeof(float) * (size_t)B * std::max(SC, 1));
  L.off_cond = A.reserve(sizeof(float) * (size_t)B * N);
  L.off_x = A.reserve(sizeof(float) * (size_t)B * N);

  enum { ST_CONVIN, ST_GN, ST_CONV, ST_FINAL, ST_TST, ST_CAT };
  struct Step {
    int type = 0;
    std::string w;          // weight-name prefix
    std::string rb;         // ResnetBlock name (temb offset / res weights), "" if none
    int srcA = -1, srcB = -1, gn = -1, out = -1;
    int s2 = 0, up = 0, res_mode = 0, rawA = -1, rawB = -1, cout = 0;
    bool temb = false;
    ConvChoice ch;
  };
  std::vector<Step> prog;
  // measured per-layer deep tiles (sddm_set_conv_tuning) apply when they were measured for this
  // lane batch, dtype and length; otherwise the round-count heuristic of choose_deep decides
  // kernel choices depend on the geometry and the lane capacity, never on the rows a lane holds:
  // every lane, and every row partition of a batch (sharded runs), gets the same kernels, tiles
  // and GroupNorm tilings, hence bit-identical rows
  const int PB = std::max(1, c->lane_rows);
  // A table measured for this exact dtype wins; failing that, a bfloat16 table also serves float16
  // (the same kernels at the same bytes and MFMA rate).  Never the other way: the float16 rows
  // (config #5) have fp16-only compile-time shapes (ConvShape::f16only).
  const sddm_ctx::TuneTable* tuned = nullptr;
  for (const auto& tt : c->tunes)
    if (tt.B == PB && tt.N == N && tt.dtype == dt) { tuned = &tt; break; }
  if (!tuned && dt == DT_F16)
    for (const auto& tt : c->tunes)
      if (tt.B == PB && tt.N == N && tt.dtype == DT_BF16) { tuned = &tt; break; }
  auto pick = [&](const std::string& name, int Cin, int RC, int res_mode, int Ho, int Wo, int cout, bool s2, bool up,
                  ConvChoice& ch) {
    int wm = 0, wn = 0, wb = 0, kind = 0, ka = 0;
    if (tuned) {
      auto it = tuned->deep_tune.find(name);
      if (it != tuned->deep_tune.end()) { wm = it->second.first; wn = it->second.second; kind = 3; }
      auto kt = tuned->kern_tune.find(name);
      if (kt != tuned->kern_tune.end()) {
        kind = kt->second.kind; ka = kt->second.a;
        if (kind == 3) { wm = kt->second.a; wn = kt->second.b; wb = kt->second.c; }
      }
    }
    // "chain": the layer runs inside the bottom-level chain launch; its tensor keeps the tiling the
    // heuristic would give it (only the chain reads or writes it)
    const bool chain = kind == 4 && dt != DT_F32 && !u.mid_tst;   // UNetTST has no mid.0: a table's chain marks are ignored
    if (kind == 4) kind = 0;
    const bool ok = choose_conv(dt, PB, Cin, RC, res_mode, Ho, Wo, cout, s2, up, ch, wm, wn, kind, ka, wb);
    ch.chain = chain ? 1 : 0;
    return ok;
  };
  const int TRin = 512 / W;
  if (u.inner != 32 || 512 % W || F % TRin || (TRin + 1) * S + W + 2 > 1024)
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "conv_in needs inner_channel 32 and segment_len dividing 512 (got %d, %d)", u.inner, W);
  const int t0 = new_tensor(u.inner, F, W, F / TRin, TRin * W);
  { Step st; st.type = ST_CONVIN; st.out = t0; prog.push_back(st); }

  auto res_block = [&](const std::string& n, int xa, int xb, int cin, int cout) -> int {
    const int H = tres[xa].H, Wd = tres[xa].W;
    ConvChoice c1, c2;
    if (!pick(n + ".block1", cin, 0, 0, H, Wd, cout, false, false, c1)) return -1;
    if (!pick(n + ".block2", cout, cin, cin != cout ? 2 : 1, H, Wd, cout, false, false, c2)) return -1;
    // block1's GroupNorm is finalized per source of cat(x, skip); where a group would straddle the
    // two (res_blocks >= 2: GroupNorm(32, 128 + 160)), the concatenation is made real first
    // (ConcatArgs) and block1 reads that one tensor.  The res_conv keeps the two raw sources
    int ga = xa, gb = xb;
    if (xb >= 0 && u.groups > 0 && cin % u.groups == 0 && tres[xa].C % (cin / u.groups)) {
      int nt = std::min(H * Wd, 256);
      while ((H * Wd) % nt) --nt;
      const int m = new_tensor(cin, H, Wd, H * Wd / nt, nt);
      Step st; st.type = ST_CAT; st.w = n + ".cat"; st.srcA = xa; st.srcB = xb; st.out = m;
      prog.push_back(st);
      ga = m; gb = -1;
    }
    const int g1 = new_gn(ga, gb, n + ".block1");
    const int h = new_tensor(cout, H, Wd, c1.n_tiles, c1.TR * c1.TW);
    { Step st; st.type = ST_CONV; st.w = n + ".block1"; st.rb = n; st.srcA = ga; st.srcB = gb; st.gn = g1;
      st.out = h; st.cout = cout; st.temb = true; st.ch = c1; prog.push_back(st); }
    const int g2 = new_gn(h, -1, n + ".block2");
    const int o = new_tensor(cout, H, Wd, c2.n_tiles, c2.TR * c2.TW);
    { Step st; st.type = ST_CONV; st.w = n + ".block2"; st.rb = n; st.srcA = h; st.gn = g2; st.out = o;
      st.cout = cout; st.res_mode = cin != cout ? 2 : 1; st.rawA = xa; st.rawB = xb; st.ch = c2; prog.push_back(st); }
    return o;
  };
  // Downsample (3x3, stride 2) or Upsample (nearest x2, then 3x3) of tensor `cur`, which becomes the output
  auto resample = [&](const LayerDesc& L, int& cur, bool up) -> int {
    const int H = up ? tres[cur].H * 2 : tres[cur].H / 2, Wd = up ? tres[cur].W * 2 : tres[cur].W / 2;
    ConvChoice ch;
    if (!pick(L.name, tres[cur].C, 0, 0, H, Wd, L.cout, !up, up, ch)) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
    const int o = new_tensor(L.cout, H, Wd, ch.n_tiles, ch.TR * ch.TW);
    Step st; st.type = ST_CONV; st.w = L.name; st.srcA = cur; st.out = o; st.s2 = !up; st.up = up; st.cout = L.cout; st.ch = ch;
    prog.push_back(st);
    cur = o;
    return SDDM_OK;
  };
  std::vector<LayerDesc> downs, mid, ups;
  unet_layers(u, &downs, &mid, &ups);
  std::vector<int> feats{t0};
  int cur = t0;
  for (size_t i = 1; i < downs.size(); ++i) {
    const LayerDesc& L = downs[i];
    if (L.kind == 1) {
      cur = res_block(L.name, cur, -1, L.cin, L.cout);
    } else {
      if (tres[cur].H % 2 || tres[cur].W % 2) FAIL(SDDM_ERR_SHAPE, "odd size before %s", L.name.c_str());
      TRY(resample(L, cur, false));
    }
    if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
    feats.push_back(cur);
  }
  for (const LayerDesc& L : mid) {
    if (L.kind == 5) {
      // Dual_Transformer in place of mid.0: one launch, one block and one statistics tile per image
      const int H = tres[cur].H, Wd = tres[cur].W;
      if (L.cin != kTstC || H * Wd > kTstMaxTokens)
        FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Dual_Transformer at %d channels, %d x %d tokens", L.cin, H, Wd);
      const int o = new_tensor(L.cout, H, Wd, 1, H * Wd);
      Step st; st.type = ST_TST; st.w = L.name; st.srcA = cur; st.out = o; st.cout = L.cout;
      prog.push_back(st);
      cur = o;
      continue;
    }
    cur = res_block(L.name, cur, -1, L.cin, L.cout);
    if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
  }
  for (const LayerDesc& L : ups) {
    if (L.kind == 1) {
      const int skip = feats.back();
      feats.pop_back();
      if (tres[skip].H != tres[cur].H || tres[skip].W != tres[cur].W)
        FAIL(SDDM_ERR_SHAPE, "skip/upsample size mismatch at %s (torch.cat would raise)", L.name.c_str());
      cur = res_block(L.name, cur, skip, L.cin, L.cout);
      if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
    } else {
      TRY(resample(L, cur, true));
    }
  }
  const int gf = new_gn(cur, -1, "final_conv");
  { Step st; st.type = ST_FINAL; st.srcA = cur; st.gn = gf; prog.push_back(st); }

  SDDM_HIP_CHECK(A.commit());

  // ---- pass 2: materialise kernel arguments ----
  for (Tensor& t : tres) { t.p = A.base + t.off; t.stats = A.at<float>(t.st_off); }
  auto TT = [&](int i) { return i < 0 ? Tensor{} : tres[i]; };   // -1: no such source
  auto WF = [&](const std::string& k) { return c->warena.at<float>(woff.at(k)); };
  auto WV = [&](const std::string& k) { return (const void*)(c->warena.base + woff.at(k)); };
  // the kernel arguments of one conv step, its algorithmic bytes and FLOPs
  auto conv_args = [&](const Step& st, ConvArgs& a, double& bytes, double& flops) -> int {
    a = ConvArgs{};
    const Tensor sa = TT(st.srcA), sb = TT(st.srcB), o = TT(st.out);
    a.srcA = sa.p; a.srcB = sb.p; a.CA = sa.C; a.CB = sb.C;
    a.Hi = sa.H; a.Wi = sa.W; a.Ho = o.H; a.Wo = o.W; a.upsample = st.up;
    a.Cout = st.cout; a.out = o.p; a.stats = o.stats;
    if (st.gn >= 0) {
      const GNRes& gr = gres[st.gn];
      const Tensor ga = TT(gr.a), gb = TT(gr.b);
      a.gstA = ga.stats; a.gtilesA = ga.tiles; a.gntileA = ga.n_tile;
      a.gstB = gb.stats; a.gtilesB = gb.tiles; a.gntileB = gb.n_tile;
      a.gamma = WF(gr.w + ".gamma"); a.beta = WF(gr.w + ".beta"); a.groups = u.groups; a.eps = 1e-5f;
      const int Ct = ga.C + gb.C;
      if (Ct % u.groups || (gb.C && ga.C % (Ct / u.groups)) || 256 % u.groups)
        FAIL(SDDM_ERR_SHAPE, "GroupNorm(%d, %d) at %s: unsupported grouping", u.groups, Ct, gr.w.c_str());
    }
    a.wgt = WV(st.w + ".w"); a.bias = WF(st.w + ".b");
    a.wgt_t = woff.count(st.w + ".w_t") ? WV(st.w + ".w_t") : nullptr;
    a.wgt_f = WV(st.w + ".w_f");
    a.res_mode = st.res_mode;
    const int Cin = a.CA + a.CB;
    bytes = (double)B * a.Hi * a.Wi * Cin * es + (double)B * a.Ho * a.Wo * a.Cout * es +
            (double)a.Cout * 9 * Cin * es;
    flops = 2.0 * B * a.Ho * a.Wo * a.Cout * 9.0 * Cin;
    if (st.res_mode == 1) {
      a.res_src = TT(st.rawA).p;
      bytes += (double)B * a.Ho * a.Wo * a.Cout * es;
    } else if (st.res_mode == 2) {
      const Tensor ra = TT(st.rawA), rb = TT(st.rawB);
      a.rawA = ra.p; a.rawB = rb.p; a.RCA = ra.C; a.RCB = rb.C;
      a.res_wgt = WV(st.rb + ".res.w");
      a.res_wgt_t = woff.count(st.rb + ".res.w_t") ? WV(st.rb + ".res.w_t") : nullptr;
      a.res_wgt_f = WV(st.rb + ".res.w_f");
      if ((ra.C + rb.C) % 32) FAIL(SDDM_ERR_SHAPE, "%s.res_conv: channels must be multiples of 32", st.rb.c_str());
      bytes += (double)B * a.Ho * a.Wo * (ra.C + rb.C) * es + (double)a.Cout * (ra.C + rb.C) * es;
      flops += 2.0 * B * a.Ho * a.Wo * a.Cout * (double)(ra.C + rb.C);
    }
    const ConvChoice& ch = st.ch;
    a.TR = ch.TR; a.TW = ch.TW; a.tiles_x = ch.tiles_x; a.n_tiles = ch.n_tiles;
    if (a.n_tiles != o.tiles || a.TR * a.TW != o.n_tile) FAIL(SDDM_ERR_STATE, "tile mismatch for %s", st.w.c_str());
    if ((a.CA + a.CB) % 32 || a.Cout % 32) FAIL(SDDM_ERR_SHAPE, "%s: channels must be multiples of 32", st.w.c_str());
    return SDDM_OK;
  };
  for (size_t si = 0; si < prog.size(); ++si) {
    const Step& st = prog[si];
    if (st.type == ST_CONV && st.ch.chain) {
      // the bottom level in one launch (conv_chain.hip): the last Downsample and the four convs of
      // mid.0 and ups.0, every one marked "chain" in the tuning table
      if (si + 4 >= prog.size()) FAIL(SDDM_ERR_SHAPE, "chain: %s is not followed by mid.0 / ups.0", st.w.c_str());
      const Step* S5[5] = {&prog[si], &prog[si + 1], &prog[si + 2], &prog[si + 3], &prog[si + 4]};
      const char* want[5] = {nullptr, "mid.0.block1", "mid.0.block2", "ups.0.block1", "ups.0.block2"};
      for (int k = 0; k < 5; ++k)
        if (S5[k]->type != ST_CONV || !S5[k]->ch.chain || (k > 0 && S5[k]->w != want[k]) || (k == 0 && !S5[k]->s2))
          FAIL(SDDM_ERR_SHAPE, "chain: the tuning table must mark the last Downsample, mid.0.block1/2 and ups.0.block1/2 (got %s)",
               S5[k]->w.c_str());
      ConvArgs ca[5];
      double bytes = 0, flops = 0;
      for (int k = 0; k < 5; ++k) {
        double by = 0, fl = 0;
        if (const int r = conv_args(*S5[k], ca[k], by, fl)) return r;
        flops += fl;
      }
      const int Cc = ca[0].Cout, Hc = ca[0].Ho, Wc = ca[0].Wo;
      if (ca[1].CA != Cc || ca[3].CA != Cc || ca[3].CB != Cc || ca[4].res_mode != 2 || ca[4].RCA != Cc || ca[4].RCB != Cc ||
          ca[2].res_mode != 1 || ca[3].srcB != ca[0].out || ca[4].rawB != ca[0].out)
        FAIL(SDDM_ERR_SHAPE, "chain: unexpected bottom-level wiring");
      ChainArgs x{};
      x.x = ca[0].srcA; x.out = ca[4].out;
      for (int k = 0; k < 5; ++k) { x.wgt[k] = ca[k].wgt_f; x.bias[k] = ca[k].bias; }
      for (int k = 0; k < 4; ++k) { x.gamma[k] = ca[k + 1].gamma; x.beta[k] = ca[k + 1].beta; }
      x.res_wgt = ca[4].res_wgt_f;
      x.temb_ld = SC; x.C = Cc; x.H = Hc; x.W = Wc; x.groups = u.groups; x.eps = 1e-5f;
      bytes = (double)B * (2 * Hc) * (2 * Wc) * Cc * es + (double)B * Hc * Wc * Cc * es;
      for (int k = 0; k < 5; ++k) bytes += (double)ca[k].Cout * (ca[k].CA + ca[k].CB) * 9 * es;
      bytes += (double)Cc * 2 * Cc * es;
      const int toff_m = temb_off.at("mid.0"), toff_u = temb_off.at("ups.0");
      std::string nm;
      for (int k = 0; k < 5; ++k) nm += (k ? "+" : "") + S5[k]->w;
      char kn[96];
      snprintf(kn, sizeof(kn), "conv_chain_kernel<%s,%d,%d,%d>", dt_name(dt), Cc, Hc, Wc);
      L.ops.push_back({2, bytes, flops, [lp, x, dt, B, toff_m, toff_u](hipStream_t s, int) {
                          ChainArgs y = x;
                          y.temb[0] = lp->rs.temb ? lp->rs.temb + toff_m : nullptr;
                          y.temb[1] = lp->rs.temb ? lp->rs.temb + toff_u : nullptr;
                          y.temb_per_b = lp->rs.temb_per_b;
                          y.t_dev = lp->rs.t_dev;
                          return launch_conv_chain(dt, y, B, s);
                        }, nm + "[chain]", kn, kn});
      si += 4;
      continue;
    }
    if (st.type == ST_CAT) {
      const Tensor sa = TT(st.srcA), sb = TT(st.srcB), o = TT(st.out);
      ConcatArgs a{};
      a.a = sa.p; a.b = sb.p; a.CA = sa.C; a.CB = sb.C; a.out = o.p; a.stats = o.stats;
      a.P = o.H * o.W; a.n_tile = o.n_tile;
      const double bytes = 2.0 * B * a.P * o.C * es;
      const std::string kn = std::string("concat_kernel<") + dt_name(dt) + ">";
      L.ops.push_back({4, bytes, 0.0, [a, dt, B](hipStream_t s, int) { return launch_concat(dt, a, B, s); }, st.w, kn, kn});
    } else if (st.type == ST_TST) {
      const Tensor src = TT(st.srcA), o = TT(st.out);
      DualTransformerArgs a{};
      a.x = src.p; a.out = o.p; a.stats = o.stats;
      a.wmat = WV(st.w + ".wmat"); a.wvec = WF(st.w + ".wvec");
      a.dim2 = src.H; a.dim1 = src.W; a.n_tstb = u.n_tstb;
      const int ne = 2 * u.n_tstb;
      const double P = (double)src.H * src.W;
      const double bytes = 2.0 * B * P * kTstC * es + ((double)kTstWEnc0 + (double)ne * kTstEncW) * es;
      const double flops = 2.0 * B * P * (2.0 * kTstC * kTstD + ne * (4.0 * kTstD * kTstD + 2.0 * 3 * kTstHid * (kTstD + kTstHid) +
                                                                   2.0 * kTstHid * kTstD));
      const std::string kn = std::string("dual_transformer_kernel<") + dt_name(dt) + ">";
      L.ops.push_back({4, bytes, flops, [a, dt, B](hipStream_t s, int) { return launch_dual_transformer(dt, a, B, s); },
                       st.w + "[dual_transformer]", kn, kn});
    } else if (st.type == ST_CONVIN) {
      ConvInArgs a{};
      a.N = N; a.F = F; a.W = W; a.S = S; a.Cout = u.inner;
      a.w = WF("downs.0.weight"); a.bias = WF("downs.0.bias");
      const Tensor o = TT(st.out);
      a.out = o.p; a.stats = o.stats; a.TR = TRin;
      const double bytes = (double)B * N * 4 * 2 + (double)B * F * W * u.inner * es;
      const double flops = 2.0 * B * F * W * u.inner * 18;
      TRY(stamp_buffer(c, "downs.0", &a.stamps));
      if (a.stamps) c->stamp_blocks = (int64_t)(F / TRin) * B;
      const std::string kn = std::string("conv_in_kernel<") + dt_name(dt) + ">";
      L.ops.push_back({0, bytes, flops, [lp, a, dt, B](hipStream_t s, int) {
                          ConvInArgs x = a;
                          x.cond = lp->rs.cond; x.x = lp->rs.x; x.t_dev = lp->rs.t_dev;
                          return launch_conv_in(dt, x, B, s);
                        }, "downs.0", kn, kn});
    } else if (st.type == ST_CONV) {
      ConvArgs a;
      double bytes = 0, flops = 0;
      if (const int r = conv_args(st, a, bytes, flops)) return r;
      const int Cin = a.CA + a.CB;
      const ConvChoice ch = st.ch;
      const bool s2 = st.s2 != 0;
      if (std::getenv("SDDM_PRINT_SHAPES"))   // rows for kTileShapes / kDeepShapes / kStripShapes
        fprintf(stderr, "SHAPE %s %s%d s2=%d TR=%d TW=%d Ho=%d Wo=%d CA=%d CB=%d Cout=%d RCA=%d RCB=%d res=%d gn=%d up=%d mt=%d nw=%d nb=%d nblk=%d mpi=%d SR=%d ntiles=%d\n",
                st.w.c_str(), ch.strip ? "strip" : (ch.tile >= 0 ? "tile" : "deep"), ch.tile >= 0 ? ch.tile : ch.mt, s2 ? 1 : 0,
                a.TR, a.TW, a.Ho, a.Wo, a.CA, a.CB, a.Cout, a.RCA, a.RCB, a.res_mode, a.gamma ? 1 : 0, a.upsample ? 1 : 0,
                ch.mt, ch.nw, ch.nb, ch.nblk, ch.mpi, ch.SR, a.n_tiles);
      TRY(stamp_buffer(c, st.w, &a.stamps));
      if (a.stamps) {
        SDDM_HIP_CHECK(hipMemset(a.stamps, 0, kStampBytes));
        if (const char* f = std::getenv("SDDM_STAMPS_DBG")) a.dbg = std::atoi(f);   // timing ablations
        int nb = 32;
        if (ch.tile >= 0) { const TileCfg tc = conv_tile_cfg(ch.tile); nb = tc.wco * tc.fc * 16; }
        c->stamp_blocks = ch.strip ? (int64_t)(a.Ho / ch.SR) * B * ((a.Cout + ch.nblk - 1) / ch.nblk)
                                   : (int64_t)a.n_tiles * B * (a.Cout / (ch.tile >= 0 ? nb : ch.nb));
      }
      const ConvLaunch cl{a, ch, dt, B, s2, st.temb, st.temb ? temb_off.at(st.rb) : 0, lp, this};
      L.ops.push_back({2, bytes, flops, [cl](hipStream_t s, int flags) { return launch_conv(cl, flags, s); },
                       st.w + (ch.strip ? "[strip]" : (ch.tile >= 0 ? "[tile" + std::to_string(ch.tile) + "]"
                                                                     : "[deep" + std::to_string(ch.mt) + "_" + std::to_string(ch.nw) + "_" + std::to_string(ch.nb) + "]"))});
      {
        char kn[160];
        if (ch.strip)
          snprintf(kn, sizeof(kn), "conv_strip_kernel<%s,%d,%d,%d,%d>", dt_name(dt), ch.nblk / 16, a.Wo, Cin, ch.mpi);
        else if (ch.tile >= 0) {
          const TileCfg tc = conv_tile_cfg(ch.tile);
          snprintf(kn, sizeof(kn), "conv_tile_kernel<%s,%d,%d,%d,%d,%d> (tile%d)", dt_name(dt), s2 ? 1 : 0, tc.wpx, tc.wco,
                   tc.fp, tc.fc, ch.tile);
        } else
          snprintf(kn, sizeof(kn), "conv_deep_kernel<%s,%d,%d,%d,%d>", dt_name(dt), s2 ? 1 : 0, ch.mt, ch.nw, ch.nb);
        L.ops.back().kname = kn;
        // instantiation: the strip kernel's residual mode / GroupNorm and the deep kernel's weight
        // ring depth are template arguments the family name leaves out
        char ki[192];
        if (ch.strip)
          snprintf(ki, sizeof(ki), "conv_strip_kernel<%s,%d,%d,%d,%d,%d,%d>", dt_name(dt), ch.nblk / 16, a.Wo, Cin,
                   ch.mpi, a.res_mode, a.gamma ? 1 : 0);
        else if (ch.tile >= 0)
          snprintf(ki, sizeof(ki), "%s", kn);
        else
          snprintf(ki, sizeof(ki), "conv_deep_kernel<%s,%d,%d,%d,%d,%d>", dt_name(dt), s2 ? 1 : 0, ch.mt, ch.nw,
                   conv_deep_ring_depth(dt, ch.mt, ch.nw, (Cin / 32) * 9 + (a.res_mode == 2 ? (a.RCA + a.RCB) / 32 : 0), ch.nb),
                   ch.nb);
        L.ops.back().kinst = ki;
      }
    } else {
      FinalArgs f{};
      const Tensor src = TT(st.srcA);
      f.src = src.p; f.C = src.C;
      {
        const GNRes& gr = gres[st.gn];
        const Tensor ga = TT(gr.a);
        f.gst = ga.stats; f.gtiles = ga.tiles; f.gntile = ga.n_tile;
        f.gamma = WF("final_conv.gamma"); f.beta = WF("final_conv.beta"); f.groups = u.groups; f.eps = 1e-5f;
        if (ga.C % u.groups || 256 % u.groups) FAIL(SDDM_ERR_SHAPE, "final GroupNorm grouping");
      }
      f.w = WF("final_conv.w");
      f.bias = c->params.at("final_conv.block.3.bias").data[0];
      // frames per block: 8 (512 threads); SDDM_FINAL_FT=16 takes 16 (one 1024-thread block per CU,
      // 19 staged frame rows per 16 instead of 11 per 8: less halo re-read)
      static const int env_ft = std::getenv("SDDM_FINAL_FT") ? std::atoi(std::getenv("SDDM_FINAL_FT")) : 0;
      f.N = N; f.F = F; f.W = W; f.S = S; f.FT = (env_ft == 16 && F % 16 == 0) ? 16 : (F % 8 == 0 ? 8 : 2);
      if (F % f.FT || W % S) FAIL(SDDM_ERR_SHAPE, "final tile: frames %d, segment %d/%d", F, W, S);
      f.co = c->coef();
      const double bytes = (double)B * F * W * src.C * es + (double)B * N * 4 * 3;
      const double flops = 2.0 * B * F * W * src.C * 9;
      TRY(stamp_buffer(c, "final_conv", &f.stamps));
      if (f.stamps) c->stamp_blocks = (int64_t)(F / f.FT) * B;
      const std::string kn = std::string("final_kernel<") + dt_name(dt) + (f.FT >= 16 ? ",1024>" : ",512>");
      L.ops.push_back({3, bytes, flops, [lp, f, dt, B](hipStream_t s, int) {
                          FinalArgs x = f;
                          x.mode = lp->rs.final_mode; x.eps_out = lp->rs.eps_out;
                          x.x = lp->rs.x; x.cond = lp->rs.cond; x.t_dev = lp->rs.t_dev;
                          x.seed = lp->rs.seed; x.row_offset = lp->rs.row_offset;
                          x.noise = lp->rs.noise; x.noise_ld = lp->rs.noise_ld;
                          x.sp = lp->rs.t_dev ? (const StepParams*)lp->rs.t_dev : nullptr;
                          return launch_final(dt, x, B, s);
                        }, "final_conv", kn, kn});
    }
  }
  return SDDM_OK;
}

// the plan of batch B, kept until B or the tuning changes: the batch split into lanes of lane_rows rows
// (the same per-lane plan for any row partition into multiples of lane_rows, so sharded runs stay
// bit-identical to a single run)
int UNetState::prepare_plan(sddm_ctx* c, int64_t Bn, int64_t N) {
  if (N != c->num_samples)
    FAIL(SDDM_ERR_SHAPE, "condition has %lld samples, network built for num_samples=%d", (long long)N, c->num_samples);
  if (Bn < 1 || Bn > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)Bn);
  const int B = (int)Bn;
  if (plan_B == B) return SDDM_OK;
  lanes.clear();
  plan_B = -1;
  const int LR = std::max(1, c->lane_rows);
  const int nl = (B + LR - 1) / LR;
  if (nl > kMaxLanes) FAIL(SDDM_ERR_INVALID_ARG, "batch %d needs %d lanes (max %d): raise SDDM_LANE_ROWS", B, nl, kMaxLanes);
  for (int l = 0; l < nl; ++l) {
    std::unique_ptr<Lane> L(new Lane());
    L->idx = l;
    L->row0 = l * LR;
    L->B = std::min(LR, B - l * LR);
    const int r = build_lane(c, *L);
    if (r) { lanes.clear(); return r; }
    lanes.push_back(std::move(L));
  }
  plan_B = B;
  plan_gen++;
  return SDDM_OK;
}

// ---------------------------------------------------------------------------------------------
// run: one step of a lane, the reverse loop, one forward
// ---------------------------------------------------------------------------------------------
int UNetState::prof_drain(sddm_ctx* c, const Lane& L) {
  if (c->ev_pend.empty()) return SDDM_OK;
  SDDM_HIP_CHECK(hipEventSynchronize(c->ev_pool[c->ev_pend.back().second + 1]));
  if (c->op_acc.size() < L.ops.size()) c->op_acc.resize(L.ops.size());
  for (const auto& pe : c->ev_pend) {
    float m = 0;
    SDDM_HIP_CHECK(hipEventElapsedTime(&m, c->ev_pool[pe.second], c->ev_pool[pe.second + 1]));
    ProfAcc& a = c->op_acc[pe.first];
    a.ms += m; a.n += 1; a.bytes += L.ops[pe.first].bytes; a.flops += L.ops[pe.first].flops;
  }
  c->ev_pend.clear();
  return SDDM_OK;
}

int UNetState::run_ops(sddm_ctx* c, Lane& L, hipStream_t s) {
  for (const Op& op : L.ops) {
    const bool timed = c->prof && c->ev_pend.size() * 2 + 2 <= c->ev_pool.size();
    int e0 = 0;
    if (timed) {
      e0 = (int)c->ev_pend.size() * 2;
      SDDM_HIP_CHECK(hipEventRecord(c->ev_pool[e0], s));
    }
    hipError_t e = op.run(s, 0);
    if (e != hipSuccess) FAIL(SDDM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    {  // dev knob: SDDM_REPEAT_OP=<layer> SDDM_REPEAT_N=<n> relaunches one (idempotent) layer
      static const char* rop = std::getenv("SDDM_REPEAT_OP");
      static const int rn = std::getenv("SDDM_REPEAT_N") ? std::atoi(std::getenv("SDDM_REPEAT_N")) : 0;
      static const int rflags = std::getenv("SDDM_REPEAT_FLAGS") ? std::atoi(std::getenv("SDDM_REPEAT_FLAGS")) : 0;
      if (rop && op.name.rfind(rop, 0) == 0)
        for (int k = 0; k < rn && e == hipSuccess; ++k) e = op.run(s, rflags);
      if (e != hipSuccess) FAIL(SDDM_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    if (timed) {
      SDDM_HIP_CHECK(hipEventRecord(c->ev_pool[e0 + 1], s));
      c->ev_pend.push_back({(int)(&op - L.ops.data()), e0});
    }
  }
  if (c->prof) return prof_drain(c, L);
  return SDDM_OK;
}

// SDDM.infer (model.py:50-124): cond [B][1][N], the initial state and the transition of the context's
// p_transition (the transition is the tail of the final kernel).  out [B][1][N]
int UNetState::sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset, float* out,
                      float* record, int sample_inter, const float* noise, hipStream_t user) {
  TRY(prepare_plan(c, B, N));
  // (caller-supplied noise: the step graphs would bake its pointer; the per-launch path reads it)
  const bool graph = c->use_graphs && !c->prof && !record && !noise;
  const int T = c->T;
  StepParams* sp0 = c->warena.at<StepParams>(off_tdev);
  float* temb_tab = c->warena.at<float>(off_temb_tab);
  // noise-level embeddings of every t (same for all rows: model.py:108)
  EmbedArgs e = embed_args(c);
  e.table = c->dtab(3); e.time_step_mode = c->noise_time_step; e.R = T + 1; e.out = temb_tab;
  SDDM_HIP_CHECK(launch_embed(e, user));
  // per-lane state: x_t (graph-stable copy when replaying graphs), condition rows, step counter
  for (auto& Lp : lanes) {
    Lane& L = *Lp;
    const int64_t rows = L.B, off = (int64_t)L.row0 * N;
    float* xb = graph ? L.arena.at<float>(L.off_x) : out + off;
    const float* cb = cond + off;
    if (graph) {
      SDDM_HIP_CHECK(hipMemcpyAsync(L.arena.at<float>(L.off_cond), cb, sizeof(float) * rows * N,
                                    hipMemcpyDeviceToDevice, user));
      cb = L.arena.at<float>(L.off_cond);
    }
    StepParams* sp = (StepParams*)((char*)sp0 + 64 * L.idx);
    InitArgs ia{};
    ia.mode = c->init_mode; ia.cond = cb; ia.out = xb; ia.total = rows * N; ia.N = N; ia.T = T;
    ia.co = c->coef(); ia.seed = seed; ia.row_offset = row_offset + L.row0;
    ia.noise = noise ? noise + off : nullptr;
    SDDM_HIP_CHECK(launch_init_state(ia, user));
    SDDM_HIP_CHECK(launch_set_params(sp, T + 1, seed, row_offset + L.row0, user));
    L.rs.cond = cb; L.rs.x = xb; L.rs.temb = temb_tab; L.rs.temb_per_b = 0; L.rs.t_dev = &sp->t;
    L.rs.final_mode = c->tr_mode; L.rs.eps_out = nullptr; L.rs.seed = seed; L.rs.row_offset = row_offset + L.row0;
    L.rs.noise = noise ? noise + off : nullptr; L.rs.noise_ld = B * N;
  }
  if (graph) {
    const int ns = std::min<int>(kStreams, (int)lanes.size());
    if (!ev_in) SDDM_HIP_CHECK(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
    for (int k = 0; k < ns; ++k)
      if (!work[k]) {
        SDDM_HIP_CHECK(hipStreamCreateWithFlags(&work[k], hipStreamNonBlocking));
        SDDM_HIP_CHECK(hipEventCreateWithFlags(&ev_done[k], hipEventDisableTiming));
      }
    SDDM_HIP_CHECK(hipEventRecord(ev_in, user));
    for (int k = 0; k < ns; ++k) SDDM_HIP_CHECK(hipStreamWaitEvent(work[k], ev_in, 0));
    int K = 1;
    for (int k : {10, 8, 5, 4, 2})
      if (T % k == 0) { K = k; break; }
    for (auto& Lp : lanes) {   // capture K steps of every lane once per plan
      Lane& L = *Lp;
      if (L.gexec && L.g_gen == plan_gen && L.g_K == K) continue;
      if (L.gexec) { (void)hipGraphExecDestroy(L.gexec); L.gexec = nullptr; }
      if (L.graph) { (void)hipGraphDestroy(L.graph); L.graph = nullptr; }
      hipStream_t s = work[L.idx % ns];
      SDDM_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
      for (int k = 0; k < K; ++k) {
        if (const int r = run_ops(c, L, s)) {
          hipGraph_t junk = nullptr;
          (void)hipStreamEndCapture(s, &junk);
          if (junk) (void)hipGraphDestroy(junk);
          return r;
        }
      }
      SDDM_HIP_CHECK(hipStreamEndCapture(s, &L.graph));
      SDDM_HIP_CHECK(hipGraphInstantiate(&L.gexec, L.graph, nullptr, nullptr, 0));
      L.g_gen = plan_gen;
      L.g_K = K;
    }
    // lanes on different streams start with a phase offset (SDDM_LANE_OFFSET_US per lane index):
    // one lane's latency-bound deep levels then overlap another lane's bandwidth-bound wide levels
    static const int off_us = std::getenv("SDDM_LANE_OFFSET_US") ? std::atoi(std::getenv("SDDM_LANE_OFFSET_US")) : 0;
    if (off_us > 0)
      for (auto& Lp : lanes)
        if (Lp->idx % ns) SDDM_HIP_CHECK(launch_delay((unsigned)(off_us * (Lp->idx % ns)), work[Lp->idx % ns]));
    for (int i = 0; i < T / K; ++i)
      for (auto& Lp : lanes) SDDM_HIP_CHECK(hipGraphLaunch(Lp->gexec, work[Lp->idx % ns]));
    for (auto& Lp : lanes)
      SDDM_HIP_CHECK(hipMemcpyAsync(out + (int64_t)Lp->row0 * N, Lp->rs.x, sizeof(float) * Lp->B * N,
                                    hipMemcpyDeviceToDevice, work[Lp->idx % ns]));
    for (int k = 0; k < ns; ++k) {
      SDDM_HIP_CHECK(hipEventRecord(ev_done[k], work[k]));
      SDDM_HIP_CHECK(hipStreamWaitEvent(user, ev_done[k], 0));
    }
    return SDDM_OK;
  }
  int64_t nrec = 0;
  for (int t = T; t >= 1; --t) {
    for (auto& Lp : lanes) TRY(run_ops(c, *Lp, user));
    if (record && t % sample_inter == 0) {  // model.py:100-101: keep x_{t-1} when t % inter == 0
      SDDM_HIP_CHECK(hipMemcpyAsync(record + nrec * B * N, out, sizeof(float) * B * N, hipMemcpyDeviceToDevice, user));
      ++nrec;
    }
  }
  return SDDM_OK;
}

// one forward (UNetModified2.py:237-269): cond, x_t [B][1][N], noise level [B] -> eps [B][1][N]
int UNetState::forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B, int64_t N,
                       float* eps_out, hipStream_t s) {
  TRY(prepare_plan(c, B, N));
  for (auto& Lp : lanes) {
    Lane& L = *Lp;
    const int64_t off = (int64_t)L.row0 * N;
    float* temb = L.arena.at<float>(L.off_temb_fwd);
    EmbedArgs e = embed_args(c);
    e.noise_levels = noise_level + L.row0; e.R = L.B; e.out = temb;
    SDDM_HIP_CHECK(launch_embed(e, s));
    L.rs.cond = cond + off; L.rs.x = const_cast<float*>(x_t) + off; L.rs.temb = temb; L.rs.temb_per_b = 1;
    L.rs.t_dev = nullptr; L.rs.final_mode = -1; L.rs.eps_out = eps_out + off; L.rs.seed = 0; L.rs.row_offset = 0;
    L.rs.noise = nullptr;
    TRY(run_ops(c, L, s));
  }
  return SDDM_OK;
}
