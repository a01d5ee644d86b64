// UNetModified2 / UNetTST path of the runtime (included by sddm_runtime.cpp after sddm_ctx, Net and the
// weight packers): configuration check, weight packing, the plan of one reverse step (unet_plan.h: pure
// host arithmetic) materialised per lane, and its run, of reference model/UNetModified2.py:146-269 and
// model/UNetTST.py:270-392 as a Net.  Unlike the sequential networks it runs in lanes whose step graphs
// replay concurrently.
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
#include "unet_plan.h"   // UNetCfg, unet_layers and the planner: which kernel and tiling every conv gets

// the network's arguments (`na`; num_samples may also stand at the config's top level) -> `u` and the
// length the network is built for.  tst: UNetTST (UNetTST.py:270-392), i.e. UNetModified2 with mid =
// Dual_Transformer and no final Swish in the noise MLP
static int unet_configure(const Json& cfg, const Json& na, bool tst, UNetCfg& u, int* num_samples, bool modified = false) {
  // UNetModified (UNetModified.py:192-323): its own default widths, attention levels, one level boundary fewer
  u.modified = modified ? 1 : 0;
  u.in_channel = (int)na.number("in_channel", 2);
  u.out_channel = (int)na.number("out_channel", 1);
  u.inner = (int)na.number("inner_channel", 32);
  u.groups = (int)na.number("norm_groups", 32);
  u.mults = na.ints("channel_mults", modified ? std::vector<int>{1, 2, 4, 8, 8} : std::vector<int>{1, 2, 3, 4, 5});
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
  if (modified && u.mults.empty()) FAIL(SDDM_ERR_INVALID_ARG, "channel_mults: at least one level");
  const int div = modified ? 1 << ((int)u.mults.size() - 1) : 1 << (int)u.mults.size();
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
  if (modified) {   // everything the plan or the attention kernels would refuse later is refused here
    // attn_layer: the reference tests `ind in attn_layer`, so an int (the class default `(4)`) is a TypeError there
    if (na.at("attn_layer").kind != Json::ARR) FAIL(SDDM_ERR_INVALID_ARG, "attn_layer must be a list of levels (UNetModified.py:238: `ind in attn_layer`)");
    u.attn = na.ints("attn_layer", {});
    if (na.has("with_noise_level_emb") && na.number("with_noise_level_emb", 1) == 0)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "with_noise_level_emb=False (the reference fails in nn.Linear(None, ...), UNetModified.py:67)");
    u.mid_tst = 0;
    if (u.res_blocks < 0) FAIL(SDDM_ERR_INVALID_ARG, "res_blocks %d", u.res_blocks);
    if (u.inner != 32 || 512 % u.seg)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "inner_channel %d / segment_len %d: conv_in needs 32 and a divisor of 512", u.inner, u.seg);
    if (u.groups < 1 || 256 % u.groups)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "norm_groups %d: the GroupNorm finalize needs a divisor of 256", u.groups);
    for (int m : u.mults)
      if (m < 1 || (u.inner * m) % u.groups)
        FAIL(SDDM_ERR_NOT_IMPLEMENTED, "channel_mults / norm_groups: %d channels in groups of %d", u.inner * m, u.groups);
    for (const auto& L : unet_layers(u, nullptr, nullptr, nullptr))
      if (!L.attn.empty() && L.cout > kAttnMaxC)
        FAIL(SDDM_ERR_NOT_IMPLEMENTED, "channel_mults / attn_layer: %s has %d channels, the self-attention kernels hold %d",
             L.attn.c_str(), L.cout, kAttnMaxC);
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
      if (!L.attn.empty()) {   // SelfAttention (UNetModified.py:146-148): the qkv conv has no bias
        s[L.attn + ".norm.weight"] = {L.cout};
        s[L.attn + ".norm.bias"] = {L.cout};
        s[L.attn + ".qkv.weight"] = {3 * (int64_t)L.cout, L.cout, 1, 1};
        s[L.attn + ".out.weight"] = {L.cout, L.cout, 1, 1};
        s[L.attn + ".out.bias"] = {L.cout};
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
  // the batch is split into lanes of at most ctx->lane_rows rows; each lane has its own launches
  // of the one plan, activations and step counter, and the lanes' step graphs are replayed concurrently
  // on kStreams streams (the deep UNet levels are latency-bound: independent lanes fill the chip)
  UNetPlan plan;
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
      if (!L.attn.empty()) {   // the two 1x1 convs as MFMA A fragments (store_frags), the rest fp32
        const std::string& an = L.attn;
        const int C = L.cout;
        pk.f32(an + ".norm.gamma", P(an + ".norm.weight").data);
        pk.f32(an + ".norm.beta", P(an + ".norm.bias").data);
        store_frags(pk.raw(an + ".qkv_f", (size_t)3 * C * C * es), 0, P(an + ".qkv.weight").data.data(), 3 * C, C, dt);
        store_frags(pk.raw(an + ".out_f", (size_t)C * C * es), 0, P(an + ".out.weight").data.data(), C, C, dt);
        pk.f32(an + ".out.b", P(an + ".out.bias").data);
      }
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
      // UNetModified.py:52-56: exp(-ln(1e4) * k / half), no 1e4 factor (the kernel multiplies by the level
      // and takes sin, then cos, as for the others)
      if (u.modified) ev[k] = std::exp((float)(-std::log(1e4)) * ((float)k / (float)half));
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
  e.SC = SC; e.no_final_swish = u.mid_tst || u.modified;
  return e;
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
  if (ch.wide) return launch_conv_wide(p.dt, p.s2, x, p.B, s);
  if (ch.strip) return launch_conv_strip(p.dt, ch.nblk, ch.mpi, ch.SR, x, p.B, s);
  if (ch.tile >= 0) return launch_conv_tile(p.dt, ch.tile, p.s2, x, p.B, s);
  x.deep_zin = deep_zin(x, p.B, dtype_size(p.dt), p.net->plan.knobs.deep_zin); x.deep_nw = ch.nw; x.deep_nb = ch.nb;
  return launch_conv_deep(p.dt, ch.mt, p.s2, x, p.B, s);
}

// ---------------------------------------------------------------------------------------------
// a lane: the plan (unet_plan.h) materialised for the lane's rows -- arena, kernel arguments, ops
// ---------------------------------------------------------------------------------------------
struct LaneBuilder {
  sddm_ctx* c;
  UNetState& net;
  Lane& L;
  const UNetPlan& plan;
  const UNetCfg& u;
  const int B, dt;
  const size_t es;
  std::vector<Tensor> tres;   // the plan's tensors in the lane's arena

  LaneBuilder(sddm_ctx* ctx, UNetState& n, Lane& lane)
      : c(ctx), net(n), L(lane), plan(n.plan), u(n.u), B(lane.B), dt(ctx->dtype), es(dtype_size(ctx->dtype)) {}

  Tensor TT(int i) const { return i < 0 ? Tensor{} : tres[i]; }   // -1: no such source
  const float* WF(const std::string& k) const { return c->warena.at<float>(net.woff.at(k)); }
  const void* WV(const std::string& k) const { return (const void*)(c->warena.base + net.woff.at(k)); }
  std::string tname(const char* kernel, const char* rest = ">") const { return std::string(kernel) + "<" + dt_name(dt) + rest; }

  // the arena of a new (empty) lane: the lane's own rows, then per tensor in creation order the
  // activation followed by its statistics
  int reserve() {
    Arena& A = L.arena;
    L.off_temb_fwd = A.reserve(sizeof(float) * (size_t)B * std::max(net.SC, 1));
    L.off_cond = A.reserve(sizeof(float) * (size_t)B * plan.N);
    L.off_x = A.reserve(sizeof(float) * (size_t)B * plan.N);
    for (const PlanTensor& pt : plan.tensors) {
      Tensor t;
      t.off = A.reserve((size_t)B * pt.H * pt.W * pt.C * es);
      t.st_off = A.reserve(sizeof(float) * (size_t)B * pt.tiles * pt.C * 2);
      t.C = pt.C; t.H = pt.H; t.W = pt.W; t.tiles = pt.tiles; t.n_tile = pt.n_tile;
      tres.push_back(t);
    }
    SDDM_HIP_CHECK(A.commit());
    for (Tensor& t : tres) { t.p = A.base + t.off; t.stats = A.at<float>(t.st_off); }
    return SDDM_OK;
  }

  // the kernel arguments of one conv step, its algorithmic bytes and FLOPs
  int conv_args(const Step& st, ConvArgs& a, double& bytes, double& flops) const {
    a = conv_geometry(plan, st);
    const Tensor sa = TT(st.srcA), sb = TT(st.srcB), o = TT(st.out);
    a.srcA = sa.p; a.srcB = sb.p; a.out = o.p; a.stats = o.stats;
    if (st.gn >= 0) {
      const PlanGN& gr = plan.gns[st.gn];
      const Tensor ga = TT(gr.a), gb = TT(gr.b);
      a.gstA = ga.stats; a.gtilesA = ga.tiles; a.gntileA = ga.n_tile;
      a.gstB = gb.stats; a.gtilesB = gb.tiles; a.gntileB = gb.n_tile;
      a.gamma = WF(gr.w + ".gamma"); a.beta = WF(gr.w + ".beta"); a.groups = u.groups; a.eps = 1e-5f;
      const int Ct = ga.C + gb.C;
      if (Ct % u.groups || (gb.C && ga.C % (Ct / u.groups)) || 256 % u.groups)
        FAIL(SDDM_ERR_SHAPE, "GroupNorm(%d, %d) at %s: unsupported grouping", u.groups, Ct, gr.w.c_str());
    }
    a.wgt = WV(st.w + ".w"); a.bias = WF(st.w + ".b");
    a.wgt_t = net.woff.count(st.w + ".w_t") ? WV(st.w + ".w_t") : nullptr;
    a.wgt_f = WV(st.w + ".w_f");
    const int Cin = a.CA + a.CB;
    bytes = (double)B * a.Hi * a.Wi * Cin * es + (double)B * a.Ho * a.Wo * a.Cout * es + (double)a.Cout * 9 * Cin * es;
    flops = 2.0 * B * a.Ho * a.Wo * a.Cout * 9.0 * Cin;
    if (st.res_mode == 1) {
      a.res_src = TT(st.rawA).p;
      bytes += (double)B * a.Ho * a.Wo * a.Cout * es;
    } else if (st.res_mode == 2) {
      const int RC = a.RCA + a.RCB;
      a.rawA = TT(st.rawA).p; a.rawB = TT(st.rawB).p;
      a.res_wgt = WV(st.rb + ".res.w");
      a.res_wgt_t = net.woff.count(st.rb + ".res.w_t") ? WV(st.rb + ".res.w_t") : nullptr;
      a.res_wgt_f = WV(st.rb + ".res.w_f");
      if (RC % 32) FAIL(SDDM_ERR_SHAPE, "%s.res_conv: channels must be multiples of 32", st.rb.c_str());
      bytes += (double)B * a.Ho * a.Wo * RC * es + (double)a.Cout * RC * es;
      flops += 2.0 * B * a.Ho * a.Wo * a.Cout * (double)RC;
    }
    if (a.n_tiles != o.tiles || a.TR * a.TW != o.n_tile) FAIL(SDDM_ERR_STATE, "tile mismatch for %s", st.w.c_str());
    if (Cin % 32 || a.Cout % 32) FAIL(SDDM_ERR_SHAPE, "%s: channels must be multiples of 32", st.w.c_str());
    return SDDM_OK;
  }

  int add_conv(const Step& st) {
    ConvArgs a;
    double bytes = 0, flops = 0;
    TRY(conv_args(st, a, bytes, flops));
    const ConvChoice& ch = st.ch;
    TRY(stamp_buffer(c, st.w, &a.stamps));
    if (a.stamps) {
      SDDM_HIP_CHECK(hipMemset(a.stamps, 0, kStampBytes));
      if (const char* f = std::getenv("SDDM_STAMPS_DBG")) a.dbg = std::atoi(f);   // timing ablations
      int nb = ch.nb;   // (conv_wide: 32, as planned)
      if (ch.tile >= 0) { const TileCfg tc = conv_tile_cfg(ch.tile); nb = tc.wco * tc.fc * 16; }
      c->stamp_blocks = ch.strip ? (int64_t)(a.Ho / ch.SR) * B * ((a.Cout + ch.nblk - 1) / ch.nblk)
                                 : (int64_t)a.n_tiles * B * (a.Cout / nb);
    }
    const ConvLaunch cl{a, ch, dt, B, st.s2 != 0, st.temb, st.temb ? net.temb_off.at(st.rb) : 0, &L, &net};
    const ConvNames nm = conv_names(dt, st.s2 != 0, ch, a, a.gamma != nullptr);
    L.ops.push_back({2, bytes, flops, [cl](hipStream_t s, int flags) { return launch_conv(cl, flags, s); }, st.w + nm.tag,
                     nm.kname, nm.kinst});
    return SDDM_OK;
  }

  // the bottom level in one launch (conv_chain.hip): the last Downsample (step si) and the four
  // convs of mid.0 and ups.0, every one marked "chain" in the tuning table
  int add_chain(size_t si) {
    const std::vector<Step>& prog = plan.steps;
    if (si + 4 >= prog.size()) FAIL(SDDM_ERR_SHAPE, "chain: %s is not followed by mid.0 / ups.0", prog[si].w.c_str());
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
      TRY(conv_args(*S5[k], ca[k], by, fl));
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
    x.temb_ld = net.SC; x.C = Cc; x.H = Hc; x.W = Wc; x.groups = u.groups; x.eps = 1e-5f;
    bytes = (double)B * (2 * Hc) * (2 * Wc) * Cc * es + (double)B * Hc * Wc * Cc * es;
    for (int k = 0; k < 5; ++k) bytes += (double)ca[k].Cout * (ca[k].CA + ca[k].CB) * 9 * es;
    bytes += (double)Cc * 2 * Cc * es;
    const int toff_m = net.temb_off.at("mid.0"), toff_u = net.temb_off.at("ups.0");
    std::string name;
    for (int k = 0; k < 5; ++k) name += (k ? "+" : "") + S5[k]->w;
    const ConvNames nm = conv_names(dt, true, S5[0]->ch, ca[0], false);
    const Lane* lp = &L;
    const int dtv = dt, Bv = B;
    L.ops.push_back({2, bytes, flops, [lp, x, dtv, Bv, toff_m, toff_u](hipStream_t s, int) {
                        ChainArgs y = x;
                        y.temb[0] = lp->rs.temb ? lp->rs.temb + toff_m : nullptr;
                        y.temb[1] = lp->rs.temb ? lp->rs.temb + toff_u : nullptr;
                        y.temb_per_b = lp->rs.temb_per_b;
                        y.t_dev = lp->rs.t_dev;
                        return launch_conv_chain(dtv, y, Bv, s);
                      }, name + nm.tag, nm.kname, nm.kinst});
    return SDDM_OK;
  }

  int add_concat(const Step& st) {
    const Tensor sa = TT(st.srcA), sb = TT(st.srcB), o = TT(st.out);
    ConcatArgs a{};
    a.a = sa.p; a.b = sb.p; a.CA = sa.C; a.CB = sb.C; a.out = o.p; a.stats = o.stats;
    a.P = o.H * o.W; a.n_tile = o.n_tile;
    const double bytes = 2.0 * B * a.P * o.C * es;
    const std::string kn = tname("concat_kernel");
    const int dtv = dt, Bv = B;
    L.ops.push_back({4, bytes, 0.0, [a, dtv, Bv](hipStream_t s, int) { return launch_concat(dtv, a, Bv, s); }, st.w, kn, kn});
    return SDDM_OK;
  }

  // SelfAttention: attn_qkv into the scratch tensor, then attn_core (self_attention.hip)
  int add_attention(const Step& st) {
    const Tensor src = TT(st.srcA), o = TT(st.out), qkv = TT(st.scratch), ga = TT(plan.gns[st.gn].a);
    const int C = src.C, P = src.H * src.W;
    if (C % 32 || C > kAttnMaxC || C % u.groups || 256 % u.groups)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "%s: %d channels in %d groups (multiples of 32 up to %d)", st.w.c_str(), C, u.groups, kAttnMaxC);
    if (attn_core_lds_bytes(dt, C) > (size_t)kLdsBytes || attn_qkv_lds_bytes(dt, C) > (size_t)kLdsBytes)
      FAIL(SDDM_ERR_STATE, "%s: LDS", st.w.c_str());
    AttnArgs a{};
    a.x = src.p; a.gst = ga.stats; a.gtiles = ga.tiles; a.gntile = ga.n_tile;
    a.gamma = WF(st.w + ".norm.gamma"); a.beta = WF(st.w + ".norm.beta"); a.groups = u.groups; a.eps = 1e-5f;
    a.wqkv_f = WV(st.w + ".qkv_f"); a.qkv = qkv.p; a.wout_f = WV(st.w + ".out_f"); a.bout = WF(st.w + ".out.b");
    a.out = o.p; a.stats = o.stats; a.P = P; a.C = C; a.QT = o.n_tile;
    a.scale_log2 = (float)(1.4426950408889634 / std::sqrt((double)C));
    if (o.tiles * o.n_tile != P || o.n_tile != attn_query_tile(P)) FAIL(SDDM_ERR_STATE, "tile mismatch for %s", st.w.c_str());
    const double bq = (double)B * P * C * es * 4 + 3.0 * C * C * es, fq = 2.0 * B * P * 3.0 * C * C;
    const double bc = (double)B * P * C * es * (3.0 * ((P + o.n_tile - 1) / o.n_tile) + 2) + (double)C * C * es;
    const double fc = 4.0 * B * (double)P * P * C + 2.0 * B * P * (double)C * C;
    const int dtv = dt, Bv = B;
    const std::string kq = tname("attn_qkv_kernel"), kc = tname("attn_core_kernel", ("," + std::to_string(C / 32) + ">").c_str());
    L.ops.push_back({4, bq, fq, [a, dtv, Bv](hipStream_t s, int) { return launch_attn_qkv(dtv, a, Bv, s); }, st.w + "[qkv]", kq, kq});
    L.ops.push_back({4, bc, fc, [a, dtv, Bv](hipStream_t s, int) { return launch_attn_core(dtv, a, Bv, s); }, st.w + "[attention]", kc, kc});
    return SDDM_OK;
  }

  int add_dual_transformer(const Step& st) {
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
    const std::string kn = tname("dual_transformer_kernel");
    const int dtv = dt, Bv = B;
    L.ops.push_back({4, bytes, flops, [a, dtv, Bv](hipStream_t s, int) { return launch_dual_transformer(dtv, a, Bv, s); },
                     st.w + "[dual_transformer]", kn, kn});
    return SDDM_OK;
  }

  int add_conv_in(const Step& st) {
    const int N = plan.N, F = plan.F, W = u.seg;
    ConvInArgs a{};
    a.N = N; a.F = F; a.W = W; a.S = u.stride; a.Cout = u.inner;
    a.w = WF("downs.0.weight"); a.bias = WF("downs.0.bias");
    const Tensor o = TT(st.out);
    a.out = o.p; a.stats = o.stats; a.TR = st.TRin;
    const double bytes = (double)B * N * 4 * 2 + (double)B * F * W * u.inner * es;
    const double flops = 2.0 * B * F * W * u.inner * 18;
    TRY(stamp_buffer(c, "downs.0", &a.stamps));
    if (a.stamps) c->stamp_blocks = (int64_t)(F / st.TRin) * B;
    const std::string kn = tname("conv_in_kernel");
    const Lane* lp = &L;
    const int dtv = dt, Bv = B;
    L.ops.push_back({0, bytes, flops, [lp, a, dtv, Bv](hipStream_t s, int) {
                        ConvInArgs x = a;
                        x.cond = lp->rs.cond; x.x = lp->rs.x; x.t_dev = lp->rs.t_dev;
                        return launch_conv_in(dtv, x, Bv, s);
                      }, "downs.0", kn, kn});
    return SDDM_OK;
  }

  int add_final(const Step& st) {
    const int N = plan.N, F = plan.F, W = u.seg;
    FinalArgs f{};
    const Tensor src = TT(st.srcA), ga = TT(plan.gns[st.gn].a);
    f.src = src.p; f.C = src.C;
    f.gst = ga.stats; f.gtiles = ga.tiles; f.gntile = ga.n_tile;
    f.gamma = WF("final_conv.gamma"); f.beta = WF("final_conv.beta"); f.groups = u.groups; f.eps = 1e-5f;
    if (ga.C % u.groups || 256 % u.groups) FAIL(SDDM_ERR_SHAPE, "final GroupNorm grouping");
    f.w = WF("final_conv.w");
    f.bias = c->params.at("final_conv.block.3.bias").data[0];
    f.N = N; f.F = F; f.W = W; f.S = u.stride; f.FT = st.FT;
    f.co = c->coef();
    const double bytes = (double)B * F * W * src.C * es + (double)B * N * 4 * 3;
    const double flops = 2.0 * B * F * W * src.C * 9;
    TRY(stamp_buffer(c, "final_conv", &f.stamps));
    if (f.stamps) c->stamp_blocks = (int64_t)(F / f.FT) * B;
    const std::string kn = tname("final_kernel", f.FT >= 16 ? ",1024>" : ",512>");
    const Lane* lp = &L;
    const int dtv = dt, Bv = B;
    L.ops.push_back({3, bytes, flops, [lp, f, dtv, Bv](hipStream_t s, int) {
                        FinalArgs x = f;
                        x.mode = lp->rs.final_mode; x.eps_out = lp->rs.eps_out;
                        x.x = lp->rs.x; x.cond = lp->rs.cond; x.t_dev = lp->rs.t_dev;
                        x.seed = lp->rs.seed; x.row_offset = lp->rs.row_offset;
                        x.noise = lp->rs.noise; x.noise_ld = lp->rs.noise_ld;
                        x.sp = lp->rs.t_dev ? (const StepParams*)lp->rs.t_dev : nullptr;
                        return launch_final(dtv, x, Bv, s);
                      }, "final_conv", kn, kn});
    return SDDM_OK;
  }
};

int UNetState::build_lane(sddm_ctx* c, Lane& L) {
  LaneBuilder b(c, *this, L);
  TRY(b.reserve());
  for (size_t si = 0; si < plan.steps.size(); ++si) {
    const Step& st = plan.steps[si];
    if (st.type == ST_CONV && st.ch.chain) { TRY(b.add_chain(si)); si += 4; }
    else if (st.type == ST_CONV) TRY(b.add_conv(st));
    else if (st.type == ST_CAT) TRY(b.add_concat(st));
    else if (st.type == ST_TST) TRY(b.add_dual_transformer(st));
    else if (st.type == ST_ATTN) TRY(b.add_attention(st));
    else if (st.type == ST_CONVIN) TRY(b.add_conv_in(st));
    else TRY(b.add_final(st));
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
  // one plan, chosen for lanes of lane_rows rows whatever a lane holds; every lane materialises it
  TRY(plan_unet(u, c->num_samples, c->dtype, LR, match_tuning(c->tunes, LR, c->num_samples, c->dtype), PlanKnobs::env(), plan));
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
