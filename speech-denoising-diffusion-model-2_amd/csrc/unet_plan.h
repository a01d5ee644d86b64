// The UNetModified2 / UNetTST planner (included by sddm_runtime.cpp before sddm_ctx): which kernel and
// tiling every conv of one reverse step gets, and the tensors and GroupNorm sources between them.
// Pure host arithmetic: a plan is a function of the architecture, the length, the dtype, the lane
// capacity, a measured tuning table (or none) and the experiment knobs, and of nothing else -- no HIP
// call, no device memory, no context, no environment read below plan_unet.  The runtime
// (unet_runtime.h) materialises a plan into launches; sddm_unet_plan returns one as JSON without a
// device, which is what tools/gen_shapes.py and tests/test_unet_plan.py read.
#pragma once
#include "kernels.h"
#include "dual_transformer.h"
#include "self_attention.h"

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
  int modified = 0;  // 1: UNetModified (UNetModified.py:192-323) -- SelfAttention after the ResnetBlocks of the levels in
  std::vector<int> attn;   // attn_layer, no Downsample after the last level, mid = (block + attention, block),
                           // res_blocks + 1 decoder blocks per level, Upsample after them; no final Swish in the noise MLP
};
// kind 0 conv,1 res,2 down,3 up,4 final,5 dual transformer; attn: the SelfAttention that follows a res block ("": none)
struct LayerDesc { int kind; std::string name; int cin, cout; std::string attn = ""; };
// UNetModified.py:237-277: blocks are ResnetBlocWithAttn, so a block's tensors sit under <layer>.res_block / <layer>.attn
static void unet_modified_layers(const UNetCfg& c, std::vector<LayerDesc>& downs, std::vector<LayerDesc>& mid,
                                 std::vector<LayerDesc>& ups, int* last) {
  auto with_attn = [&](int ind) { return std::find(c.attn.begin(), c.attn.end(), ind) != c.attn.end(); };
  auto block = [](const char* part, int idx, int cin, int cout, bool attn) {
    const std::string n = std::string(part) + "." + std::to_string(idx);
    return LayerDesc{1, n + ".res_block", cin, cout, attn ? n + ".attn" : ""};
  };
  downs.push_back({0, "downs.0", c.in_channel, c.inner});
  std::vector<int> feat{c.inner};
  int cin = c.inner, idx = 1;
  const int nm = (int)c.mults.size();
  for (int ind = 0; ind < nm; ++ind) {
    const int cout = c.inner * c.mults[ind];
    for (int r = 0; r < c.res_blocks; ++r) {
      downs.push_back(block("downs", idx++, cin, cout, with_attn(ind)));
      feat.push_back(cout);
      cin = cout;
    }
    if (ind != nm - 1) {
      downs.push_back({2, "downs." + std::to_string(idx++), cin, cin});
      feat.push_back(cin);
    }
  }
  mid.push_back(block("mid", 0, cin, cin, true));
  mid.push_back(block("mid", 1, cin, cin, false));
  idx = 0;
  for (int ind = nm - 1; ind >= 0; --ind) {
    const int cout = c.inner * c.mults[ind];
    for (int r = 0; r < c.res_blocks + 1; ++r) {
      ups.push_back(block("ups", idx++, cin + feat.back(), cout, with_attn(ind)));
      feat.pop_back();
      cin = cout;
    }
    if (ind >= 1) ups.push_back({3, "ups." + std::to_string(idx++), cin, cin});
  }
  *last = cin;
}
static std::vector<LayerDesc> unet_layers(const UNetCfg& c, std::vector<LayerDesc>* downs_out,
                                          std::vector<LayerDesc>* mid_out, std::vector<LayerDesc>* ups_out) {
  std::vector<LayerDesc> downs, mid, ups;
  int cin = c.inner, idx = 1, cout = c.inner;
  if (c.modified) {
    unet_modified_layers(c, downs, mid, ups, &cout);
  } else {
  downs.push_back({0, "downs.0", c.in_channel, c.inner});
  std::vector<int> feat{c.inner};
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

// ---------------------------------------------------------------------------------------------
// inputs of a plan besides the architecture: experiment knobs and measured tuning tables
// ---------------------------------------------------------------------------------------------
// The experiment knobs, read from the environment once per process (the sweep tools set them per
// process).  Unset = the defaults below.
struct PlanKnobs {
  int deep_mt = 0, deep_nw = 0, deep_nb = 0;   // SDDM_DEEP_CFG=mt:nw[:nb] forces one conv_deep configuration wherever it fits
  int tile_cfg = -1;                           // SDDM_TILE_CFG=<i> forces conv_tile configuration i wherever it fits
  bool no_tile = false;                        // SDDM_NO_TILE=1 keeps every 16-bit layer on conv_deep
  bool no_strip = false;                       // SDDM_NO_STRIP=1 keeps every layer off conv_strip
  int strip_mpi = 0, strip_blocks = 0;         // SDDM_STRIP_MPI=128|256, SDDM_STRIP_BLOCKS=target grid
  int deep_zin = -1;                           // SDDM_DEEP_ZIN=0/1 forces one conv_deep block order (A/B runs)
  int final_ft = 0;                            // SDDM_FINAL_FT=16: 16 frames per block of the final kernel
  static const PlanKnobs& env() {
    static const PlanKnobs k = [] {
      PlanKnobs r;
      auto num = [](const char* name, int unset) { const char* e = std::getenv(name); return e ? std::atoi(e) : unset; };
      if (const char* e = std::getenv("SDDM_DEEP_CFG")) std::sscanf(e, "%d:%d:%d", &r.deep_mt, &r.deep_nw, &r.deep_nb);
      r.tile_cfg = num("SDDM_TILE_CFG", -1);
      r.no_tile = std::getenv("SDDM_NO_TILE") != nullptr;
      r.no_strip = std::getenv("SDDM_NO_STRIP") != nullptr;
      r.strip_mpi = num("SDDM_STRIP_MPI", 0);
      r.strip_blocks = num("SDDM_STRIP_BLOCKS", 0);
      r.deep_zin = num("SDDM_DEEP_ZIN", -1);
      r.final_ft = num("SDDM_FINAL_FT", 0);
      return r;
    }();
    return k;
  }
};

// A measured per-layer kernel table (sddm_set_conv_tuning), valid for one lane batch / dtype /
// num_samples: conv_deep tiles per layer name (pixels per block, waves) and the kernel choice
// (1 strip, 2 tile (a = configuration), 3 deep (a = pixels, b = waves, c = channels), 4 chain)
struct KernTune { int kind, a, b, c; };
struct TuneTable {
  std::map<std::string, std::pair<int, int>> deep_tune;
  std::map<std::string, KernTune> kern_tune;
  int B = -1, dtype = -1, N = -1;
};

// a tuning JSON -> tables: one table, or {"tables": [table, ...]}
static int parse_conv_tuning(const char* json, std::vector<TuneTable>& out) {
  Json j;
  try {
    j = Json::parse(json);
  } catch (const std::exception& e) {
    FAIL(SDDM_ERR_INVALID_ARG, "tuning JSON: %s", e.what());
  }
  std::vector<const Json*> tabs;
  if (j.has("tables")) {
    const Json& arr = j.at("tables");
    if (arr.kind != Json::ARR) FAIL(SDDM_ERR_INVALID_ARG, "tables: a list");
    for (const auto& t : arr.arr) tabs.push_back(&t);
  } else {
    tabs.push_back(&j);
  }
  out.clear();
  for (const Json* tp : tabs) {
    const Json& t = *tp;
    if (t.kind != Json::OBJ) FAIL(SDDM_ERR_INVALID_ARG, "tuning table: an object");
    TuneTable tt;
    const std::string dts = t.string("dtype", "");
    tt.dtype = dts == "float32" ? DT_F32 : dts == "bfloat16" ? DT_BF16 : dts == "float16" ? DT_F16 : -1;
    if (t.has("deep"))
      for (const auto& kv : t.at("deep").obj) {
        if (kv.second.kind != Json::ARR || kv.second.arr.size() != 2) FAIL(SDDM_ERR_INVALID_ARG, "deep.%s: [mt, nw]", kv.first.c_str());
        tt.deep_tune[kv.first] = {(int)kv.second.arr[0].num, (int)kv.second.arr[1].num};
      }
    // "kernel": {"<layer>": "strip" | "tile:<cfg>" | "deep" | "deep:<mt>:<nw>[:<nb>]" | "chain"}
    if (t.has("kernel"))
      for (const auto& kv : t.at("kernel").obj) {
        if (kv.second.kind != Json::STR) FAIL(SDDM_ERR_INVALID_ARG, "kernel.%s: a string", kv.first.c_str());
        const std::string& v = kv.second.str;
        KernTune k{0, 0, 0, 0};
        if (v == "strip") k.kind = 1;
        else if (v.rfind("tile:", 0) == 0) { k.kind = 2; k.a = std::atoi(v.c_str() + 5); }
        else if (v == "deep") k.kind = 3;
        else if (v.rfind("deep:", 0) == 0) { k.kind = 3; std::sscanf(v.c_str() + 5, "%d:%d:%d", &k.a, &k.b, &k.c); }
        else if (v == "chain") k.kind = 4;
        else FAIL(SDDM_ERR_INVALID_ARG, "kernel.%s: unknown choice '%s'", kv.first.c_str(), v.c_str());
        if (k.kind == 2 && (k.a < 0 || k.a >= conv_tile_ncfg())) FAIL(SDDM_ERR_INVALID_ARG, "kernel.%s: tile configuration %d", kv.first.c_str(), k.a);
        tt.kern_tune[kv.first] = k;
      }
    tt.B = (int)t.number("lane_batch", -1);
    tt.N = (int)t.number("num_samples", -1);
    out.push_back(std::move(tt));
  }
  return SDDM_OK;
}

// The table of a plan: the first measured for this lane capacity, length and exact dtype; failing
// that, a bfloat16 table also serves float16 (the same kernels at the same bytes and MFMA rate).
// Never the other way: the float16 rows (config #5) have fp16-only compile-time shapes
// (ConvShape::f16only).  Null: the heuristics of choose_conv decide
static const TuneTable* match_tuning(const std::vector<TuneTable>& tunes, int lane_rows, int N, int dt) {
  const int PB = std::max(1, lane_rows);
  for (const auto& tt : tunes)
    if (tt.B == PB && tt.N == N && tt.dtype == dt) return &tt;
  if (dt == DT_F16)
    for (const auto& tt : tunes)
      if (tt.B == PB && tt.N == N && tt.dtype == DT_BF16) return &tt;
  return nullptr;
}

// ---------------------------------------------------------------------------------------------
// the kernel choice of one conv
// ---------------------------------------------------------------------------------------------
struct ConvChoice {
  int strip = 0;      // 1: row-streaming kernel (conv_strip.hip), 0: whole-K tile kernel (conv_deep.hip)
  int nblk = 32, SR = 0, mpi = 128;
  int mt = 0, nw = 4, nb = 32;                    // conv_deep: pixels per block, waves, channels
  int tile = -1;                                  // conv_tile configuration (16-bit dtypes), -1: none
  int TR = 0, TW = 0, tiles_x = 0, n_tiles = 0;  // stats tiling of the output
  int chain = 0;                                  // 1: part of the bottom-level chain launch (conv_chain.hip)
  int wide = 0;                                   // 1: K-chunked kernel (conv_wide.hip): mt = pixels per block
};

// conv_deep tile (pixels per block) and waves per block.  A block's time is dominated by its
// one memory round trip, so the grid should need as few rounds of resident blocks as possible
// (256 CUs x 2 blocks at 4 waves, x 1 block at 8 waves); among equal round counts 8 waves (the
// K split 8 ways, weights resident) and then the smaller tile (less work per block) win.
// PlanKnobs::deep_* force one configuration wherever it fits (experiments).
static bool choose_deep(const PlanKnobs& k, int dt, int B, ConvArgs a, bool s2, ConvChoice& ch, int want_mt = 0,
                        int want_nw = 0, int want_nb = 0) {
  // 16-channel blocks only where asked for (tuning table or the knob): twice the blocks, each
  // with half the weight bytes (the per-CU load volume bounds these layers) but the input halo
  // transformed twice as often
  // (a forced block width that does not divide a layer's channels leaves that layer at 32)
  const int nb = want_mt ? (want_nb ? want_nb : 32) : (k.deep_nb && a.Cout % k.deep_nb == 0 ? k.deep_nb : 32);
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
  const int fm = want_mt ? want_mt : k.deep_mt, fn = want_mt ? want_nw : k.deep_nw;
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

// conv_deep block order: a tile's channel blocks on one XCD (the input halo read once per XCD,
// every XCD reading every weight slice) when the layer's input is at least its weights, else
// z-major (each XCD its own weight slices; the 8x4 / 16x8 levels, where weights dominate).  PMC:
// deep-level traffic 200.6 MB (z-major everywhere) -> 138.6 (channel-inner everywhere) -> ~130 MB
// per step.  force >= 0 (PlanKnobs::deep_zin) takes that order.
static int deep_zin(const ConvArgs& a, int B, size_t es, int force) {
  if (force >= 0) return force;
  const double in = (double)B * a.Hi * a.Wi * (a.CA + a.CB) * es;
  const double w = (double)a.Cout * ((a.CA + a.CB) * 9 + (a.res_mode == 2 ? a.RCA + a.RCB : 0)) * es;
  return in >= w ? 1 : 0;
}

// conv_tile configuration: the largest pixel x channel tile (most reuse of each transformed input
// element and weight) among those whose grid still fills the chip; when no tile reaches 256
// blocks, the one with the most blocks.  PlanKnobs::tile_cfg forces one configuration wherever it
// fits; no_tile keeps every 16-bit layer on conv_deep (experiments).
static bool choose_tile(const PlanKnobs& k, int dt, int B, ConvArgs a, bool s2, ConvChoice& ch, int want = -1) {
  if (dt == DT_F32) return false;
  if (k.no_tile) return false;
  const int fw = want >= 0 ? want : k.tile_cfg;
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

// conv_wide tile: the layers whose K no other kernel holds (float32 from about 256 input channels plus a
// res_conv).  The largest tile of at most 64 pixels whose rows divide the image; untuned
static bool choose_wide(int dt, ConvArgs a, bool s2, ConvChoice& ch) {
  if (a.Cout % 32 || (a.CA + a.CB) % 32) return false;
  for (int mt : {64, 32, 16}) {
    const int TW = std::min(a.Wo, mt);
    if (mt % TW || a.Wo % TW) continue;
    int TR = std::min(mt / TW, a.Ho);
    while (a.Ho % TR) --TR;
    a.TR = TR; a.TW = TW; a.tiles_x = a.Wo / TW; a.n_tiles = a.tiles_x * (a.Ho / TR);
    if (conv_wide_lds_bytes(dt, s2, a) > (size_t)kLdsBytes) continue;
    ch.strip = 0; ch.tile = -1; ch.wide = 1; ch.mt = TR * TW; ch.nw = 4; ch.nb = 32;
    ch.TR = TR; ch.TW = TW; ch.tiles_x = a.tiles_x; ch.n_tiles = a.n_tiles;
    return true;
  }
  return false;
}

static bool choose_conv(const PlanKnobs& k, int dt, int B, int Cin, int RC, int res_mode, int Ho, int Wo, int Cout, bool s2,
                        bool up, ConvChoice& ch, int want_mt = 0, int want_nw = 0, int kind = 0, int ka = 0, int want_nb = 0) {
  ConvArgs a{};
  a.CA = Cin; a.CB = 0; a.RCA = RC; a.RCB = 0; a.res_mode = res_mode; a.Ho = Ho; a.Wo = Wo; a.Cout = Cout;
  a.upsample = up ? 1 : 0;
  a.Hi = up ? Ho / 2 : (s2 ? Ho * 2 : Ho); a.Wi = up ? Wo / 2 : (s2 ? Wo * 2 : Wo);
  if (kind == 2) {
    ConvChoice t = ch;
    if (choose_tile(k, dt, B, a, s2, t, ka) && t.tile == ka) { ch = t; return true; }
  }
  // (the strip kernel holds a res_conv of at most 128 input channels in registers: launch_conv_strip refuses more)
  const bool strip_res_ok = res_mode != 2 || RC <= 128;
  if (!s2 && (Wo == 128 || Wo == 64) && !k.no_strip && (kind == 0 || kind == 1) && strip_res_ok) {
    const int nbs[2] = {(Cout % 64 == 0) ? 64 : 32, 32};
    for (int mpi : {256, 128}) {
      if (k.strip_mpi && mpi != k.strip_mpi) continue;
      const int TRs = mpi / Wo;
      if (Ho % TRs) continue;
      for (int ni = 0; ni < 2; ++ni) {
        const int nb = nbs[ni];
        if (conv_strip_lds_bytes(dt, nb, mpi, a) > kLdsBytes) continue;
        const int nz = (Cout + nb - 1) / nb;
        int SR = 0;
        const int target = k.strip_blocks ? k.strip_blocks : 256;
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
  if (want_mt == 0 && kind != 3 && choose_tile(k, dt, B, a, s2, ch)) return true;
  if (choose_deep(k, dt, B, a, s2, ch, want_mt, want_nw, want_nb)) return true;
  return choose_wide(dt, a, s2, ch);   // only where nothing above fits: no earlier plan changes
}

// ---------------------------------------------------------------------------------------------
// the plan: the launch sequence of one UNetModified2 step, symbolically
// ---------------------------------------------------------------------------------------------
struct PlanTensor { int C = 0, H = 0, W = 0, tiles = 0, n_tile = 0; };   // an activation and its per-tile GroupNorm statistics
struct PlanGN { int a, b; std::string w; };   // GroupNorm sources (finalized in the consumer), `w`: whose gamma / beta
enum { ST_CONVIN, ST_CONV, ST_FINAL, ST_TST, ST_CAT, ST_ATTN };
struct Step {
  int type = 0;
  std::string w;          // weight-name prefix
  std::string rb;         // ResnetBlock name (temb offset / res weights), "" if none
  int srcA = -1, srcB = -1, gn = -1, out = -1;   // indices into UNetPlan::tensors / gns
  int s2 = 0, up = 0, res_mode = 0, rawA = -1, rawB = -1, cout = 0;
  bool temb = false;
  ConvChoice ch;
  int TRin = 0, FT = 0;   // ST_CONVIN: frame rows per block; ST_FINAL: frames per block
  int scratch = -1;       // ST_ATTN: the qkv tensor [P][3C] (no statistics)
};
struct UNetPlan {
  int N = 0, F = 0, dt = 0, PB = 0;    // length, frames, dtype, the lane capacity the kernels are chosen for
  PlanKnobs knobs;
  std::vector<PlanTensor> tensors;     // in creation order (the order of the arena reservations)
  std::vector<PlanGN> gns;
  std::vector<Step> steps;             // in launch order
};

// the layer walk that fills a UNetPlan (plan_unet below is the entry point)
struct UNetPlanner {
  const UNetCfg& u;
  const TuneTable* tuned;
  const PlanKnobs& k;
  UNetPlan& p;

  int new_tensor(int C, int H, int W, int tiles, int n_tile) {
    p.tensors.push_back({C, H, W, tiles, n_tile});
    return (int)p.tensors.size() - 1;
  }
  int new_gn(int xa, int xb, const std::string& w) {
    p.gns.push_back({xa, xb, w});
    return (int)p.gns.size() - 1;
  }
  // Measured per-layer kernels (the tuning table) where the table names the layer; otherwise the
  // heuristics of choose_conv.  Kernel choices depend on the geometry and the lane capacity, never
  // on the rows a lane holds: every lane, and every row partition of a batch (sharded runs), gets
  // the same kernels, tiles and GroupNorm tilings, hence bit-identical rows
  bool pick(const std::string& name, int Cin, int RC, int res_mode, int Ho, int Wo, int cout, bool s2, bool up, ConvChoice& ch) {
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
    const bool chain = kind == 4 && p.dt != DT_F32 && !u.mid_tst;   // UNetTST has no mid.0: a table's chain marks are ignored
    if (kind == 4) kind = 0;
    const bool ok = choose_conv(k, p.dt, p.PB, Cin, RC, res_mode, Ho, Wo, cout, s2, up, ch, wm, wn, kind, ka, wb);
    ch.chain = chain ? 1 : 0;
    return ok;
  }
  // a ResnetBlock over cat(xa, xb) (xb -1: over xa alone); the output tensor, or -1: no tile fits
  int res_block(const std::string& n, int xa, int xb, int cin, int cout) {
    const int H = p.tensors[xa].H, Wd = p.tensors[xa].W;
    ConvChoice c1, c2;
    if (!pick(n + ".block1", cin, 0, 0, H, Wd, cout, false, false, c1)) return -1;
    if (!pick(n + ".block2", cout, cin, cin != cout ? 2 : 1, H, Wd, cout, false, false, c2)) return -1;
    // block1's GroupNorm is finalized per source of cat(x, skip); where a group would straddle the
    // two (res_blocks >= 2: GroupNorm(32, 128 + 160)), the concatenation is made real first
    // (ConcatArgs) and block1 reads that one tensor.  The res_conv keeps the two raw sources
    int ga = xa, gb = xb;
    if (xb >= 0 && u.groups > 0 && cin % u.groups == 0 && p.tensors[xa].C % (cin / u.groups)) {
      int nt = std::min(H * Wd, 256);
      while ((H * Wd) % nt) --nt;
      const int m = new_tensor(cin, H, Wd, H * Wd / nt, nt);
      Step st; st.type = ST_CAT; st.w = n + ".cat"; st.srcA = xa; st.srcB = xb; st.out = m;
      p.steps.push_back(st);
      ga = m; gb = -1;
    }
    const int g1 = new_gn(ga, gb, n + ".block1");
    const int h = new_tensor(cout, H, Wd, c1.n_tiles, c1.TR * c1.TW);
    { Step st; st.type = ST_CONV; st.w = n + ".block1"; st.rb = n; st.srcA = ga; st.srcB = gb; st.gn = g1;
      st.out = h; st.cout = cout; st.temb = true; st.ch = c1; p.steps.push_back(st); }
    const int g2 = new_gn(h, -1, n + ".block2");
    const int o = new_tensor(cout, H, Wd, c2.n_tiles, c2.TR * c2.TW);
    { Step st; st.type = ST_CONV; st.w = n + ".block2"; st.rb = n; st.srcA = h; st.gn = g2; st.out = o;
      st.cout = cout; st.res_mode = cin != cout ? 2 : 1; st.rawA = xa; st.rawB = xb; st.ch = c2; p.steps.push_back(st); }
    return o;
  }
  // SelfAttention `n` (UNetModified.py:140-169) over tensor x: two launches (attn_qkv, attn_core) in one step;
  // the output's statistics tiles are the query tiles
  int attention(const std::string& n, int x) {
    const PlanTensor t = p.tensors[x];
    const int P = t.H * t.W, QT = attn_query_tile(P);
    const int qkv = new_tensor(3 * t.C, t.H, t.W, 0, 0);
    const int o = new_tensor(t.C, t.H, t.W, P / QT, QT);
    Step st; st.type = ST_ATTN; st.w = n; st.srcA = x; st.gn = new_gn(x, -1, n + ".norm"); st.scratch = qkv; st.out = o;
    st.cout = t.C;
    p.steps.push_back(st);
    return o;
  }
  // a ResnetBlock and the SelfAttention behind it, if the layer has one
  int block(const LayerDesc& L, int xa, int xb) {
    const int o = res_block(L.name, xa, xb, L.cin, L.cout);
    return o < 0 || L.attn.empty() ? o : attention(L.attn, o);
  }
  // Downsample (3x3, stride 2) or Upsample (nearest x2, then 3x3) of tensor `cur`, which becomes the output
  int resample(const LayerDesc& L, int& cur, bool up) {
    const PlanTensor t = p.tensors[cur];
    const int H = up ? t.H * 2 : t.H / 2, Wd = up ? t.W * 2 : t.W / 2;
    ConvChoice ch;
    if (!pick(L.name, t.C, 0, 0, H, Wd, L.cout, !up, up, ch)) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
    const int o = new_tensor(L.cout, H, Wd, ch.n_tiles, ch.TR * ch.TW);
    Step st; st.type = ST_CONV; st.w = L.name; st.srcA = cur; st.out = o; st.s2 = !up; st.up = up; st.cout = L.cout; st.ch = ch;
    p.steps.push_back(st);
    cur = o;
    return SDDM_OK;
  }
  int walk() {
    const int W = u.seg, S = u.stride, F = p.F;
    const int TRin = 512 / std::max(W, 1);
    if (u.inner != 32 || W < 1 || 512 % W || F % TRin || (TRin + 1) * S + W + 2 > 1024)
      FAIL(SDDM_ERR_NOT_IMPLEMENTED, "conv_in needs inner_channel 32 and segment_len dividing 512 (got %d, %d)", u.inner, W);
    const int t0 = new_tensor(u.inner, F, W, F / TRin, TRin * W);
    { Step st; st.type = ST_CONVIN; st.w = "downs.0"; st.out = t0; st.TRin = TRin; p.steps.push_back(st); }
    std::vector<LayerDesc> downs, mid, ups;
    unet_layers(u, &downs, &mid, &ups);
    std::vector<int> feats{t0};
    int cur = t0;
    for (size_t i = 1; i < downs.size(); ++i) {
      const LayerDesc& L = downs[i];
      if (L.kind == 1) {
        cur = block(L, cur, -1);
      } else {
        if (p.tensors[cur].H % 2 || p.tensors[cur].W % 2) FAIL(SDDM_ERR_SHAPE, "odd size before %s", L.name.c_str());
        TRY(resample(L, cur, false));
      }
      if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
      feats.push_back(cur);
    }
    for (const LayerDesc& L : mid) {
      if (L.kind == 5) {
        // Dual_Transformer in place of mid.0: one launch, one block and one statistics tile per image
        const int H = p.tensors[cur].H, Wd = p.tensors[cur].W;
        if (L.cin != kTstC || H * Wd > kTstMaxTokens)
          FAIL(SDDM_ERR_NOT_IMPLEMENTED, "Dual_Transformer at %d channels, %d x %d tokens", L.cin, H, Wd);
        const int o = new_tensor(L.cout, H, Wd, 1, H * Wd);
        Step st; st.type = ST_TST; st.w = L.name; st.srcA = cur; st.out = o; st.cout = L.cout;
        p.steps.push_back(st);
        cur = o;
        continue;
      }
      cur = block(L, cur, -1);
      if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
    }
    for (const LayerDesc& L : ups) {
      if (L.kind == 1) {
        const int skip = feats.back();
        feats.pop_back();
        if (p.tensors[skip].H != p.tensors[cur].H || p.tensors[skip].W != p.tensors[cur].W)
          FAIL(SDDM_ERR_SHAPE, "skip/upsample size mismatch at %s (torch.cat would raise)", L.name.c_str());
        cur = block(L, cur, skip);
        if (cur < 0) FAIL(SDDM_ERR_SHAPE, "no tile for %s", L.name.c_str());
      } else {
        TRY(resample(L, cur, true));
      }
    }
    // final kernel, frames per block: 8 (512 threads); PlanKnobs::final_ft 16 takes 16 (one
    // 1024-thread block per CU, 19 staged frame rows per 16 instead of 11 per 8: less halo re-read)
    Step st; st.type = ST_FINAL; st.w = "final_conv"; st.srcA = cur; st.gn = new_gn(cur, -1, "final_conv");
    st.FT = (k.final_ft == 16 && F % 16 == 0) ? 16 : (F % 8 == 0 ? 8 : 2);
    if (F % st.FT || W % S) FAIL(SDDM_ERR_SHAPE, "final tile: frames %d, segment %d/%d", F, W, S);
    p.steps.push_back(st);
    return SDDM_OK;
  }
};

// The plan of one reverse step of network `u` at length num_samples in dtype dt, its kernels chosen
// for lanes of lane_rows rows; `tuned`: the measured table of this geometry (match_tuning), or null
static int plan_unet(const UNetCfg& u, int num_samples, int dt, int lane_rows, const TuneTable* tuned, const PlanKnobs& k,
                     UNetPlan& out) {
  out = UNetPlan{};
  out.N = num_samples; out.dt = dt; out.PB = std::max(1, lane_rows); out.knobs = k;
  out.F = (num_samples - u.seg) / u.stride + 1;
  // (UNetModified: the measured tables name UNetModified2's layers, whose names mean other layers here)
  UNetPlanner w{u, u.modified ? nullptr : tuned, k, out};
  return w.walk();
}

// ---------------------------------------------------------------------------------------------
// a plan as seen from outside: the conv geometry and names of a step, and the plan as JSON
// ---------------------------------------------------------------------------------------------
// the geometry fields of a conv step's kernel arguments (no pointers)
static ConvArgs conv_geometry(const UNetPlan& p, const Step& st) {
  auto T = [&](int i) { return i < 0 ? PlanTensor{} : p.tensors[i]; };   // -1: no such source
  const PlanTensor sa = T(st.srcA), sb = T(st.srcB), o = T(st.out);
  ConvArgs a{};
  a.CA = sa.C; a.CB = sb.C; a.Hi = sa.H; a.Wi = sa.W; a.Ho = o.H; a.Wo = o.W; a.upsample = st.up;
  a.Cout = st.cout; a.res_mode = st.res_mode;
  if (st.res_mode == 2) { a.RCA = T(st.rawA).C; a.RCB = T(st.rawB).C; }
  a.TR = st.ch.TR; a.TW = st.ch.TW; a.tiles_x = st.ch.tiles_x; a.n_tiles = st.ch.n_tiles;
  return a;
}

// What the profile shows of a conv op: the tag of its name ("[strip]", "[tile3]", "[deep64_8_32]",
// "[chain]"), the kernel family (the template arguments that pick the tiling) and the exact
// instantiation (the strip kernel's residual mode / GroupNorm and the deep kernel's weight ring
// depth are template arguments the family name leaves out).  tools/traffic.py, tune_deep.py and
// ops_cmp.py parse them.  chain: `a` is the chain's first conv
struct ConvNames { std::string tag, kname, kinst; };
static ConvNames conv_names(int dt, bool s2, const ConvChoice& ch, const ConvArgs& a, bool gn) {
  const int Cin = a.CA + a.CB;
  char kn[160], ki[192];
  std::string tag;
  if (ch.wide) {
    tag = "[wide" + std::to_string(ch.mt) + "]";
    snprintf(kn, sizeof(kn), "conv_wide_kernel<%s,%d>", dt_name(dt), s2 ? 1 : 0);
    snprintf(ki, sizeof(ki), "%s", kn);
  } else if (ch.chain) {
    tag = "[chain]";
    snprintf(kn, sizeof(kn), "conv_chain_kernel<%s,%d,%d,%d>", dt_name(dt), a.Cout, a.Ho, a.Wo);
    snprintf(ki, sizeof(ki), "%s", kn);
  } else if (ch.strip) {
    tag = "[strip]";
    snprintf(kn, sizeof(kn), "conv_strip_kernel<%s,%d,%d,%d,%d>", dt_name(dt), ch.nblk / 16, a.Wo, Cin, ch.mpi);
    snprintf(ki, sizeof(ki), "conv_strip_kernel<%s,%d,%d,%d,%d,%d,%d>", dt_name(dt), ch.nblk / 16, a.Wo, Cin, ch.mpi,
             a.res_mode, gn ? 1 : 0);
  } else if (ch.tile >= 0) {
    tag = "[tile" + std::to_string(ch.tile) + "]";
    const TileCfg tc = conv_tile_cfg(ch.tile);
    snprintf(kn, sizeof(kn), "conv_tile_kernel<%s,%d,%d,%d,%d,%d> (tile%d)", dt_name(dt), s2 ? 1 : 0, tc.wpx, tc.wco, tc.fp,
             tc.fc, ch.tile);
    snprintf(ki, sizeof(ki), "%s", kn);
  } else {
    tag = "[deep" + std::to_string(ch.mt) + "_" + std::to_string(ch.nw) + "_" + std::to_string(ch.nb) + "]";
    snprintf(kn, sizeof(kn), "conv_deep_kernel<%s,%d,%d,%d,%d>", dt_name(dt), s2 ? 1 : 0, ch.mt, ch.nw, ch.nb);
    snprintf(ki, sizeof(ki), "conv_deep_kernel<%s,%d,%d,%d,%d,%d>", dt_name(dt), s2 ? 1 : 0, ch.mt, ch.nw,
             conv_deep_ring_depth(dt, ch.mt, ch.nw, (Cin / 32) * 9 + (a.res_mode == 2 ? (a.RCA + a.RCB) / 32 : 0), ch.nb), ch.nb);
  }
  return {tag, kn, ki};
}

// A plan as a JSON list, one object per step in launch order (sddm_unet_plan).  Every object has the
// layer `name`, the step `type` and, where the step writes one, its `out` tensor with the GroupNorm
// statistics tiling; conv steps carry the kernel family, the geometry and the whole ConvChoice
static std::string plan_json(const UNetPlan& p) {
  static const char* kTypes[] = {"conv_in", "conv", "final", "dual_transformer", "concat", "attention"};
  std::string js = "[";
  char tmp[1024];
  for (size_t i = 0; i < p.steps.size(); ++i) {
    const Step& st = p.steps[i];
    snprintf(tmp, sizeof(tmp), "%s{\"name\": \"%s\", \"type\": \"%s\"", i ? ",\n " : "", st.w.c_str(), kTypes[st.type]);
    js += tmp;
    if (st.out >= 0) {
      const PlanTensor& o = p.tensors[st.out];
      snprintf(tmp, sizeof(tmp), ", \"out\": {\"C\": %d, \"H\": %d, \"W\": %d, \"tiles\": %d, \"n_tile\": %d}", o.C, o.H, o.W,
               o.tiles, o.n_tile);
      js += tmp;
    }
    if (st.type == ST_CONVIN) { snprintf(tmp, sizeof(tmp), ", \"TR\": %d", st.TRin); js += tmp; }
    if (st.type == ST_FINAL) { snprintf(tmp, sizeof(tmp), ", \"FT\": %d", st.FT); js += tmp; }
    if (st.type == ST_ATTN) {
      const PlanTensor& o = p.tensors[st.out];
      snprintf(tmp, sizeof(tmp), ", \"P\": %d, \"C\": %d, \"QT\": %d, \"key_tile\": %d", o.H * o.W, o.C, o.n_tile, kAttnKeyTile);
      js += tmp;
    }
    if (st.type == ST_CONV) {
      const ConvChoice& ch = st.ch;
      const ConvArgs a = conv_geometry(p, st);
      snprintf(tmp, sizeof(tmp),
               ", \"kernel\": \"%s\", \"s2\": %d, \"up\": %d, \"Ho\": %d, \"Wo\": %d, \"CA\": %d, \"CB\": %d, \"Cout\": %d, "
               "\"RCA\": %d, \"RCB\": %d, \"res\": %d, \"gn\": %d, \"TR\": %d, \"TW\": %d, \"tiles_x\": %d, \"n_tiles\": %d, "
               "\"tile\": %d, \"mt\": %d, \"nw\": %d, \"nb\": %d, \"nblk\": %d, \"mpi\": %d, \"SR\": %d",
               ch.wide ? "wide" : ch.chain ? "chain" : ch.strip ? "strip" : ch.tile >= 0 ? "tile" : "deep", st.s2, st.up, a.Ho, a.Wo, a.CA, a.CB,
               a.Cout, a.RCA, a.RCB, a.res_mode, st.gn >= 0 ? 1 : 0, ch.TR, ch.TW, ch.tiles_x, ch.n_tiles, ch.tile, ch.mt, ch.nw,
               ch.nb, ch.nblk, ch.mpi, ch.SR);
      js += tmp;
      if (ch.tile >= 0 && !ch.chain) {
        const TileCfg tc = conv_tile_cfg(ch.tile);
        snprintf(tmp, sizeof(tmp), ", \"wpx\": %d, \"wco\": %d, \"fp\": %d, \"fc\": %d", tc.wpx, tc.wco, tc.fp, tc.fc);
        js += tmp;
      }
    }
    js += "}";
  }
  return js + "]";
}
