// libsddm_hip runtime: context, parameter registry, weight packers (WeightPacker, store_frags, the
// Dual_Transformer's dt_pack) and the C ABI declared in include/sddm_hip.h.  The ABI drives whichever
// network is configured through Net; every network path is one header:
//   UNetModified2, UNetTST, UNetModified  unet_runtime.h   the per-batch plan of one reverse step, run in lanes whose
//                                            step graphs replay concurrently; unet_plan.h is its planner
//                                            (host arithmetic only; sddm_unet_plan returns a plan as JSON)
//   DiffWave             dw_runtime.h  \
//   WaveGrad, DenoiseWaveGrad1 / 3  wg_runtime.h   >  sequential networks: each implements SeqNet, and
//   Waveunet3            wu_runtime.h  |   seq_sample / seq_forward here drive whichever is configured
//   Waveunet2, Waveunet  wu2_runtime.h |
//   CAUNet               cau_runtime.h |
//   TSTNN                tstnn_runtime.h /
// A further sequential network is one such header and one branch on net_type in sddm_configure.
//
// Reference counterparts:
//   sddm_configure      ConfigParser.init_obj('diffusion'|'network'|'arch') (parse_config.py:82-95)
//   sddm_load_param     model.load_state_dict (infer.py:46-51)
//   sddm_sample         SDDM.infer (model/model.py:50-124), SDDM_spectrogram.infer (model.py:212-257)
//   sddm_network_forward the network's forward (e.g. model/UNetModified2.py:237-269)
//   sddm_transition     GaussianDiffusion.p_transition* (model/diffusion.py:164-223)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sddm_hip.h"
#include "json_mini.h"
#include "kernels.h"
#include "dual_transformer.h"
#include "caunet.h"
#include "tstnn.h"
#include "q_kernels.h"
#include "stft_kernels.h"
#include "sddm_common.h"

namespace sddm {
int compute_schedule(const std::string& schedule, int T, double linear_start, double linear_end,
                     float* out);
}
using namespace sddm;

static thread_local std::string g_last_error;
static void sddm_set_error(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  (void)code;
}
#define FAIL(code, ...)                 \
  do {                                  \
    sddm_set_error(code, __VA_ARGS__);  \
    return code;                        \
  } while (0)
#define TRY(x) do { const int _r = (x); if (_r) return _r; } while (0)
#define TRY_LAUNCH(name, x) do { const hipError_t _e = (x); if (_e != hipSuccess) FAIL(SDDM_ERR_HIP, "%s: %s", name, hipGetErrorString(_e)); } while (0)

static const char* kTableNames[14] = {"betas", "alphas", "alpha_bar", "sqrt_alpha_bar",
                                      "predicted_noise_coeff", "sigma", "supportive_gamma",
                                      "supportive_sigma_hat", "m", "sqrt_delta", "c_xt", "c_yt",
                                      "c_epst", "sqrt_delta_estimated"};

// ---------------------------------------------------------------------------------------------
// fp32 -> storage dtype (round to nearest even) on the host
// ---------------------------------------------------------------------------------------------
static uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static uint16_t f32_to_f16_bits(float f) {
  _Float16 h = (_Float16)f;
  uint16_t r;
  std::memcpy(&r, &h, 2);
  return r;
}
static size_t dtype_size(int dt) { return dt == DT_F32 ? 4 : 2; }
static const char* dt_name(int dt) { return dt == DT_F32 ? "f32" : dt == DT_BF16 ? "bf16" : "f16"; }
static void store_elem(void* base, size_t idx, float v, int dt) {
  if (dt == DT_F32) ((float*)base)[idx] = v;
  else if (dt == DT_BF16) ((uint16_t*)base)[idx] = f32_to_bf16_bits(v);
  else ((uint16_t*)base)[idx] = f32_to_f16_bits(v);
}

#include "unet_plan.h"   // the UNet planner: host arithmetic only (TuneTable is part of the context)

// ---------------------------------------------------------------------------------------------
// device arena (one hipMalloc, bump allocation, 256-B alignment)
// ---------------------------------------------------------------------------------------------
struct Arena {
  char* base = nullptr;
  size_t cap = 0, used = 0;
  std::vector<std::pair<size_t, size_t>> pending;  // (offset, bytes) reservations before alloc
  size_t reserve(size_t bytes) {
    const size_t off = (used + 255) & ~(size_t)255;
    used = off + bytes;
    return off;
  }
  hipError_t commit() {
    if (base) { (void)hipFree(base); base = nullptr; }
    cap = used;
    if (cap == 0) return hipSuccess;
    hipError_t e = hipMalloc(&base, cap);
    if (e == hipSuccess) e = hipMemset(base, 0, cap);
    return e;
  }
  void reset() {
    if (base) (void)hipFree(base);
    base = nullptr; cap = used = 0;
  }
  template <typename T> T* at(size_t off) const { return (T*)(base + off); }
};

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
struct Param { std::vector<int64_t> shape; std::vector<float> data; bool loaded = false; };
struct Op {
  int cls;  // 0 conv_in, 1 gn, 2 conv3x3, 3 final, 4 other
  double bytes, flops;
  std::function<hipError_t(hipStream_t, int)> run;   // (stream, flags): flags 0, or a conv's timing ablations (SDDM_REPEAT_FLAGS)
  std::string name = "";
  std::string kname = "";   // kernel family the op launches (template arguments that pick the tiling)
  std::string kinst = "";   // the exact template instantiation (as rocprofv3 lists it), for per-kernel profiles
};
struct ProfAcc { double ms = 0; int64_t n = 0; double bytes = 0, flops = 0; };

struct sddm_ctx;
struct WeightPacker;

// What the C ABI needs from the configured network
struct Net {
  std::map<std::string, std::vector<int64_t>> shapes;  // state-dict shapes (set by sddm_configure)
  virtual ~Net() {}
  // packs the loaded parameters into a new weight arena (ctx->warena), the schedule tables behind them
  virtual int upload_weights(sddm_ctx* c) = 0;
  // the reverse loop: cond as the arch gives it, out [B][1][N]; record (or null) takes x_{t-1} of
  // every t % sample_inter == 0; noise (or null): the caller's draws [T + 1][B][N]
  virtual int sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset, float* out,
                     float* record, int sample_inter, const float* noise, hipStream_t s) = 0;
  // one forward: cond as above, x_t [B][1][N], noise level [B] -> eps [B][1][N]
  virtual int forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B, int64_t N,
                      float* eps_out, hipStream_t s) = 0;
  // the launches of one step as sddm_profile_* reports them (a sequential network has none)
  virtual const std::vector<Op>& ops() const { static const std::vector<Op> kNoOps; return kNoOps; }
  // the context's tuning tables changed: drop what was planned with them
  virtual void replan() {}
};

// A sequential network: its forward is one launch sequence on the caller's stream.  DiffWave
// (dw_runtime.h), the WaveGrad family (wg_runtime.h), Waveunet3 (wu_runtime.h), Waveunet2 and Waveunet
// (wu2_runtime.h), CAUNet (cau_runtime.h) and TSTNN (tstnn_runtime.h) derive from it; seq_sample /
// seq_forward below drive any of them.  UNetModified2 (unet_runtime.h) runs in lanes and graphs instead
struct SeqNet : Net {
  std::map<std::string, size_t> woff;                  // packed weights in ctx->warena
  size_t off_sp = 0, off_rows = 0;                      // StepParams; the path's rows of every t (`pack`)
  Arena act;                                           // activations of the current (B, N)
  int B = -1;
  int64_t N = -1;
  ~SeqNet() override { act.reset(); }
  int upload_weights(sddm_ctx* c) override;
  int sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset, float* out,
             float* record, int sample_inter, const float* noise, hipStream_t s) override;
  int forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B, int64_t N,
              float* eps_out, hipStream_t s) override;
  // packs the weights; returns the bytes of the path's per-t table (embedding / encoding rows of
  // t = 0..T), which lands at off_rows
  virtual size_t pack(sddm_ctx* c, WeightPacker& pk) = 0;
  // shape checks, then the workspace of (B, N); the same (B, N) again: nothing to do
  virtual int prepare(sddm_ctx* c, int64_t B, int64_t N) = 0;
  // step-invariant work of one call at the prepared shape.  noise_level null: the rows of every t
  // (sampling); otherwise [B]: one row per batch item (a forward)
  virtual int begin(sddm_ctx* c, const float* cond, const float* noise_level, hipStream_t s) = 0;
  // one forward: x [B][N] fp32 -> eps().  per_b: the rows of `begin` are per batch item (else row *t_dev)
  virtual int network(sddm_ctx* c, const float* cond, const float* x, int per_b, int* t_dev, hipStream_t s) = 0;
  virtual float* eps() = 0;                            // [B][N] fp32 in the workspace
};

struct sddm_ctx {
  int device = 0, dtype = DT_BF16;
  bool configured = false;
  // arch / diffusion
  std::string arch_type, net_type, p_transition = "original";
  int noise_time_step = 0;
  int tr_mode = SDDM_TR_ORIGINAL, init_mode = 0;
  int T = 0, num_samples = -1;
  std::vector<float> tables;  // [14][T+1]
  bool tables_dirty = true;
  std::map<std::string, Param> params;
  bool params_dirty = true;
  // device state
  Arena warena;      // weights + tables + the network's own blocks (WeightPacker::finish)
  size_t off_tables = 0;
  std::unique_ptr<Net> net;   // the configured network (null: a diffusion-only context)
  // settings of the UNet's lanes (unet_runtime.h); they outlive a re-configure
  int lane_rows = 16;
  bool use_graphs = true;
  // profiling
  unsigned long long* stamp_buf = nullptr;   // SDDM_STAMPS builds: phase stamps of one op
  int64_t stamp_blocks = 0;
  bool prof = false;
  // profiling (sddm_profile_enable): HIP events around every launch, drained after each step of
  // a lane into per-op accumulators, so every launch of a sampling run is timed with a small pool
  std::vector<hipEvent_t> ev_pool;
  std::vector<std::pair<int, int>> ev_pend;   // (op index, pool index of the start event)
  std::vector<ProfAcc> op_acc;                // per op index (the same layer list in every lane)
  // measured per-layer kernel tables (sddm_set_conv_tuning; unet_plan.h)
  std::vector<TuneTable> tunes;
  int hop_samples = 256;

  const float* dtab(int k) const { return warena.at<float>(off_tables) + (size_t)k * (T + 1); }
  TransCoef coef() const {
    TransCoef c;
    c.betas = dtab(0); c.alphas = dtab(1); c.sqrt_alpha_bar = dtab(3); c.pnc = dtab(4);
    c.sigma = dtab(5); c.sgamma = dtab(6); c.ssh = dtab(7); c.sqrt_delta = dtab(9);
    c.c_xt = dtab(10); c.c_yt = dtab(11); c.c_epst = dtab(12); c.sde = dtab(13);
    return c;
  }
};

// ---------------------------------------------------------------------------------------------
// weight upload: pack every layer into the kernels' layouts in the compute dtype.  WeightPacker
// (every network): host images of the blobs, reserved in the weight arena in the order they are
// added and copied in one pass once the arena is allocated
// ---------------------------------------------------------------------------------------------
struct WeightPacker {
  struct Blob { size_t off; std::vector<char> bytes; };
  sddm_ctx* c;
  std::map<std::string, size_t>& woff;   // blob name -> offset in c->warena
  std::vector<Blob> blobs;
  WeightPacker(sddm_ctx* ctx, std::map<std::string, size_t>& offsets) : c(ctx), woff(offsets) {
    c->warena.reset();
    woff.clear();
  }
  // a zero-filled image of `bytes` bytes that the caller fills with store_elem (the kernel families'
  // own conv layouts); the pointer holds until finish (a moved vector keeps its buffer)
  char* raw(const std::string& name, size_t bytes) {
    Blob b;
    b.bytes.assign(bytes, 0);
    b.off = c->warena.reserve(bytes);
    woff[name] = b.off;
    blobs.push_back(std::move(b));
    return blobs.back().bytes.data();
  }
  void f32(const std::string& name, const std::vector<float>& v) { std::memcpy(raw(name, v.size() * 4), v.data(), v.size() * 4); }
  void typed(const std::string& name, const std::vector<float>& v) {   // compute dtype
    char* p = raw(name, v.size() * dtype_size(c->dtype));
    for (size_t i = 0; i < v.size(); ++i) store_elem(p, i, v[i], c->dtype);
  }
  // after the last blob: the 14 schedule tables, the step parameters (`sp_bytes`) and, if it has
  // any bytes, one more block of the caller's; allocate, copy the blobs, mark the tables for upload
  int finish(size_t sp_bytes, size_t* off_sp, size_t more_bytes, size_t* off_more) {
    Arena& A = c->warena;
    c->off_tables = A.reserve(sizeof(float) * 14 * (c->T + 1));
    *off_sp = A.reserve(sp_bytes);
    if (more_bytes) *off_more = A.reserve(more_bytes);
    SDDM_HIP_CHECK(A.commit());
    for (const auto& b : blobs) SDDM_HIP_CHECK(hipMemcpy(A.base + b.off, b.bytes.data(), b.bytes.size(), hipMemcpyHostToDevice));
    c->params_dirty = false;
    c->tables_dirty = true;
    return SDDM_OK;
  }
};

// W[N][K] (row-major, torch's [out][in]) -> MFMA A fragments [N / 16][ceil(K / 32)][64 lanes][8] at
// element `off` of the zero-filled image `dst`: lane l of fragment (nt, kc) holds
// W[16 nt + (l & 15)][32 kc + 8 (l >> 4) + j], j = 0..7 (zero where k >= K)
static void store_frags(void* dst, size_t off, const float* w, int N, int K, int dt) {
  const int KC = (K + 31) / 32;
  for (int o = 0; o < N; ++o)
    for (int k = 0; k < K; ++k)
      store_elem(dst, off + ((size_t)((o / 16) * KC + k / 32) * 64 + (o % 16) + 16 * ((k % 32) / 8)) * 8 + k % 8, w[(size_t)o * K + k], dt);
}

// ---------------------------------------------------------------------------------------------
// Dual_Transformer(C, C, 0, n_tstb), the mid block of UNetTST (UNetTST.py:184-210) and of CAUNet
// (CAUNet.py:152-178) and TSTNN's dual_transformer (tstnn.py:114-141): state-dict shapes and weight
// packing, d_model = C / 2, GRU hidden C
// ---------------------------------------------------------------------------------------------
// The block's two PReLUs.  Shared: input.1 / output.1 hold one slope in all (UNetTST).  PerChannel:
// one slope per channel (CAUNet).  SharedFirst: one slope each and output = (PReLU, Conv2d), so the
// keys are output.0.weight [1], output.1.weight, output.1.bias (TSTNN); dt_pack broadcasts the two
// slopes into the layout's per-channel slots
enum DtPrelu { kDtPreluShared = 0, kDtPreluPerChannel = 1, kDtPreluSharedFirst = 2 };
static void dt_param_shapes(std::map<std::string, std::vector<int64_t>>& s, const std::string& n, int64_t C, int n_tstb,
                            DtPrelu prelu) {
  const int64_t d = C / 2;
  const bool per_channel = prelu == kDtPreluPerChannel;
  const char* oc = prelu == kDtPreluSharedFirst ? ".output.1" : ".output.0";   // the output conv, and its PReLU
  const char* op = prelu == kDtPreluSharedFirst ? ".output.0" : ".output.1";
  s[n + ".input.0.weight"] = {d, C, 1, 1}; s[n + ".input.0.bias"] = {d}; s[n + ".input.1.weight"] = {per_channel ? d : 1};
  s[n + oc + ".weight"] = {C, d, 1, 1}; s[n + oc + ".bias"] = {C}; s[n + op + ".weight"] = {per_channel ? C : 1};
  for (int i = 0; i < n_tstb; ++i)
    for (const char* pass : {"row", "col"}) {
      const std::string e = n + "." + pass + "_trans." + std::to_string(i);
      s[e + ".self_attn.in_proj_weight"] = {3 * d, d}; s[e + ".self_attn.in_proj_bias"] = {3 * d};
      s[e + ".self_attn.out_proj.weight"] = {d, d}; s[e + ".self_attn.out_proj.bias"] = {d};
      for (const char* sfx : {"", "_reverse"}) {
        s[e + ".gru.weight_ih_l0" + sfx] = {6 * d, d}; s[e + ".gru.weight_hh_l0" + sfx] = {6 * d, 2 * d};
        s[e + ".gru.bias_ih_l0" + sfx] = {6 * d}; s[e + ".gru.bias_hh_l0" + sfx] = {6 * d};
      }
      s[e + ".linear2.weight"] = {d, 4 * d}; s[e + ".linear2.bias"] = {d};
      for (const char* nm : {".norm1", ".norm2"}) { s[e + nm + ".weight"] = {d}; s[e + nm + ".bias"] = {d}; }
      const std::string gn = n + "." + pass + "_norm." + std::to_string(i);
      s[gn + ".weight"] = {d}; s[gn + ".bias"] = {d};
    }
}

// where a kernel family expects the block's weights: element offsets into the matrix blob (compute
// dtype, every matrix as store_frags) and into the vector blob (fp32), per encoder from WEnc0 / VEnc0
// in steps of EncW / EncV.  The kernels' headers define them; the two instances restate those names
struct DtLayout {
  int C, D, Hid;
  int WIn, WOut, WEnc0, EInProj, EOutProj, EIh, EIhSize, EHh, EHhSize, ELin2, EncW;
  int VInB, VInA, VOutB, VOutA, VEnc0;
  int VInProjB, VOutProjB, VLn1W, VLn1B, VBih, VBhh, VLin2B, VLn2W, VLn2B, VGnW, VGnB, EncV;
};
static const DtLayout kTstLayout = {   // dual_transformer.h
    kTstC, kTstD, kTstHid,
    kTstWIn, kTstWOut, kTstWEnc0, kTstEInProj, kTstEOutProj, kTstEIh, kTstEIhSize, kTstEHh, kTstEHhSize, kTstELin2, kTstEncW,
    kTstVInB, kTstVInA, kTstVOutB, kTstVOutA, kTstVEnc0,
    kTstVInProjB, kTstVOutProjB, kTstVLn1W, kTstVLn1B, kTstVBih, kTstVBhh, kTstVLin2B, kTstVLn2W, kTstVLn2B, kTstVGnW, kTstVGnB,
    kTstEncV};
static const DtLayout kCauLayout = {   // caunet.h
    kCauC, kCauD, kCauHid,
    kCauWIn, kCauWOut, kCauWEnc0, kCauEInProj, kCauEOutProj, kCauEIh, kCauEIhSize, kCauEHh, kCauEHhSize, kCauELin2, kCauEncW,
    kCauVInB, kCauVInA, kCauVOutB, kCauVOutA, kCauVEnc0,
    kCauVInProjB, kCauVOutProjB, kCauVLn1W, kCauVLn1B, kCauVBih, kCauVBhh, kCauVLin2B, kCauVLn2W, kCauVLn2B, kCauVGnW, kCauVGnB,
    kCauEncV};

// packs the block `n` ("mid") as the blobs n.wmat and n.wvec
static void dt_pack(sddm_ctx* c, WeightPacker& pk, const std::string& n, const DtLayout& L, int n_tstb, DtPrelu prelu) {
  const int dt = c->dtype, ne = 2 * n_tstb;
  auto P = [&](const std::string& k) -> const std::vector<float>& { return c->params.at(k).data; };
  char* wm = pk.raw(n + ".wmat", ((size_t)L.WEnc0 + (size_t)ne * L.EncW) * dtype_size(dt));
  std::vector<float> wv((size_t)L.VEnc0 + (size_t)ne * L.EncV, 0.f);
  auto frag = [&](size_t off, const std::vector<float>& w, int N, int K) { store_frags(wm, off, w.data(), N, K, dt); };
  auto vec = [&](size_t off, const std::vector<float>& v) { std::copy(v.begin(), v.end(), wv.begin() + off); };
  frag(L.WIn, P(n + ".input.0.weight"), L.D, L.C);
  vec(L.VInB, P(n + ".input.0.bias"));
  if (prelu == kDtPreluSharedFirst) {
    frag(L.WOut, P(n + ".output.1.weight"), L.C, L.D);
    vec(L.VOutB, P(n + ".output.1.bias"));
    vec(L.VInA, std::vector<float>(L.D, P(n + ".input.1.weight")[0]));
    vec(L.VOutA, std::vector<float>(L.C, P(n + ".output.0.weight")[0]));   // the conv's D inputs read the first D
  } else {
    frag(L.WOut, P(n + ".output.0.weight"), L.C, L.D);
    vec(L.VOutB, P(n + ".output.0.bias"));
    vec(L.VInA, P(n + ".input.1.weight"));
    vec(L.VOutA, P(n + ".output.1.weight"));
  }
  for (int e = 0; e < ne; ++e) {
    const char* pass = e % 2 ? "col" : "row";
    const std::string p = n + "." + pass + "_trans." + std::to_string(e / 2);
    const std::string gn = n + "." + pass + "_norm." + std::to_string(e / 2);
    const size_t wo = (size_t)L.WEnc0 + (size_t)e * L.EncW, vo = (size_t)L.VEnc0 + (size_t)e * L.EncV;
    frag(wo + L.EInProj, P(p + ".self_attn.in_proj_weight"), 3 * L.D, L.D);
    frag(wo + L.EOutProj, P(p + ".self_attn.out_proj.weight"), L.D, L.D);
    for (int d = 0; d < 2; ++d) {                      // forward, reverse (a direction's bias vector: 6 Hid)
      const std::string sfx = d ? "_reverse" : "";
      frag(wo + L.EIh + (size_t)d * L.EIhSize, P(p + ".gru.weight_ih_l0" + sfx), 3 * L.Hid, L.D);
      frag(wo + L.EHh + (size_t)d * L.EHhSize, P(p + ".gru.weight_hh_l0" + sfx), 3 * L.Hid, L.Hid);
      vec(vo + L.VBih + 6 * L.Hid * d, P(p + ".gru.bias_ih_l0" + sfx));
      vec(vo + L.VBhh + 6 * L.Hid * d, P(p + ".gru.bias_hh_l0" + sfx));
    }
    frag(wo + L.ELin2, P(p + ".linear2.weight"), L.D, 2 * L.Hid);
    vec(vo + L.VInProjB, P(p + ".self_attn.in_proj_bias"));
    vec(vo + L.VOutProjB, P(p + ".self_attn.out_proj.bias"));
    vec(vo + L.VLn1W, P(p + ".norm1.weight"));
    vec(vo + L.VLn1B, P(p + ".norm1.bias"));
    vec(vo + L.VLin2B, P(p + ".linear2.bias"));
    vec(vo + L.VLn2W, P(p + ".norm2.weight"));
    vec(vo + L.VLn2B, P(p + ".norm2.bias"));
    vec(vo + L.VGnW, P(gn + ".weight"));
    vec(vo + L.VGnB, P(gn + ".bias"));
  }
  pk.f32(n + ".wvec", wv);
}

static int upload_tables(sddm_ctx* c) {
  SDDM_HIP_CHECK(hipMemcpy(c->warena.base + c->off_tables, c->tables.data(), sizeof(float) * c->tables.size(),
                           hipMemcpyHostToDevice));
  c->tables_dirty = false;
  return SDDM_OK;
}

// the schedule tables on the device for an entry point that needs no network (a transition, q_sample,
// the initial state): where no weights were uploaded yet, an arena of the tables alone
static int ensure_tables(sddm_ctx* c) {
  if (!c->warena.base) {
    c->warena.reset();
    c->off_tables = c->warena.reserve(sizeof(float) * 14 * (c->T + 1));
    SDDM_HIP_CHECK(c->warena.commit());
    c->params_dirty = true;
    c->tables_dirty = true;
  }
  if (c->tables_dirty) TRY(upload_tables(c));
  return SDDM_OK;
}

static constexpr size_t kStampBytes = sizeof(unsigned long long) * 8 * 65536;
// SDDM_STAMPS builds: *stamps = the context's stamp buffer (allocated at its first use) if the
// environment variable SDDM_STAMPS names `op`; otherwise, and in every other build, it stays null
static int stamp_buffer(sddm_ctx* c, const std::string& op, unsigned long long** stamps) {
#ifdef SDDM_STAMPS
  const char* sn = std::getenv("SDDM_STAMPS");
  if (!sn || op != sn) return SDDM_OK;
  if (!c->stamp_buf) SDDM_HIP_CHECK(hipMalloc(&c->stamp_buf, kStampBytes));
  *stamps = c->stamp_buf;
#endif
  return SDDM_OK;
}

// ---------------------------------------------------------------------------------------------
// sequential networks: weight upload, the reverse loop and the forward of any SeqNet
// ---------------------------------------------------------------------------------------------
static int seq_upload_weights(sddm_ctx* c, SeqNet& n) {
  WeightPacker pk(c, n.woff);
  const size_t rows_bytes = n.pack(c, pk);
  n.B = -1;                                            // the next call prepares its workspace anew
  return pk.finish(64, &n.off_sp, rows_bytes, &n.off_rows);
}

// The reverse loop.  SDDM_spectrogram.infer (model.py:212-257): cond = spectrogram [B][bins][F],
// x_T = randn, p_transition 'original' (the context's init / transition modes are those).  SDDM.infer
// (model.py:50-124): cond = waveform [B][1][N], the initial state and the transition of the
// context's p_transition.  out [B][1][N]
static int seq_sample(sddm_ctx* c, SeqNet& n, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset,
                      float* out, float* record, int sample_inter, const float* noise, hipStream_t s) {
  TRY(n.prepare(c, B, N));
  TRY(n.begin(c, cond, nullptr, s));
  const int T = c->T;
  const float* wave = c->arch_type == "SDDM" ? cond : nullptr;   // the condition as a waveform, or none
  InitArgs ia{};                                       // x_T (model.py:57-68, 216)
  ia.mode = c->init_mode; ia.cond = wave; ia.out = out; ia.total = B * N; ia.N = N; ia.T = T;
  ia.co = c->coef(); ia.seed = seed; ia.row_offset = row_offset; ia.noise = noise;
  SDDM_HIP_CHECK(launch_init_state(ia, s));
  StepParams* sp = c->warena.at<StepParams>(n.off_sp);
  SDDM_HIP_CHECK(launch_set_params(sp, T + 1, seed, row_offset, s));
  int64_t nrec = 0;
  for (int t = T; t >= 1; --t) {
    TRY(n.network(c, cond, out, 0, &sp->t, s));
    TransArgs ta{};                                    // p_transition* (diffusion.py:164-223)
    ta.mode = c->tr_mode; ta.x_t = out; ta.eps = n.eps(); ta.cond = wave; ta.out = out;
    ta.total = B * N; ta.N = N; ta.t = t; ta.t_dev = &sp->t; ta.co = c->coef(); ta.seed = seed; ta.row_offset = row_offset;
    ta.noise = noise; ta.noise_ld = B * N;
    SDDM_HIP_CHECK(launch_transition(ta, s));
    if (record && t % sample_inter == 0) {             // model.py:100-101: keep x_{t-1} when t % inter == 0
      SDDM_HIP_CHECK(hipMemcpyAsync(record + nrec * B * N, out, sizeof(float) * B * N, hipMemcpyDeviceToDevice, s));
      ++nrec;
    }
  }
  return SDDM_OK;
}

// one forward: cond as above, x_t [B][1][N], noise level [B] -> eps [B][1][N]
static int seq_forward(sddm_ctx* c, SeqNet& n, const float* cond, const float* x_t, const float* noise_level, int64_t B,
                       int64_t N, float* eps_out, hipStream_t s) {
  TRY(n.prepare(c, B, N));
  TRY(n.begin(c, cond, noise_level, s));
  TRY(n.network(c, cond, x_t, 1, nullptr, s));
  SDDM_HIP_CHECK(hipMemcpyAsync(eps_out, n.eps(), sizeof(float) * B * N, hipMemcpyDeviceToDevice, s));
  return SDDM_OK;
}

int SeqNet::upload_weights(sddm_ctx* c) { return seq_upload_weights(c, *this); }
int SeqNet::sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset, float* out,
                   float* record, int sample_inter, const float* noise, hipStream_t s) {
  return seq_sample(c, *this, cond, B, N, seed, row_offset, out, record, sample_inter, noise, s);
}
int SeqNet::forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B, int64_t N,
                    float* eps_out, hipStream_t s) {
  return seq_forward(c, *this, cond, x_t, noise_level, B, N, eps_out, s);
}

#include "dw_runtime.h"
#include "wg_runtime.h"
#include "wu_runtime.h"
#include "wu2_runtime.h"
#include "cau_runtime.h"
#include "tstnn_runtime.h"
#include "unet_runtime.h"

// =============================================================================================
// C ABI
// =============================================================================================
static int ensure_ready(sddm_ctx* c) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (c->net_type.empty()) FAIL(SDDM_ERR_STATE, "context has no network (diffusion-only)");
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  for (const auto& kv : c->params)
    if (!kv.second.loaded) FAIL(SDDM_ERR_STATE, "parameter %s not loaded", kv.first.c_str());
  if (c->params_dirty) TRY(c->net->upload_weights(c));
  if (c->tables_dirty) TRY(upload_tables(c));
  return SDDM_OK;
}

extern "C" {

int sddm_abi_version(void) { return SDDM_ABI_VERSION; }
const char* sddm_last_error(void) { return g_last_error.c_str(); }

int sddm_create(int device, int compute_dtype, sddm_ctx** out) {
  if (!out) FAIL(SDDM_ERR_INVALID_ARG, "out is NULL");
  if (compute_dtype < 0 || compute_dtype > 2) FAIL(SDDM_ERR_INVALID_ARG, "bad dtype %d", compute_dtype);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
    FAIL(SDDM_ERR_HIP, "no HIP device %d (count %d)", device, n);
  int lds = 0;
  if (hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess || lds < kLdsBytes)
    FAIL(SDDM_ERR_HIP, "device %d offers %d bytes of LDS per workgroup; the kernels are planned for %d (gfx950)", device,
         lds, kLdsBytes);
  sddm_ctx* c = new sddm_ctx();
  c->device = device;
  c->dtype = compute_dtype;
  c->use_graphs = std::getenv("SDDM_NO_GRAPH") == nullptr;
  if (const char* lr = std::getenv("SDDM_LANE_ROWS")) c->lane_rows = std::max(1, std::atoi(lr));
  *out = c;
  return SDDM_OK;
}

void sddm_destroy(sddm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->net.reset();
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  c->warena.reset();
  delete c;
}

int sddm_schedule(const char* schedule, int n_timestep, double linear_start, double linear_end, float* out) {
  if (!schedule || !out || n_timestep < 1) FAIL(SDDM_ERR_INVALID_ARG, "bad schedule arguments");
  if (compute_schedule(schedule, n_timestep, linear_start, linear_end, out))
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "schedule '%s'", schedule);
  return SDDM_OK;
}

// the common ending of sddm_configure: the schedule, the parameter registry of `shapes` (all
// unloaded), the network (null: none) and a weight arena to be rebuilt
static int finish_configure(sddm_ctx* c, int T, std::vector<float>& tabs, const std::map<std::string, std::vector<int64_t>>& shapes,
                            std::unique_ptr<Net> net, int num_samples) {
  c->T = T;
  c->tables.swap(tabs);
  c->tables_dirty = true;
  c->num_samples = num_samples;
  c->params.clear();
  for (const auto& kv : shapes) c->params[kv.first].shape = kv.second;
  c->net = std::move(net);
  if (c->net) c->net->shapes = shapes;
  c->params_dirty = true;
  c->warena.reset();
  c->configured = true;
  return SDDM_OK;
}

// a network runs under one arch: SDDM.infer feeds it a waveform, SDDM_spectrogram.infer a spectrogram
static int needs_arch(const sddm_ctx* c, const char* net, const char* arch) {
  if (c->arch_type != arch)
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "%s needs arch %s%s", net, arch, std::strcmp(arch, "SDDM") ? "" : " (its condition is a waveform)");
  return SDDM_OK;
}

int sddm_configure(sddm_ctx* c, const char* json) {
  if (!c || !json) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  Json cfg;
  try {
    cfg = Json::parse(json);
  } catch (const std::exception& e) {
    FAIL(SDDM_ERR_INVALID_ARG, "config JSON: %s", e.what());
  }
  const Json& arch = cfg.at("arch");
  const Json& diff = cfg.at("diffusion");
  const Json& net = cfg.at("network");
  c->arch_type = arch.string("type", "SDDM");
  // rows per lane ("lane_rows", default 16; SDDM_LANE_ROWS overrides).  Every lane's kernels are
  // chosen for lane_rows rows, so any row partition samples bit-identically; larger lanes give the
  // latency-bound deep levels bigger grids for large per-GPU batches (config #5, B=128 per GPU:
  // lanes of 64 sample 1.18x faster than lanes of 16) but grids sized for 64 rows underfill a
  // 16-row batch (the config #2 headline ran 0.62x as fast on them)
  if (!std::getenv("SDDM_LANE_ROWS")) {
    const int lr = (int)cfg.number("lane_rows", 16);
    if (lr < 1) FAIL(SDDM_ERR_INVALID_ARG, "lane_rows %d", lr);
    c->lane_rows = lr;
    if (c->net) c->net->replan();
  }
  const Json& aa = arch.at("args");
  const std::string nc = aa.string("noise_condition", "sqrt_alpha_bar");
  if (nc != "sqrt_alpha_bar" && nc != "time_step") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "noise_condition '%s'", nc.c_str());
  c->noise_time_step = nc == "time_step";
  if (c->arch_type == "SDDM") {
    const std::string pt = aa.string("p_transition", "original");
    const std::string qt = aa.string("q_transition", "original");
    if (pt == "original") { c->tr_mode = SDDM_TR_ORIGINAL; c->init_mode = 0; }
    else if (pt == "condition_in") { c->tr_mode = SDDM_TR_ORIGINAL; c->init_mode = 4; }
    else if (pt == "sr3") { c->tr_mode = SDDM_TR_SR3; c->init_mode = 1; }
    else if (pt == "supportive") { c->tr_mode = SDDM_TR_SUPPORTIVE; c->init_mode = 2; }
    else if (pt == "conditional") { c->tr_mode = SDDM_TR_CONDITIONAL; c->init_mode = 3; }
    else FAIL(SDDM_ERR_NOT_IMPLEMENTED, "p_transition '%s' (model.py:20-23)", pt.c_str());
    if (qt != "original" && qt != "conditional") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "q_transition '%s'", qt.c_str());
    c->p_transition = pt;
  } else if (c->arch_type == "SDDM_spectrogram") {              // model.py:206-257
    c->tr_mode = SDDM_TR_ORIGINAL;
    c->init_mode = 0;
    c->p_transition = "original";
    c->hop_samples = (int)aa.number("hop_samples", 256);          // SURVEY Q6 default
    if (c->hop_samples < 1) FAIL(SDDM_ERR_INVALID_ARG, "hop_samples %d", c->hop_samples);
  } else {
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "arch type '%s'", c->arch_type.c_str());
  }
  if (diff.string("type", "GaussianDiffusion") != "GaussianDiffusion")
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "diffusion type '%s'", diff.string("type", "").c_str());
  const Json& da = diff.at("args");
  const std::string sched = da.string("schedule", "linear");
  const int T = (int)da.number("n_timestep", 1000);
  const double ls = da.number("linear_start", 1e-4), le = da.number("linear_end", 2e-2);
  if (T < 1) FAIL(SDDM_ERR_INVALID_ARG, "n_timestep %d", T);
  std::vector<float> tabs((size_t)14 * (T + 1));
  if (compute_schedule(sched, T, ls, le, tabs.data())) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "schedule '%s' (diffusion.py:84)", sched.c_str());
  c->net_type = net.string("type", "");
  if (c->net_type.empty())    // diffusion-only context: transitions / initial state
    return finish_configure(c, T, tabs, {}, nullptr, c->num_samples);
  if (c->net_type == "DiffWave") {                               // diffwave.py:113-131
    TRY(needs_arch(c, "DiffWave", "SDDM_spectrogram"));
    const Json& na = net.at("args");
    auto d = std::make_unique<DWState>();
    d->C = (int)na.number("residual_channels", 64);
    d->L = (int)na.number("residual_layers", 30);
    d->cycle = (int)na.number("dilation_cycle_length", 10);
    d->bins = (int)na.number("freq_bins", na.number("stft_bins", na.number("n_mels", 513)));
    d->hop = c->hop_samples;
    d->Kp = (d->bins + 31) / 32 * 32;
    if (d->C != 64) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "DiffWave residual_channels %d (kernels are built for 64)", d->C);
    if (d->L < 1 || d->cycle < 1 || d->bins < 1) FAIL(SDDM_ERR_INVALID_ARG, "DiffWave geometry");
    if (d->hop != 256) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "hop_samples %d: SpectrogramUpsampler upsamples x256", d->hop);
    const auto shapes = dw_param_shapes(*d);
    finish_configure(c, T, tabs, shapes, std::move(d), -1);
    c->params["diffusion_embedding.embedding_vector"].loaded = true;   // optional (default computed)
    return SDDM_OK;
  }
  if (const wg::Variant* wv = wg::find_variant(c->net_type)) {   // wavegrad.py:140-179, 184-242, 307-353
    if (wv->kind == wg::kWaveGrad) {
      TRY(needs_arch(c, "WaveGrad", "SDDM_spectrogram"));
      if (c->hop_samples != wv->hop)
        FAIL(SDDM_ERR_NOT_IMPLEMENTED, "hop_samples %d: WaveGrad upsamples x300 (config_wavegrad.json:8)", c->hop_samples);
    } else {                                                     // waveform-conditioned: SDDM.infer (model.py:50-124)
      TRY(needs_arch(c, wv->name, "SDDM"));
      c->hop_samples = wv->hop;
    }
    auto ws = std::make_unique<WGState>();
    ws->v = wv;
    return finish_configure(c, T, tabs, wg_param_shapes(*wv), std::move(ws), -1);
  }
  if (c->net_type == "Waveunet3") {                              // waveunet3.py:314-416, config_waveunet3.json
    TRY(needs_arch(c, "Waveunet3", "SDDM"));
    TRY(wu_check_config(net.at("args")));
    auto us = std::make_unique<WUState>();
    const auto shapes = wu_param_shapes(us->net);
    return finish_configure(c, T, tabs, shapes, std::move(us), -1);
  }
  if (const wu2::Net* wn = wu2::find_net(c->net_type)) {         // waveunet2.py:226-324, waveunet.py:358-506
    TRY(needs_arch(c, wn->name, "SDDM"));
    TRY(wn->check_config(net.at("args")));
    auto us = std::make_unique<WUFilmState>(*wn);
    const auto shapes = wu2_param_shapes(*us);
    return finish_configure(c, T, tabs, shapes, std::move(us), -1);
  }
  if (c->net_type == "CAUNet") {                                 // CAUNet.py:307-374, config_caunet.json
    TRY(needs_arch(c, "CAUNet", "SDDM"));
    auto us = std::make_unique<CAUState>();
    TRY(cau_check_config(net.at("args"), *us));
    const auto shapes = cau_param_shapes(*us);
    return finish_configure(c, T, tabs, shapes, std::move(us), -1);
  }
  if (c->net_type == "TSTNN") {                                  // tstnn.py:216-299, config_tstnn.json
    TRY(needs_arch(c, "TSTNN", "SDDM"));
    auto us = std::make_unique<TSTNNState>();
    TRY(tstnn_check_config(net.at("args"), *us));
    const auto shapes = tstnn_param_shapes(*us);
    return finish_configure(c, T, tabs, shapes, std::move(us), -1);
  }
  // UNetTST (UNetTST.py:270-392): UNetModified2 with mid = Dual_Transformer and no final Swish in the noise MLP
  // UNetModified (UNetModified.py:192-323): the SR3-style U-Net with SelfAttention at the levels of attn_layer
  const bool tst = c->net_type == "UNetTST", modified = c->net_type == "UNetModified";
  if (c->net_type != "UNetModified2" && !tst && !modified) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "network type '%s'", c->net_type.c_str());
  if (c->arch_type != "SDDM") FAIL(SDDM_ERR_NOT_IMPLEMENTED, "%s under arch '%s'", c->net_type.c_str(), c->arch_type.c_str());
  auto us = std::make_unique<UNetState>();
  int Ns = -1;
  TRY(unet_configure(cfg, net.at("args"), tst, us->u, &Ns, modified));
  const auto shapes = unet_param_shapes(us->u);
  return finish_configure(c, T, tabs, shapes, std::move(us), Ns);
}

int sddm_load_param(sddm_ctx* c, const char* key_c, const void* host_ptr, const int64_t* shape, int ndim,
                    int src_dtype) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (!key_c || !host_ptr || (ndim > 0 && !shape)) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  std::string key = key_c;
  if (key.rfind("module.", 0) == 0) key = key.substr(7);
  int64_t n = 1;
  for (int i = 0; i < ndim; ++i) n *= shape[i];
  auto read = [&](std::vector<float>& dst) -> int {
    dst.resize((size_t)n);
    if (src_dtype == DT_F32) std::memcpy(dst.data(), host_ptr, sizeof(float) * n);
    else if (src_dtype == DT_BF16) {
      for (int64_t i = 0; i < n; ++i) {
        uint32_t u = (uint32_t)((const uint16_t*)host_ptr)[i] << 16;
        std::memcpy(&dst[i], &u, 4);
      }
    } else if (src_dtype == DT_F16) {
      for (int64_t i = 0; i < n; ++i) dst[i] = (float)((const _Float16*)host_ptr)[i];
    } else {
      return 1;
    }
    return 0;
  };
  if (key.rfind("diffusion.", 0) == 0) {
    const std::string name = key.substr(10);
    for (int k = 0; k < 14; ++k)
      if (name == kTableNames[k]) {
        if (ndim != 1 || shape[0] != c->T + 1)
          FAIL(SDDM_ERR_SHAPE, "%s: expected [%d]", key.c_str(), c->T + 1);
        std::vector<float> v;
        if (read(v)) FAIL(SDDM_ERR_INVALID_ARG, "bad src dtype %d", src_dtype);
        std::memcpy(c->tables.data() + (size_t)k * (c->T + 1), v.data(), sizeof(float) * v.size());
        c->tables_dirty = true;
        return SDDM_OK;
      }
    FAIL(SDDM_ERR_INVALID_ARG, "unexpected key %s", key.c_str());
  }
  if (key.rfind("noise_estimate_model.", 0) == 0) key = key.substr(21);
  auto it = c->params.find(key);
  if (it == c->params.end()) FAIL(SDDM_ERR_INVALID_ARG, "unexpected key %s", key_c);
  Param& p = it->second;
  if ((int)p.shape.size() != ndim) FAIL(SDDM_ERR_SHAPE, "%s: rank %d != %d", key_c, ndim, (int)p.shape.size());
  for (int i = 0; i < ndim; ++i)
    if (p.shape[i] != shape[i]) FAIL(SDDM_ERR_SHAPE, "%s: shape mismatch in dim %d", key_c, i);
  if (read(p.data)) FAIL(SDDM_ERR_INVALID_ARG, "bad src dtype %d", src_dtype);
  p.loaded = true;
  c->params_dirty = true;
  return SDDM_OK;
}

int sddm_missing_params(sddm_ctx* c, int64_t* n_missing) {
  if (!c || !n_missing) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  int64_t m = 0;
  for (const auto& kv : c->params) m += kv.second.loaded ? 0 : 1;
  *n_missing = m;
  return SDDM_OK;
}

static int sample_impl(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset,
                       float* out, float* record, int sample_inter, void* stream, const float* noise = nullptr) {
  TRY(ensure_ready(c));
  if (!cond || !out) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  return c->net->sample(c, cond, B, N, seed, row_offset, out, record, sample_inter, noise, (hipStream_t)stream);
}

int sddm_sample(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed, int64_t row_offset,
                float* out, void* stream) {
  return sample_impl(c, cond, B, N, seed, row_offset, out, nullptr, 0, stream);
}

int sddm_sample_noise(sddm_ctx* c, const float* cond, int64_t B, int64_t N, const float* noise, float* out,
                      void* stream) {
  if (!noise) FAIL(SDDM_ERR_INVALID_ARG, "NULL noise");
  return sample_impl(c, cond, B, N, 0, 0, out, nullptr, 0, stream, noise);
}

int sddm_sample_continuous(sddm_ctx* c, const float* cond, int64_t B, int64_t N, uint64_t seed,
                           int64_t row_offset, float* out, float* record, int sample_inter, void* stream) {
  if (!record || sample_inter < 1) FAIL(SDDM_ERR_INVALID_ARG, "record buffer / sample_inter");
  return sample_impl(c, cond, B, N, seed, row_offset, out, record, sample_inter, stream);
}

int sddm_network_forward(sddm_ctx* c, const float* cond, const float* x_t, const float* noise_level, int64_t B,
                         int64_t N, float* eps_out, void* stream) {
  TRY(ensure_ready(c));
  if (!cond || !x_t || !noise_level || !eps_out) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  return c->net->forward(c, cond, x_t, noise_level, B, N, eps_out, (hipStream_t)stream);
}

// The Dual_Transformer of a UNetTST, CAUNet or TSTNN context alone (UNetTST.py:212-233,
// CAUNet.py:180-201, tstnn.py:143-164).  Only the block's parameters (mid.*; TSTNN: dual_transformer.*)
// need to be loaded: parameters outside it that are still missing are packed as zeros
int sddm_dual_transformer(sddm_ctx* c, const float* in, int64_t B, int64_t dim2, int64_t dim1, float* out, void* stream) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  const bool tstnn = c->net_type == "TSTNN", cau = c->net_type == "CAUNet" || tstnn;   // cau: caunet.hip's kernels
  if (c->net_type != "UNetTST" && !cau) FAIL(SDDM_ERR_STATE, "sddm_dual_transformer needs a context configured for UNetTST, CAUNet or TSTNN");
  const std::string blk = tstnn ? "dual_transformer" : "mid";
  if (!in || !out) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  if (B < 1 || B > 65535 || dim2 < 1 || dim1 < 1) FAIL(SDDM_ERR_INVALID_ARG, "shape B=%lld dim2=%lld dim1=%lld", (long long)B, (long long)dim2, (long long)dim1);
  if (!cau && dim2 * dim1 > kTstMaxTokens)
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "dim2 * dim1 = %lld tokens: the Dual_Transformer kernel holds %d", (long long)(dim2 * dim1), kTstMaxTokens);
  if (cau && (dim2 > (1 << 20) || dim1 > (1 << 20) || B * dim2 * dim1 > ((int64_t)1 << 24)))
    FAIL(SDDM_ERR_SHAPE, "B * dim2 * dim1 = %lld tokens: the Dual_Transformer kernels index 2^24", (long long)(B * dim2 * dim1));
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  for (auto& kv : c->params) {
    if (kv.second.loaded) continue;
    if (kv.first.rfind(blk + ".", 0) == 0) FAIL(SDDM_ERR_STATE, "parameter %s not loaded", kv.first.c_str());
    int64_t n = 1;
    for (int64_t d : kv.second.shape) n *= d;
    if ((int64_t)kv.second.data.size() != n) kv.second.data.assign((size_t)n, 0.f);
  }
  if (c->params_dirty) TRY(c->net->upload_weights(c));
  if (c->tables_dirty) TRY(upload_tables(c));
  hipStream_t s = (hipStream_t)stream;
  const int P = (int)(dim2 * dim1), C = cau ? kCauC : kTstC;
  const size_t bytes = ((size_t)B * P * C * dtype_size(c->dtype) + 255) & ~(size_t)255;
  const size_t ws = cau ? cau_dt_ws_bytes(c->dtype, B, P) : 0;
  char* buf = nullptr;
  SDDM_HIP_CHECK(hipMalloc(&buf, 2 * bytes + ws));
  hipError_t e = launch_dt_pack(c->dtype, in, buf, (int)B, C, P, s);
  if (cau) {
    const SeqNet& n = static_cast<const SeqNet&>(*c->net);
    const int layers = tstnn ? static_cast<const TSTNNState&>(n).layers : static_cast<const CAUState&>(n).n_tstb;
    CauDtArgs a{buf, buf + bytes, c->warena.base + n.woff.at(blk + ".wmat"), c->warena.at<float>(n.woff.at(blk + ".wvec")), buf + 2 * bytes,
                (int)B, (int)dim2, (int)dim1, layers, tstnn ? 1 : 0};
    if (e == hipSuccess) e = launch_cau_dual_transformer(c->dtype, a, s);
  } else {
    const UNetState& n = static_cast<const UNetState&>(*c->net);
    DualTransformerArgs a{};
    a.x = buf; a.out = buf + bytes; a.stats = nullptr;
    a.wmat = c->warena.base + n.woff.at("mid.wmat"); a.wvec = c->warena.at<float>(n.woff.at("mid.wvec"));
    a.dim2 = (int)dim2; a.dim1 = (int)dim1; a.n_tstb = n.u.n_tstb;
    if (e == hipSuccess) e = launch_dual_transformer(c->dtype, a, (int)B, s);
  }
  if (e == hipSuccess) e = launch_dt_unpack(c->dtype, buf + bytes, out, (int)B, C, P, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(buf);
  if (e != hipSuccess) FAIL(SDDM_ERR_HIP, "dual_transformer: %s", hipGetErrorString(e));
  return SDDM_OK;
}

// One SelfAttention of a UNetModified context alone (UNetModified.py:150-169).  Only the layer's own
// parameters need to be loaded: parameters outside it that are still missing are packed as zeros
int sddm_self_attention(sddm_ctx* c, const char* layer, const float* in, int64_t B, int64_t H, int64_t W, float* out,
                        void* stream) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (c->net_type != "UNetModified") FAIL(SDDM_ERR_STATE, "sddm_self_attention needs a context configured for UNetModified");
  if (!layer || !in || !out) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  const std::string blk = layer;
  const auto it = c->params.find(blk + ".qkv.weight");
  if (it == c->params.end()) FAIL(SDDM_ERR_INVALID_ARG, "the network has no attention layer '%s'", layer);
  const int C = (int)it->second.shape[1];
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > (1 << 20) || W > (1 << 20) || B * H * W > ((int64_t)1 << 24))
    FAIL(SDDM_ERR_SHAPE, "B=%lld H=%lld W=%lld: the attention kernels index B * H * W up to 2^24", (long long)B, (long long)H, (long long)W);
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  for (auto& kv : c->params) {
    if (kv.second.loaded) continue;
    if (kv.first.rfind(blk + ".", 0) == 0) FAIL(SDDM_ERR_STATE, "parameter %s not loaded", kv.first.c_str());
    int64_t n = 1;
    for (int64_t d : kv.second.shape) n *= d;
    if ((int64_t)kv.second.data.size() != n) kv.second.data.assign((size_t)n, 0.f);
  }
  if (c->params_dirty) TRY(c->net->upload_weights(c));
  if (c->tables_dirty) TRY(upload_tables(c));
  const UNetState& n = static_cast<const UNetState&>(*c->net);
  hipStream_t s = (hipStream_t)stream;
  const int P = (int)(H * W), QT = attn_query_tile(P);
  if (attn_core_lds_bytes(c->dtype, C) > (size_t)kLdsBytes) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "%s: %d channels", layer, C);
  auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t act = al((size_t)B * P * C * dtype_size(c->dtype)), st = al(sizeof(float) * (size_t)B * (P / QT) * C * 2);
  char* buf = nullptr;
  SDDM_HIP_CHECK(hipMalloc(&buf, 5 * act + st));       // x, out, qkv (3), the input's statistics
  AttnArgs a{};
  a.x = buf; a.out = buf + act; a.qkv = buf + 2 * act; a.gst = (const float*)(buf + 5 * act); a.gtiles = P / QT; a.gntile = QT;
  a.gamma = c->warena.at<float>(n.woff.at(blk + ".norm.gamma")); a.beta = c->warena.at<float>(n.woff.at(blk + ".norm.beta"));
  a.groups = n.u.groups; a.eps = 1e-5f;
  a.wqkv_f = c->warena.base + n.woff.at(blk + ".qkv_f"); a.wout_f = c->warena.base + n.woff.at(blk + ".out_f");
  a.bout = c->warena.at<float>(n.woff.at(blk + ".out.b"));
  a.stats = nullptr; a.P = P; a.C = C; a.QT = QT;
  a.scale_log2 = (float)(1.4426950408889634 / std::sqrt((double)C));
  hipError_t e = launch_dt_pack(c->dtype, in, buf, (int)B, C, P, s);
  if (e == hipSuccess) e = launch_attn_input_stats(c->dtype, buf, (float*)(buf + 5 * act), (int)B, P, C, QT, s);
  if (e == hipSuccess) e = launch_attn_qkv(c->dtype, a, (int)B, s);
  if (e == hipSuccess) e = launch_attn_core(c->dtype, a, (int)B, s);
  if (e == hipSuccess) e = launch_dt_unpack(c->dtype, buf + act, out, (int)B, C, P, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(buf);
  if (e != hipSuccess) FAIL(SDDM_ERR_HIP, "self_attention: %s", hipGetErrorString(e));
  return SDDM_OK;
}

int sddm_transition(sddm_ctx* c, int mode, const float* x_t, const float* eps, const float* cond, int t, int64_t B,
                    int64_t N, uint64_t seed, int64_t row_offset, float* out, void* stream) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (mode < 0 || mode > 4) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "transition mode %d", mode);
  if (t < 1 || t > c->T) FAIL(SDDM_ERR_INVALID_ARG, "t=%d outside [1, %d]", t, c->T);
  if (!x_t || !eps || !out || (mode >= 2 && mode <= 3 && !cond)) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  TRY(ensure_tables(c));
  TransArgs a{};
  a.mode = mode; a.x_t = x_t; a.eps = eps; a.cond = cond; a.out = out; a.total = B * N; a.N = N; a.t = t;
  a.co = c->coef(); a.seed = seed; a.row_offset = row_offset;
  SDDM_HIP_CHECK(launch_transition(a, (hipStream_t)stream));
  return SDDM_OK;
}

int sddm_q_sample(sddm_ctx* c, int mode, const float* x0, const float* y, const float* noise, const int64_t* t,
                  const float* r, int64_t B, int64_t N, float* x_t, float* combined, float* s_out, float* level_out,
                  void* stream) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (mode < 0 || mode > 1) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "q_sample mode %d", mode);
  if (!x0 || !noise || !t || !x_t || (mode == 1 && !y)) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  if (B < 0 || N < 1) FAIL(SDDM_ERR_INVALID_ARG, "shape B=%lld N=%lld", (long long)B, (long long)N);
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  TRY(ensure_tables(c));
  QArgs a{};
  a.mode = mode; a.x0 = x0; a.y = y; a.noise = noise; a.t = t; a.r = r;
  a.sab = c->dtab(3); a.alpha_bar = c->dtab(2); a.m = c->dtab(8); a.sqrt_delta = c->dtab(9);
  a.x_t = x_t; a.combined = combined; a.s_out = s_out; a.level_out = level_out; a.B = B; a.N = N;
  SDDM_HIP_CHECK(launch_q_sample(a, (hipStream_t)stream));
  return SDDM_OK;
}

int sddm_set_conv_tuning(sddm_ctx* c, const char* json) {
  if (!c || !json) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  // the plan takes the first table whose lane batch, dtype and length match it (match_tuning)
  std::vector<TuneTable> out;
  TRY(parse_conv_tuning(json, out));
  c->tunes = std::move(out);
  if (c->net) c->net->replan();                     // re-plan on the next call
  return SDDM_OK;
}

int sddm_unet_plan(const char* config_json, const char* tuning_json, int compute_dtype, char* buf, int64_t buflen) {
  if (!config_json || !buf || buflen < 3) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  if (compute_dtype < 0 || compute_dtype > 2) FAIL(SDDM_ERR_INVALID_ARG, "bad dtype %d", compute_dtype);
  Json cfg;
  try {
    cfg = Json::parse(config_json);
  } catch (const std::exception& e) {
    FAIL(SDDM_ERR_INVALID_ARG, "config JSON: %s", e.what());
  }
  const Json& net = cfg.at("network");
  const std::string type = net.string("type", "");
  if (type != "UNetModified2" && type != "UNetTST" && type != "UNetModified")
    FAIL(SDDM_ERR_NOT_IMPLEMENTED, "network type '%s' has no plan", type.c_str());
  UNetCfg u;
  int Ns = -1;
  TRY(unet_configure(cfg, net.at("args"), type == "UNetTST", u, &Ns, type == "UNetModified"));
  int lane_rows = (int)cfg.number("lane_rows", 16);            // as sddm_create / sddm_configure: SDDM_LANE_ROWS overrides
  if (const char* lr = std::getenv("SDDM_LANE_ROWS")) lane_rows = std::max(1, std::atoi(lr));
  if (lane_rows < 1) FAIL(SDDM_ERR_INVALID_ARG, "lane_rows %d", lane_rows);
  std::vector<TuneTable> tunes;
  if (tuning_json) TRY(parse_conv_tuning(tuning_json, tunes));
  UNetPlan plan;
  TRY(plan_unet(u, Ns, compute_dtype, lane_rows, match_tuning(tunes, lane_rows, Ns, compute_dtype), PlanKnobs::env(), plan));
  const std::string js = plan_json(plan);
  if ((int64_t)js.size() + 1 > buflen) FAIL(SDDM_ERR_INVALID_ARG, "buffer too small (%zu)", js.size() + 1);
  std::memcpy(buf, js.c_str(), js.size() + 1);
  return SDDM_OK;
}

int sddm_log_spectrogram(const float* audio, int64_t B, int64_t N, int n_fft, int hop, const float* window,
                         const float* fb, int n_out, float* out, void* stream) {
  if (!audio || !window || !out) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  if (n_fft < 2 || n_fft > 1024 || (n_fft & (n_fft - 1))) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "n_fft %d (powers of two <= 1024)", n_fft);
  if (hop < 1 || B < 1 || N <= n_fft / 2) FAIL(SDDM_ERR_SHAPE, "B=%lld N=%lld hop=%d n_fft=%d", (long long)B, (long long)N, hop, n_fft);
  if (!fb && n_out != n_fft / 2 + 1) FAIL(SDDM_ERR_INVALID_ARG, "linear spectrogram has %d bins, not %d", n_fft / 2 + 1, n_out);
  StftArgs a{};
  a.audio = audio; a.B = B; a.N = N; a.n_fft = n_fft; a.hop = hop; a.frames = (int)(1 + N / hop); a.n_out = n_out;
  a.window = window; a.fb = fb; a.out = out;
  SDDM_HIP_CHECK(launch_stft_features(a, (hipStream_t)stream));
  return SDDM_OK;
}

int sddm_initial_state(sddm_ctx* c, int mode, const float* cond, int64_t B, int64_t N, uint64_t seed,
                       int64_t row_offset, float* out, void* stream) {
  if (!c || !c->configured) FAIL(SDDM_ERR_STATE, "context not configured");
  if (mode < 0 || mode > 4) FAIL(SDDM_ERR_NOT_IMPLEMENTED, "init mode %d", mode);
  if (!out || (mode >= 2 && !cond)) FAIL(SDDM_ERR_INVALID_ARG, "NULL tensor");
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  TRY(ensure_tables(c));
  InitArgs ia{};
  ia.mode = mode; ia.cond = cond; ia.out = out; ia.total = B * N; ia.N = N; ia.T = c->T;
  ia.co = c->coef(); ia.seed = seed; ia.row_offset = row_offset;
  SDDM_HIP_CHECK(launch_init_state(ia, (hipStream_t)stream));
  return SDDM_OK;
}

int sddm_profile_enable(sddm_ctx* c, int enable) {
  if (!c) FAIL(SDDM_ERR_INVALID_ARG, "NULL ctx");
  SDDM_HIP_CHECK(hipSetDevice(c->device));
  c->prof = enable != 0;
  c->ev_pend.clear();
  c->op_acc.clear();
  if (c->prof && c->ev_pool.empty()) {
    c->ev_pool.resize(512);
    for (auto& e : c->ev_pool) SDDM_HIP_CHECK(hipEventCreate(&e));
  }
  return SDDM_OK;
}

static const std::vector<Op>& profiled_ops(sddm_ctx* c) {   // of a diffusion-only context: none
  static const std::vector<Op> kNoOps;
  return c->net ? c->net->ops() : kNoOps;
}

int sddm_profile_read(sddm_ctx* c, const char* kernel_class, double* avg_ms, int64_t* launches,
                      double* bytes_per_launch, double* flops_per_launch) {
  if (!c || !kernel_class) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  const std::string k = kernel_class;
  const int cls = k == "conv_in" ? 0 : k == "gn_finalize" ? 1 : k == "conv3x3" ? 2 : k == "final" ? 3 : -1;
  if (cls < 0) FAIL(SDDM_ERR_INVALID_ARG, "kernel class %s", kernel_class);
  const std::vector<Op>& ops = profiled_ops(c);
  double ms = 0, bytes = 0, flops = 0;
  int64_t n = 0;
  for (size_t i = 0; i < c->op_acc.size() && i < ops.size(); ++i) {
    if (ops[i].cls != cls) continue;
    ms += c->op_acc[i].ms; bytes += c->op_acc[i].bytes; flops += c->op_acc[i].flops; n += c->op_acc[i].n;
  }
  if (avg_ms) *avg_ms = n ? ms / n : 0.0;
  if (launches) *launches = n;
  if (bytes_per_launch) *bytes_per_launch = n ? bytes / n : 0.0;
  if (flops_per_launch) *flops_per_launch = n ? flops / n : 0.0;
  return SDDM_OK;
}

// profiling builds only (not part of the C ABI): copy the phase stamps of the op named by the
// SDDM_STAMPS environment variable, [blocks][8] u64
int sddm_debug_stamps(sddm_ctx* c, void* host, int64_t max_blocks, int64_t* n_blocks) {
  if (!c || !host || !n_blocks) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  *n_blocks = 0;
  if (!c->stamp_buf) return SDDM_OK;
  const int64_t n = std::min<int64_t>(c->stamp_blocks, max_blocks);
  SDDM_HIP_CHECK(hipDeviceSynchronize());
  SDDM_HIP_CHECK(hipMemcpy(host, c->stamp_buf, sizeof(unsigned long long) * 8 * n, hipMemcpyDeviceToHost));
  *n_blocks = n;
  return SDDM_OK;
}

int sddm_profile_ops(sddm_ctx* c, char* buf, int64_t buflen) {
  if (!c || !buf || buflen < 3) FAIL(SDDM_ERR_INVALID_ARG, "NULL argument");
  const std::vector<Op>& ops = profiled_ops(c);
  std::string js = "[";
  char tmp[768];
  for (size_t i = 0; i < ops.size(); ++i) {
    const ProfAcc a = i < c->op_acc.size() ? c->op_acc[i] : ProfAcc{};
    snprintf(tmp, sizeof(tmp),
             "%s{\"name\": \"%s\", \"kernel\": \"%s\", \"inst\": \"%s\", \"cls\": %d, \"launches\": %lld, "
             "\"avg_ms\": %.6f, \"bytes\": %.0f, \"flops\": %.0f}",
             i ? ", " : "", ops[i].name.c_str(), ops[i].kname.c_str(), ops[i].kinst.c_str(), ops[i].cls, (long long)a.n,
             a.n ? a.ms / a.n : 0.0, ops[i].bytes, ops[i].flops);
    js += tmp;
  }
  js += "]";
  if ((int64_t)js.size() + 1 > buflen) FAIL(SDDM_ERR_INVALID_ARG, "buffer too small (%zu)", js.size() + 1);
  std::memcpy(buf, js.c_str(), js.size() + 1);
  return SDDM_OK;
}

}  // extern "C"
