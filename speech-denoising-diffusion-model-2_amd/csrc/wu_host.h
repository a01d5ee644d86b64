// Host code the Waveunet3 and the FiLM Wave-U-Net paths of the runtime share (included by wu_runtime.h and
// wu2_runtime.h, i.e. by sddm_runtime.cpp after sddm_ctx and SeqNet).
#pragma once
#include "wu_kernels.h"

// conv weight -> [co][k][ci] in the compute dtype; transposed: the source is ConvTranspose1d's [ci][co][k]
static void wu_add_conv(sddm_ctx* c, WeightPacker& pk, const std::string& name, int co, int ci, int k,
                        const std::vector<float>& w, bool transposed) {
  char* b = pk.raw(name, (size_t)co * k * ci * dtype_size(c->dtype));
  for (int o = 0; o < co; ++o)
    for (int i = 0; i < ci; ++i)
      for (int t = 0; t < k; ++t) {
        const size_t src = transposed ? ((size_t)i * co + o) * k + t : ((size_t)o * ci + i) * k + t;
        store_elem(b, ((size_t)o * k + t) * ci + i, w[src], c->dtype);
      }
}

// the (B, N) a network that halves the length `halvings` (at most eleven) times takes; `net` names
// it in the message
static int wu_check_shape(const char* net, int64_t B, int64_t N, int halvings = 3) {
  if (B < 1 || B > 65535) FAIL(SDDM_ERR_INVALID_ARG, "batch %lld", (long long)B);
  static const char* const kTimes[] = {"zero", "one", "two", "three", "four", "five", "six", "seven", "eight", "nine", "ten", "eleven"};
  const int hop = 1 << halvings;
  if (N < hop || N % hop)
    FAIL(SDDM_ERR_SHAPE, "%lld samples is not a positive multiple of %d (%s halves the length %s times)", (long long)N, hop, net,
         kTimes[halvings]);
  if (N > (int64_t)1 << 30) FAIL(SDDM_ERR_SHAPE, "%lld samples: %s positions are 32-bit", (long long)N, net);
  return SDDM_OK;
}

// the noise level of the current call: the caller's [B] (a forward), else sqrt_alpha_bar[t] or t of
// the step counter in the StepParams at off_sp (sampling, model.py:84-89)
static WULevel wu_begin_level(sddm_ctx* c, const float* noise_level, size_t off_sp) {
  if (noise_level) return WULevel{noise_level, nullptr, 0, nullptr};
  return WULevel{nullptr, c->dtab(3), c->noise_time_step, &c->warena.at<StepParams>(off_sp)->t};
}
