"""Time model.infer of the waveform-conditioned WaveGrad variants against the WaveGrad yardstick.

    python tools/bench_denoise_wavegrad.py [--batch 8] [--steps 50] [--reps 3] [--log profiles/NAME.log]

Cases: DenoiseWaveGrad1 at B x 32000 samples (bf16 and fp32), DenoiseWaveGrad3 at B x 32100 and the
existing WaveGrad net at B x 32100 (107 frames of 300) on the same device, all with `steps` steps of
the reference config.json's schedule (linear, 1e-4 .. 2e-2).  Each case is one warm-up call (context,
weight upload, workspace), then `reps` timed calls between device synchronisations; the best call
is reported as ms per reverse step and audio seconds generated per second (16 kHz), and
DenoiseWaveGrad1 / 3 as a ratio to WaveGrad's ms per step at the same dtype.  The weights are the
modules' initial values: the launch sequence does not depend on them.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-denoising-diffusion-model-2_amd"))

SAMPLE_RATE = 16000


def run_case(torch, name, dtype, B, N, steps, reps):
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    torch.manual_seed(0)
    net = getattr(NW, name)()
    net.compute_dtype = dtype
    d = D.GaussianDiffusion("linear", steps, 1e-4, 2e-2, device="cuda")
    if name == "WaveGrad":
        model = M.SDDM_spectrogram(d, net, hop_samples=net.hop_samples, compute_dtype=dtype).cuda()
        cond = torch.rand(B, net.freq_bins, N // net.hop_samples, device="cuda")
    else:
        model = M.SDDM(d, net, compute_dtype=dtype).cuda()
        cond = (0.3 * torch.randn(B, 1, N, device="cuda")).clamp(-1, 1)
    out = model.infer(cond, seed=1)                       # warm-up
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, 1, N) and bool(torch.isfinite(out).all())
    best = float("inf")
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.infer(cond, seed=2 + r)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return {"network": name, "dtype": dtype, "B": B, "N": N, "steps": steps,
            "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--log", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    cases = [("WaveGrad", "bfloat16", 32100), ("DenoiseWaveGrad1", "bfloat16", 32000),
             ("DenoiseWaveGrad3", "bfloat16", 32100), ("WaveGrad", "float32", 32100),
             ("DenoiseWaveGrad1", "float32", 32000), ("DenoiseWaveGrad3", "float32", 32100)]
    lines, base = [], {}
    for name, dtype, N in cases:
        r = run_case(torch, name, dtype, args.batch, N, args.steps, args.reps)
        if name == "WaveGrad":
            base[dtype] = r["ms_per_step"]
        r["ms_per_step_vs_wavegrad"] = r["ms_per_step"] / base[dtype]
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
        print(line, flush=True)
        lines.append(line)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
