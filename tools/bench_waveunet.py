"""Time model.infer of Waveunet (config_waveunet.json's network and schedule).

    python tools/bench_waveunet.py [--batch 16] [--samples 16384] [--steps 50] [--reps 3]
                                   [--dtypes bfloat16,float16,float32] [--log profiles/NAME.log]

Cases: B x N samples in bfloat16, float16 and float32, `steps` reverse steps of the config's schedule
(linear, 1e-6 .. 0.01).  Each case is one warm-up call (context, weight upload, workspace, code
objects), then `reps` timed calls between device synchronisations; the best call is reported as ms
per reverse step and audio seconds generated per second (16 kHz).  launches_per_step is the
library's launch sequence (csrc/wu2_runtime.h at twelve levels): stem, 66 MFMA ConvLayer convs, 67
GroupNorm finalizes, 22 FiLM convs, head, transition, at any N.  The weights are the module's initial
values: the launch sequence does not depend on them.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-denoising-diffusion-model-2_amd"))

SAMPLE_RATE = 16000


LAUNCHES_PER_STEP = 1 + 66 + 67 + 22 + 1 + 1


def run_case(torch, dtype, B, N, steps, reps):
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    with open(os.path.join(REPO, "speech-denoising-diffusion-model-2_amd", "configs", "config_waveunet.json")) as f:
        cfg = json.load(f)
    torch.manual_seed(0)
    net = NW.Waveunet(**cfg["network"]["args"])
    net.compute_dtype = dtype
    da = cfg["diffusion"]["args"]
    d = D.GaussianDiffusion(da["schedule"], steps, da["linear_start"], da["linear_end"], device="cuda")
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
    return {"network": "Waveunet", "dtype": dtype, "B": B, "N": N, "steps": steps,
            "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best,
            "launches_per_step": LAUNCHES_PER_STEP}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="bfloat16,float16,float32")
    ap.add_argument("--log", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for dtype in args.dtypes.split(","):
        r = run_case(torch, dtype, args.batch, args.samples, args.steps, args.reps)
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
        print(line, flush=True)
        lines.append(line)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
