"""Time model.infer of Waveunet (config_waveunet.json's network and schedule).

    python tools/bench_waveunet.py [--batch 16] [--samples 16384] [--steps 50] [--reps 3]
                                   [--dtypes bfloat16,float16,float32] [--log profiles/NAME.log]

Cases: B x N samples in bfloat16, float16 and float32, `steps` reverse steps of the config's schedule
(linear, 1e-6 .. 0.01).  Each case is one warm-up call (context, weight upload, workspace, code
objects), then `reps` timed calls between device synchronisations; the best call is reported as ms
per reverse step and audio seconds generated per second (16 kHz).  launches_per_step restates the
library's launch sequence (csrc/wu1_runtime.h) in Python -- it is not counted by the library;
tools/wu_fold_trace.py checks the same sequence against a kernel trace, launch by launch: stem, 66 MFMA ConvLayer convs, 22 FiLM convs, head,
transition, and a GroupNorm finalize behind the stem and every ConvLayer that is not folded.
`path` is "default", "per_row" when SDDM_WU_NO_FOLD is set in the environment, or "fold_all" when
SDDM_WU_FOLD_ALL is (ConvLayers with rows shorter than 128 positions run the batch-folded kernel,
which finishes the norm itself); the library reads the knobs when the context is configured, so a
path is one process.  The default is the per-row path at every length.  The weights are the
module's initial values: the launch sequence does not depend on them.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-denoising-diffusion-model-2_amd"))

SAMPLE_RATE = 16000


def _set(name):
    v = os.environ.get(name, "")
    return bool(v) and v[0] != "0"


def path():
    return "per_row" if _set("SDDM_WU_NO_FOLD") else ("fold_all" if _set("SDDM_WU_FOLD_ALL") else "default")


def launches_per_step(N, levels=12):
    """wu1_runtime.h: level i is N / 2^i long; under fold_all a ConvLayer is folded when its output is
    < 128 long (wu1::fold_default folds none)."""
    L = [N >> i for i in range(levels)]
    outs = [L[0]]                                                       # stem
    for i in range(levels - 1):
        outs += [L[i]] * (1 if i == 0 else 2) + [L[i + 1]]               # pre (i > 0), post, downconv
    outs.append(L[-1])                                                  # bottleneck
    for i in range(levels - 1, 0, -1):
        outs += [L[i - 1]] * 3                                          # upconv, pre, post
    assert len(outs) == 67
    folded = sum(1 for k, n in enumerate(outs) if k > 0 and n < 128) if path() == "fold_all" else 0
    return 1 + 66 + 22 + (67 - folded) + 1 + 1


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
    return {"network": "Waveunet", "path": path(), "dtype": dtype, "B": B, "N": N, "steps": steps,
            "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best,
            "launches_per_step": launches_per_step(N)}


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
