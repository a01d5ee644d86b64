"""Time model.infer of UNetTST (config_unettst.json's network and schedule).

    python tools/bench_unettst.py [--batch 16] [--samples 16448] [--steps 50] [--reps 3]
                                  [--dtypes bfloat16,float16,float32] [--no-unet] [--log profiles/NAME.log]

Cases: B x N samples in bfloat16, float16 and float32, `steps` reverse steps of the config's schedule
(linear, 1e-6 .. 0.01).  Each case is one warm-up call (context, weight upload, plan, graph capture),
then `reps` timed calls between device synchronisations; the best call is reported as ms per reverse
step and audio seconds generated per second (16 kHz).  A further profiled call (per-launch events, no
graphs) gives launches_per_step (the ops of one lane's step) and transformer_share, the
Dual_Transformer op's part of the summed op times.  Unless --no-unet, every dtype is followed by the
same case for UNetModified2 at the same arguments without n_TSTB: UNetTST is that network with
mid.0's two convs swapped for the block, so the difference is the block's cost.  The weights are the
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


def run_case(torch, network, dtype, B, N, steps, reps):
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    with open(os.path.join(REPO, "speech-denoising-diffusion-model-2_amd", "configs", "config_unettst.json")) as f:
        cfg = json.load(f)
    torch.manual_seed(0)
    args = dict(cfg["network"]["args"])
    if network == "UNetModified2":
        args.pop("n_TSTB")
    net = getattr(NW, network)(num_samples=N, **args)
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
    ctx = model._context(cond.device)
    ctx.profile(True)
    model.infer(cond, seed=1)
    torch.cuda.synchronize()
    ops = ctx.profile_ops()
    ctx.profile(False)
    total = sum(o["avg_ms"] * o["launches"] for o in ops)
    tst = [o for o in ops if "dual_transformer" in o["name"]]
    res = {"network": network, "dtype": dtype, "B": B, "N": N, "steps": steps,
           "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best,
           "launches_per_step": len(ops)}
    if tst:
        res["transformer_launches_per_step"] = len(tst)
        res["transformer_ms"] = sum(o["avg_ms"] for o in tst)
        res["transformer_share"] = sum(o["avg_ms"] * o["launches"] for o in tst) / total if total else 0.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=16448)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="bfloat16,float16,float32")
    ap.add_argument("--no-unet", action="store_true", help="skip the UNetModified2 cases")
    ap.add_argument("--log", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for dtype in args.dtypes.split(","):
        for network in ("UNetTST",) + (() if args.no_unet else ("UNetModified2",)):
            r = run_case(torch, network, dtype, args.batch, args.samples, args.steps, args.reps)
            line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
            print(line, flush=True)
            lines.append(line)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
