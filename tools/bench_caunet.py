"""Time model.infer of CAUNet (config_caunet.json's network and schedule).

    python tools/bench_caunet.py [--batch 16] [--samples 16448] [--steps 50] [--reps 3]
                                 [--dtypes bfloat16,float16,float32] [--no-kernels] [--log profiles/NAME.log]

Cases: B x N samples in bfloat16, float16 and float32, `steps` reverse steps of the config's schedule
(linear, 1e-6 .. 0.01).  Each case is one warm-up call (context, weight upload, workspace), then `reps`
timed calls between device synchronisations; the best call is reported as ms per reverse step and
audio seconds generated per second (16 kHz).  launches_per_step restates the runtime's sequence
(csrc/cau_runtime.h): first_conv 1, noise MLPs 1, 8 layers x 4 convs, the Dual_Transformer
2 + 10 n_TSTB, final_conv 1, transition 1.  Unless --no-kernels, one further call of 5 steps runs under
torch.profiler and kernel_share gives every kernel family's part of the summed kernel time of that
call (template arguments stripped), gru_us_per_recurrent_step the GRU kernels' time divided by the
recurrent steps they ran (per reverse step 2 n_TSTB launches of dim1 or dim2 steps; the two directions
run in one launch).  The weights are the modules' initial values: the launch sequence does not depend
on them.
"""
import argparse
import json
import os
import re
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "speech-denoising-diffusion-model-2_amd"))

SAMPLE_RATE = 16000
PROFILE_STEPS = 5


def _model(torch, dtype, N, steps):
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    with open(os.path.join(REPO, "speech-denoising-diffusion-model-2_amd", "configs", "config_caunet.json")) as f:
        cfg = json.load(f)
    torch.manual_seed(0)
    net = NW.CAUNet(num_samples=N, **cfg["network"]["args"])
    net.compute_dtype = dtype
    da = cfg["diffusion"]["args"]
    d = D.GaussianDiffusion(da["schedule"], steps, da["linear_start"], da["linear_end"], device="cuda")
    return M.SDDM(d, net, compute_dtype=dtype).cuda(), cfg["network"]["args"]["n_TSTB"]


def _family(name):
    """Kernel name without namespaces and the dtype argument, e.g. cau_conv_kernel<0>; the profiler gives
    some names mangled (_ZN4sddm12_GLOBAL__N_115cau_conv_kernelIDF16bLi0EEEv...)."""
    if name.startswith("_ZN"):
        pos, ident = 3, ""
        while pos < len(name) and name[pos].isdigit():   # the nested name's length-prefixed parts
            m = re.match(r"\d+", name[pos:])
            n = int(m.group())
            ident = name[pos + m.end():pos + m.end() + n]
            pos += m.end() + n
        mode = re.match(r"I\w*?Li(\d+)E", name[pos:])
        return ident + ("<%s>" % mode.group(1) if mode else "")
    name = re.sub(r"^void\s+", "", name).replace("(anonymous namespace)::", "").replace("sddm::", "")
    m = re.match(r"(\w+)(?:<[^,>]*,\s*(\d+)>)?", re.sub(r"\(.*$", "", name))
    return (m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")) if m else name


def kernel_shares(torch, dtype, B, N, n_tstb):
    """Kernel families' shares of one PROFILE_STEPS-step call, and the GRU's time per recurrent step."""
    from torch.profiler import ProfilerActivity, profile
    model, _ = _model(torch, dtype, N, PROFILE_STEPS)
    cond = (0.3 * torch.randn(B, 1, N, device="cuda")).clamp(-1, 1)
    model.infer(cond, seed=1)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model.infer(cond, seed=2)
        torch.cuda.synchronize()
    fam = {}
    for e in prof.events():
        us = float(getattr(e, "device_time_total", 0.0) or getattr(e, "cuda_time_total", 0.0) or 0.0)
        if us <= 0:
            continue
        key = _family(e.name)
        fam[key] = fam.get(key, 0.0) + us
    total = sum(fam.values())
    if not total:
        raise RuntimeError("torch.profiler recorded no kernels")
    frames = (N - 128) // 64 + 1
    recurrent = PROFILE_STEPS * n_tstb * (8 + frames)
    gru = sum(v for k, v in fam.items() if "gru" in k)
    return ({k: round(v / total, 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])},
            gru / recurrent, total / PROFILE_STEPS / 1e3)


def run_case(torch, dtype, B, N, steps, reps, kernels):
    model, n_tstb = _model(torch, dtype, N, steps)
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
    res = {"network": "CAUNet", "dtype": dtype, "B": B, "N": N, "steps": steps,
           "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best,
           "launches_per_step": 1 + 1 + 8 * 4 + 2 + 10 * n_tstb + 1 + 1}
    if kernels:
        res["kernel_share"], res["gru_us_per_recurrent_step"], res["kernel_ms_per_step"] = kernel_shares(torch, dtype, B, N, n_tstb)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--samples", type=int, default=16448)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default="bfloat16,float16,float32")
    ap.add_argument("--no-kernels", action="store_true", help="skip the profiled call")
    ap.add_argument("--log", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    lines = []
    for dtype in args.dtypes.split(","):
        r = run_case(torch, dtype, args.batch, args.samples, args.steps, args.reps, not args.no_kernels)
        line = json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r.items()})
        print(line, flush=True)
        lines.append(line)
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
