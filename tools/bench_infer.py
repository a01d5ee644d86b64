"""Time model.infer of one of the sequential denoisers at its config's network and schedule.

    python tools/bench_infer.py --network NAME [--batch B] [--samples N] [--steps 50] [--reps 3]
                                [--dtypes bfloat16,float16,float32] [--log profiles/NAME.log]
                                [--no-kernels] [--no-unet]

NAME is a key of NETWORKS: Waveunet, Waveunet2, Waveunet3, UNetTST, UNetModified, CAUNet, TSTNN or DenoiseWaveGrad; the
table gives the config file and the default batch and samples.  Cases: B x N samples in every dtype,
`steps` reverse steps of the config's schedule (linear, 1e-6 .. 0.01).  Each case is one warm-up call
(context, weight upload, workspace, code objects, plan and graph capture where the runtime has them),
then `reps` timed calls between device synchronisations; the best call is reported as ms per reverse
step and audio seconds generated per second (16 kHz), one JSON line per case.  The weights are the
modules' initial values: the launch sequence does not depend on them.

launches_per_step restates the library's launch sequence, at any N:
  Waveunet   csrc/wu2_runtime.h at twelve levels: stem, 66 MFMA ConvLayer convs, 67 GroupNorm
             finalizes, 22 FiLM convs, head, transition
  Waveunet2  csrc/wu2_runtime.h at four levels: stem, 18 convs, 19 finalizes, 6 FiLM convs, head, transition
  Waveunet3  csrc/wu_runtime.h: input statistics, stem, 27 MFMA Block convs with one GroupNorm finalize
             each, 6 ConvLayers of three launches, head, transition
  CAUNet     csrc/cau_runtime.h: first_conv 1, noise MLPs 1, 8 layers x 4 convs, the Dual_Transformer
             2 + 10 n_TSTB, final_conv 1, transition 1
  TSTNN      csrc/tstnn_runtime.h: first 1, dense convs 4 + 4, down 1, up 1, the Dual_Transformer
             2 + 10 * 4, gate 1, final 1, transition 1
  UNetTST    counted: a further profiled call (per-launch events, no graphs) gives the ops of one lane's
             step, and transformer_share, the Dual_Transformer op's part of the summed op times
  UNetModified  counted the same way; attention_share is the part of the SelfAttention launches (attn_qkv and
             attn_core per attention layer) in the summed op times

CAUNet and TSTNN: unless --no-kernels, one further call of 5 steps runs under torch.profiler and
kernel_share gives every kernel family's part of the summed kernel time of that call (template
arguments stripped), gru_us_per_recurrent_step the GRU kernels' time divided by the recurrent steps they
ran (per reverse step two launches per layer, of dim1 and of dim2 steps; the two directions run in one
launch.  CAUNet: n_TSTB layers over [frames][8]; TSTNN: 4 layers over [frames][256]).

UNetTST: unless --no-unet, every dtype is followed by the same case for UNetModified2 at the same
arguments without n_TSTB: UNetTST is that network with mid.0's two convs swapped for the block, so the
difference is the block's cost.

DenoiseWaveGrad: DenoiseWaveGrad1 at B x 32000 samples, DenoiseWaveGrad3 at B x 32100 and the WaveGrad
net at B x 32100 (107 frames of 300) as the yardstick on the same device, in bfloat16 and float32, with
the reference config.json's schedule (linear, 1e-4 .. 2e-2); every line also gives the ratio to
WaveGrad's ms per step at the same dtype, and none gives launches_per_step.  --samples does not apply.
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

# config: the file under configs/ (None: no arguments, the reference config.json's schedule);
# transformer: (layers, dim2, dim1) of the Dual_Transformer from the network's arguments and N, for the
# networks whose profiled call reports kernel shares;
# num_samples: the constructor takes the length; launches: launches_per_step, a number, a function of
# the network's arguments, "ops" (counted from the profiled ops) or None (not reported);
# cases: the (network, N) pairs of one dtype where they are not (NAME, --samples)
NETWORKS = {
    "Waveunet": {"config": "config_waveunet.json", "batch": 16, "samples": 16384, "num_samples": False,
                 "launches": 1 + 66 + 67 + 22 + 1 + 1},
    "Waveunet2": {"config": "config_waveunet2.json", "batch": 16, "samples": 16384, "num_samples": False,
                  "launches": 1 + 18 + 19 + 6 + 1 + 1},
    "Waveunet3": {"config": "config_waveunet3.json", "batch": 16, "samples": 16384, "num_samples": False,
                  "launches": 1 + 1 + 27 + 27 + 6 * 3 + 1 + 1},
    "UNetTST": {"config": "config_unettst.json", "batch": 16, "samples": 16448, "num_samples": True, "launches": "ops"},
    "UNetModified": {"config": "config_unetmodified.json", "batch": 16, "samples": 16448, "num_samples": True,
                     "launches": "ops"},
    "CAUNet": {"config": "config_caunet.json", "batch": 16, "samples": 16448, "num_samples": True,
               "launches": lambda a: 1 + 1 + 8 * 4 + 2 + 10 * a["n_TSTB"] + 1 + 1,
               "transformer": lambda a, N: (a["n_TSTB"], (N - 128) // 64 + 1, 8)},
    "TSTNN": {"config": "config_tstnn.json", "batch": 16, "samples": 16384, "num_samples": True,
              "launches": 1 + (4 + 4) + 1 + 1 + (2 + 10 * 4) + 1 + 1 + 1,
              "transformer": lambda a, N: (4, (N - 512) // 256 + 1, 256)},
    "DenoiseWaveGrad": {"config": None, "batch": 8, "samples": None, "num_samples": False, "launches": None,
                        "dtypes": "bfloat16,float32",
                        "cases": (("WaveGrad", 32100), ("DenoiseWaveGrad1", 32000), ("DenoiseWaveGrad3", 32100))},
}


def _model(torch, spec, network, dtype, N, steps):
    """SDDM around `network` built from the spec's config, and the network's arguments."""
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    args, start, end = {}, 1e-4, 2e-2
    if spec["config"]:
        with open(os.path.join(REPO, "speech-denoising-diffusion-model-2_amd", "configs", spec["config"])) as f:
            cfg = json.load(f)
        args = dict(cfg["network"]["args"])
        if network == "UNetModified2":
            args.pop("n_TSTB")
        start, end = cfg["diffusion"]["args"]["linear_start"], cfg["diffusion"]["args"]["linear_end"]
    torch.manual_seed(0)
    net = getattr(NW, network)(**(dict(args, num_samples=N) if spec["num_samples"] else args))
    net.compute_dtype = dtype
    d = D.GaussianDiffusion("linear", steps, start, end, device="cuda")
    if network == "WaveGrad":
        return M.SDDM_spectrogram(d, net, hop_samples=net.hop_samples, compute_dtype=dtype).cuda(), args
    return M.SDDM(d, net, compute_dtype=dtype).cuda(), args


def _condition(torch, model, B, N):
    net = model.noise_estimate_model
    if type(net).__name__ == "WaveGrad":
        return torch.rand(B, net.freq_bins, N // net.hop_samples, device="cuda")
    return (0.3 * torch.randn(B, 1, N, device="cuda")).clamp(-1, 1)


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
    m = re.match(r"(\w+)(?:<[^,>]*,\s*(\d+)\s*[,>])?", re.sub(r"\(.*$", "", name))
    return (m.group(1) + ("<%s>" % m.group(2) if m.group(2) else "")) if m else name


def kernel_shares(torch, spec, network, dtype, B, N, net_args):
    """Kernel families' shares of one PROFILE_STEPS-step call, and the GRU's time per recurrent step."""
    from torch.profiler import ProfilerActivity, profile
    model, _ = _model(torch, spec, network, dtype, N, PROFILE_STEPS)
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
    layers, dim2, dim1 = spec["transformer"](net_args, N)
    recurrent = PROFILE_STEPS * layers * (dim1 + dim2)
    gru = sum(v for k, v in fam.items() if "gru" in k)
    return ({k: round(v / total, 4) for k, v in sorted(fam.items(), key=lambda kv: -kv[1])},
            gru / recurrent, total / PROFILE_STEPS / 1e3)


def profiled_ops(torch, model, cond, res):
    """UNetTST, its UNetModified2 companion and UNetModified: the ops of one lane's step and the share of the
    Dual_Transformer or of the SelfAttention launches in them."""
    ctx = model._context(cond.device)
    ctx.profile(True)
    model.infer(cond, seed=1)
    torch.cuda.synchronize()
    ops = ctx.profile_ops()
    ctx.profile(False)
    total = sum(o["avg_ms"] * o["launches"] for o in ops)
    tst = [o for o in ops if "dual_transformer" in o["name"]]
    res["launches_per_step"] = len(ops)
    if tst:
        res["transformer_launches_per_step"] = len(tst)
        res["transformer_ms"] = sum(o["avg_ms"] for o in tst)
        res["transformer_share"] = sum(o["avg_ms"] * o["launches"] for o in tst) / total if total else 0.0
    attn = [o for o in ops if ".attn[" in o["name"]]
    if attn:
        res["attention_launches_per_step"] = len(attn)
        res["attention_ms"] = sum(o["avg_ms"] for o in attn)
        res["attention_share"] = sum(o["avg_ms"] * o["launches"] for o in attn) / total if total else 0.0


def run_case(torch, spec, network, dtype, B, N, steps, reps, kernels):
    model, net_args = _model(torch, spec, network, dtype, N, steps)
    cond = _condition(torch, model, B, N)
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
    res = {"network": network, "dtype": dtype, "B": B, "N": N, "steps": steps,
           "ms_per_step": 1e3 * best / steps, "audio_s_per_s": B * N / SAMPLE_RATE / best}
    launches = spec["launches"]
    if launches == "ops":
        profiled_ops(torch, model, cond, res)
    elif launches is not None:
        res["launches_per_step"] = launches(net_args) if callable(launches) else launches
    if "transformer" in spec and kernels:
        res["kernel_share"], res["gru_us_per_recurrent_step"], res["kernel_ms_per_step"] = kernel_shares(
            torch, spec, network, dtype, B, N, net_args)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--network", required=True, choices=sorted(NETWORKS))
    ap.add_argument("--batch", type=int, default=None, help="default: the network's in NETWORKS")
    ap.add_argument("--samples", type=int, default=None, help="default: the network's in NETWORKS")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dtypes", default=None, help="default: bfloat16,float16,float32 (DenoiseWaveGrad: bfloat16,float32)")
    ap.add_argument("--no-kernels", action="store_true", help="CAUNet, TSTNN: skip the profiled call")
    ap.add_argument("--no-unet", action="store_true", help="UNetTST: skip the UNetModified2 cases")
    ap.add_argument("--log", default=None, help="also append the result lines to this file")
    args = ap.parse_args()
    spec = NETWORKS[args.network]
    if "cases" in spec and args.samples is not None:
        ap.error(f"--samples does not apply to {args.network}: its cases have their own lengths")
    B = args.batch or spec["batch"]
    cases = spec.get("cases") or ((args.network, args.samples or spec["samples"]),)
    if args.network == "UNetTST" and not args.no_unet:
        cases += (("UNetModified2", cases[0][1]),)
    import torch
    assert torch.cuda.is_available(), "needs a HIP device"
    lines, base = [], {}
    for dtype in (args.dtypes or spec.get("dtypes", "bfloat16,float16,float32")).split(","):
        for network, N in cases:
            r = run_case(torch, spec, network, dtype, B, N, args.steps, args.reps, not args.no_kernels)
            if "cases" in spec:                           # DenoiseWaveGrad: WaveGrad comes first in every dtype
                base.setdefault(dtype, r["ms_per_step"])
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
