"""The output bits of the sequential networks (DiffWave, the WaveGrad family, Waveunet3, Waveunet2,
Waveunet), pinned across changes of the host code that drives them and across kernel refactors that claim bit
equality.

None of their kernels uses an atomic and every path's own tests assert run-to-run bit equality, so
host-side work on the runtime (the sampling loop, the forward wrapper, the weight packer, the
workspace cache) and a kernel refactor that keeps every float expression and every summation order
have an exact criterion: every output bit stays.  tests/golden/seq_path_digests.json holds SHA-256
digests of the outputs below.  Every case asserts digest equality.

The digests are recorded on the GPU with the library of the commit before the change they guard,
never with the code under test (tools/record_store_digests.py --module test_gpu_seq_digests).  The
first 60 were recorded before the paths were given one loop and one packer.  The Waveunet2,
float16, tiles and bottom entries were recorded before the two Wave-U-Nets were given one conv
kernel and one stem kernel; that recording reproduced the first 60.  The Waveunet entries (the
12-level network) were recorded before Waveunet2 and Waveunet were given one runtime and the
batch-folded kernel of Waveunet's short levels was removed; that recording reproduced the first 112.

Cases are <net>/<dtype>/<kind>, B = 2, N = two hops (296 for the Waveunets: the smallest sizes of
the path tests at which every level has more than one position), T = 4, one library context per
(net, dtype).  The spectrogram nets run under their only mode, the waveform-conditioned ones under
p_transition "conditional" (the condition enters the initial state and the transition).  DiffWave
and the -time_step entries take the step as the noise condition, the rest sqrt_alpha_bar.
  fw       network_forward at distinct noise levels
  sample   sample, seed 7, row_offset 3
  record   sample_continuous, sample_inter 2: out, then the two recorded states
  noise    sample_noise with seeded draws [T + 1][B][1][N]
  reshape  fw, a forward at B = 3 and another length on the same context, fw again: both equal the
           pinned fw digest (the workspace cache)
The four Waveunet entries also run fw and sample in float16 (their <f16_t> kernels), and two
forward-only kinds in all three dtypes, the shapes of their test_forward_matches_oracle:
  tiles    network_forward at B = 2, N = 2072 (2072 / 1036 / 518 / 259): every level has several
           128-position tiles and a partial last one, WU_UP4 blocks use both 64-position halves
  bottom   network_forward at B = 3, N = 8: the bottleneck is one position, the transposed conv
           starts from one position, every tile is partial
The 12-level Waveunet takes multiples of 2048 only: its N is 2048 (the lengths are 2048 ... 1: every
level below 128 positions, the one-position bottleneck and a transposed conv that starts from one
position are in every run), its reshape length 4096.  It runs the five kinds in float32 and
bfloat16, fw and sample under time_step and in float16, and one forward-only kind of its own in all
three dtypes:
  odd      network_forward at B = 3, N = 6144 (96 ... 3): no powers of two, partly filled tiles, an
           odd batch
The CAUNet entries were recorded before the UNet runtime moved into unet_runtime.h and CAUNet's
Dual_Transformer packer was shared with UNetTST's; that recording reproduced the first 131.  CAUNet
(_caunet_oracle.ARGS) frames 128 samples every 64: its N is 704 (10 frames, more than the widest dense
dilation), its reshape length 320.  It runs the five kinds in float32 and bfloat16, fw and sample in
float16, and one kind of its own in float32 and bfloat16:
  dt       dual_transformer on [2, 64, 17, 8], on a context of its own where only mid.* is loaded
           (every other parameter packs as zeros)
"""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import _caunet_oracle as CO
import _denoise_wavegrad_oracle as DO
import _waveunet3_oracle as WO
from _waveunet_film_oracle import WAVEUNET as W1O, WAVEUNET2 as W2O
from _helpers import GOLDEN, diffwave_params, wavegrad_params
from _weights import make_params

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "seq_path_digests.json")
B, T = 2, 4
# net -> (network type, N, another N for the reshape case, spectrogram bins or 0, hop, noise_condition)
NETS = {"DiffWave": ("DiffWave", 512, 768, 513, 256, "time_step"),
        "WaveGrad": ("WaveGrad", 600, 900, 128, 300, "sqrt_alpha_bar"),
        "DenoiseWaveGrad1": ("DenoiseWaveGrad1", 800, 1200, 0, 400, "sqrt_alpha_bar"),
        "DenoiseWaveGrad3": ("DenoiseWaveGrad3", 600, 900, 0, 300, "sqrt_alpha_bar"),
        "Waveunet3": ("Waveunet3", 296, 304, 0, 1, "sqrt_alpha_bar"),
        "Waveunet3-time_step": ("Waveunet3", 296, 304, 0, 1, "time_step")}
KINDS = ("fw", "sample", "record", "noise", "reshape")
CASES = [f"{n}/{d}/{k}" for n in NETS for d in ("float32", "bfloat16") for k in KINDS]
NETS.update({"Waveunet2": ("Waveunet2", 296, 304, 0, 1, "sqrt_alpha_bar"),
             "Waveunet2-time_step": ("Waveunet2", 296, 304, 0, 1, "time_step")})
WAVEUNETS = ("Waveunet3", "Waveunet3-time_step", "Waveunet2", "Waveunet2-time_step")
NET_ARGS = {"Waveunet3": WO.ARGS, "Waveunet2": W2O.ARGS}
SHAPES = {"tiles": (2, 2072, 12), "bottom": (3, 8, 13)}   # kind -> rows, N, seed of the inputs
# appended behind the first 60, whose names and order stay
CASES += [f"{n}/{d}/{k}" for n in WAVEUNETS[2:] for d in ("float32", "bfloat16") for k in KINDS]
CASES += [f"{n}/float16/{k}" for n in WAVEUNETS for k in ("fw", "sample")]
CASES += [f"{n}/{d}/{k}" for n in WAVEUNETS for d in ("float32", "bfloat16", "float16") for k in SHAPES]
# the 12-level Waveunet, appended behind the first 112: its lengths are multiples of 2048
NETS.update({"Waveunet": ("Waveunet", 2048, 4096, 0, 1, "sqrt_alpha_bar"),
             "Waveunet-time_step": ("Waveunet", 2048, 4096, 0, 1, "time_step")})
NET_ARGS["Waveunet"] = W1O.ARGS
SHAPES12 = {"odd": (3, 6144, 14)}                         # kind -> rows, N, seed of the inputs
ALL_SHAPES = {**SHAPES, **SHAPES12}
CASES += [f"Waveunet/{d}/{k}" for d in ("float32", "bfloat16") for k in KINDS]
CASES += [f"Waveunet-time_step/{d}/{k}" for d in ("float32", "bfloat16") for k in ("fw", "sample")]
CASES += [f"Waveunet/float16/{k}" for k in ("fw", "sample")]
CASES += [f"Waveunet/{d}/{k}" for d in ("float32", "bfloat16", "float16") for k in SHAPES12]
# CAUNet, appended behind the first 131
NETS["CAUNet"] = ("CAUNet", 704, 320, 0, 1, "sqrt_alpha_bar")
NET_ARGS["CAUNet"] = CO.ARGS
CASES += [f"CAUNet/{d}/{k}" for d in ("float32", "bfloat16") for k in KINDS]
CASES += [f"CAUNet/float16/{k}" for k in ("fw", "sample")]
CASES += [f"CAUNet/{d}/dt" for d in ("float32", "bfloat16")]

_CTX = {}


@functools.lru_cache(maxsize=None)
def _params(net_type):
    if net_type == "DiffWave":
        return diffwave_params()
    if net_type == "WaveGrad":
        return wavegrad_params()
    if net_type == "Waveunet3":
        return make_params(WO.param_shapes(), 0)
    if net_type == "Waveunet2":
        return make_params(W2O.param_shapes(), 0)
    if net_type == "Waveunet":
        return make_params(W1O.param_shapes(), 0)
    if net_type == "CAUNet":
        return make_params(CO.param_shapes(), 0)
    return make_params(DO.param_shapes(net_type), 0)


def _ctx(net, dtype, only=None):
    """The context of (net, dtype); `only`: a context of its own with just that prefix's parameters."""
    if only is not None or (net, dtype) not in _CTX:
        import sddm_hip
        net_type, _, _, bins, hop, nc = NETS[net]
        if bins:
            arch = {"type": "SDDM_spectrogram", "args": {"noise_condition": nc, "hop_samples": hop}}
        else:
            arch = {"type": "SDDM", "args": {"noise_condition": nc, "p_transition": "conditional",
                                             "q_transition": "original"}}
        cfg = {"arch": arch,
               "diffusion": {"type": "GaussianDiffusion",
                             "args": {"schedule": "linear", "n_timestep": T, "linear_start": 1e-4, "linear_end": 0.05}},
               "network": {"type": net_type, "args": dict(NET_ARGS.get(net_type, {}))},
               "num_samples": -1}
        ctx = sddm_hip.Context(cfg, 0, dtype)
        if only is not None:
            ctx.load_state_dict({k: v for k, v in _params(net_type).items() if k.startswith(only)})
            assert ctx.missing() > 0
            return ctx
        ctx.load_state_dict(_params(net_type))
        assert ctx.missing() == 0
        _CTX[net, dtype] = ctx
    return _CTX[net, dtype]


def _inputs(net, rows, N, seed):
    """cond (spectrogram [rows][bins][F] or waveform [rows][1][N]), x_t [rows][1][N], distinct levels [rows]."""
    _, _, _, bins, hop, _ = NETS[net]
    rng = np.random.default_rng(seed)
    if bins:
        cond = rng.uniform(0, 1, (rows, bins, N // hop)).astype(np.float32)
    else:
        cond = np.clip(0.3 * rng.standard_normal((rows, 1, N)), -1, 1).astype(np.float32)
    x_t = rng.standard_normal((rows, 1, N)).astype(np.float32)
    nl = np.linspace(0.95, 0.15, rows).astype(np.float32)
    return cond, x_t, nl


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def _forward(torch, ctx, net, rows, N, seed):
    dev = torch.device("cuda", 0)
    cond, x_t, nl = (torch.from_numpy(a).to(dev) for a in _inputs(net, rows, N, seed))
    eps = torch.full((rows, 1, N), float("nan"), device=dev)
    ctx.network_forward(cond, x_t, nl, eps)
    torch.cuda.synchronize()
    return eps.cpu().numpy()


def run_case(torch, case):
    """The output array of one case (fp32 on the host)."""
    net, dtype, kind = case.split("/")
    N, N2 = NETS[net][1:3]
    dev = torch.device("cuda", 0)
    if kind == "dt":
        x = np.random.default_rng(17).standard_normal((2, 64, 17, 8)).astype(np.float32)
        y = torch.full(x.shape, float("nan"), device=dev)
        _ctx(net, dtype, only="mid.").dual_transformer(torch.from_numpy(x).to(dev), y)
        torch.cuda.synchronize()
        return y.cpu().numpy()
    ctx = _ctx(net, dtype)
    if kind == "fw":
        return _forward(torch, ctx, net, B, N, 5)
    if kind in ALL_SHAPES:
        return _forward(torch, ctx, net, *ALL_SHAPES[kind])
    if kind == "reshape":
        first = _forward(torch, ctx, net, B, N, 5)
        other = _forward(torch, ctx, net, 3, N2, 6)
        assert np.isfinite(other).all() and np.abs(other).max() > 0
        again = _forward(torch, ctx, net, B, N, 5)
        assert digest(first) == digest(again), "the forward changed after a forward at another shape"
        return again
    cond = torch.from_numpy(_inputs(net, B, N, 9)[0]).to(dev)
    out = torch.full((B, 1, N), float("nan"), device=dev)
    if kind == "sample":
        ctx.sample(cond, out, 7, 3)
    elif kind == "record":
        record = torch.full((T // 2, B, 1, N), float("nan"), device=dev)
        ctx.sample_continuous(cond, out, record, 2, 7, 3)
        out = torch.cat([out[None], record])
    else:
        draws = np.random.default_rng(11).standard_normal((T + 1, B, 1, N)).astype(np.float32)
        ctx.sample_noise(cond, out, torch.from_numpy(draws).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_output_digest_is_pinned(torch_cuda, case):
    pinned = json.load(open(FIXTURE))["digests"]
    out = run_case(torch_cuda, case)
    assert np.isfinite(out).all() and np.abs(out).max() > 0
    got = digest(out)
    print(f"{case}: {got[:16]} (pinned {pinned[case][:16]})")
    assert got == pinned[case]
    if case.endswith("/reshape"):
        assert got == pinned[case.rsplit("/", 1)[0] + "/fw"]
