"""GPU: Waveunet2 (reference model/waveunet2.py:226-324, config_waveunet2.json) under SDDM.infer
(model.py:50-124) through the facade and libsddm_hip, against goldens generated from the reference
and the torch oracle pinned by test_waveunet2.py.

Measured on MI355X (rms of the difference / rms of the reference):
  forward vs golden (B=2, N=296)      float32 1.0e-6   bfloat16 1.04e-2   float16 1.47e-3
  forward at B=2, N=16384 vs oracle   bfloat16 1.16e-2  float16 1.44e-3
  bottom1 / tiles / single, float32   2.6e-7 / 3.1e-7 / 3.4e-7 rms
  sampling vs golden, every x_t       <= 1.1e-7 rms
  SDDM.forward vs oracle              3.2e-7 rms
The 16-bit bars (3e-2, 5e-3) are the project's bars for a single forward of every network; a CPU
emulation with conv inputs, outputs and weights rounded to the 16-bit type (the oracle's `rounding`)
gives 1.1e-2 / 1.5e-3 at the golden shape and 1.2e-2 / 1.5e-3 at B=2, N=16384.
"""
import functools
import json
import os
import struct

import numpy as np
import pytest
import torch

from _waveunet_film_oracle import WAVEUNET2 as O
from _helpers import golden, rms
from _weights import make_params

pytestmark = pytest.mark.gpu

SCHED = ("linear", 3, 1e-4, 0.05)
MODES = ("original", "condition_in", "sr3", "supportive", "conditional")
_NETS = {}


@functools.lru_cache(maxsize=None)
def _params():
    return make_params(O.param_shapes(), 0)


def _net(dtype="float32"):
    """One facade network per dtype, shared by the tests (its weights never change)."""
    if dtype not in _NETS:
        import model.network as NW
        n = NW.Waveunet2(**O.ARGS)
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _params().items()})
        n.compute_dtype = dtype
        _NETS[dtype] = n.cuda()
    return _NETS[dtype]


def _model(mode="original", noise_condition="sqrt_alpha_bar", dtype="float32", sched=SCHED):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*sched, device="cuda")
    return M.SDDM(d, _net(dtype), noise_condition=noise_condition, p_transition=mode, compute_dtype=dtype).cuda()


def _inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    cond = np.clip(0.3 * rng.standard_normal((B, 1, N)), -1, 1).astype(np.float32)
    x_t = rng.standard_normal((B, 1, N)).astype(np.float32)
    nl = rng.uniform(0.05, 0.99, B).astype(np.float32)
    return cond, x_t, nl


def _gate(ref):
    return max(1.0, rms(ref, 0))


def _clamped(x):
    return float(np.mean(np.abs(x) >= 1.0))


@functools.lru_cache(maxsize=None)
def _big_case():
    """The config's own chunk length, B = 2: inputs and the oracle's output, computed once."""
    cond, x_t, nl = _inputs(2, 16384, seed=41)
    return cond, x_t, nl, O.forward(_params(), cond, x_t, nl)


@pytest.mark.parametrize("dtype,tol", [("float32", 1e-4), ("bfloat16", 3e-2), ("float16", 5e-3)])
def test_forward_matches_reference(torch_cuda, dtype, tol):
    z = golden("waveunet2.npz")
    cond, x_t, nl = (torch.from_numpy(z[f"fw/{k}"]).cuda() for k in ("cond", "x_t", "noise_level"))
    ref = z["fw/eps"]
    eps = _net(dtype)(cond, x_t, nl).cpu().numpy()
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"Waveunet2 {dtype}: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    if dtype == "float32":
        assert err <= tol * _gate(ref)
    else:
        emu = O.forward(_params(), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], rounding=getattr(torch, dtype))
        print(f"Waveunet2 {dtype}: CPU emulation (conv inputs, weights, outputs rounded) relative {rms(emu, ref) / rms(ref, 0):.3e}")
        assert err / rms(ref, 0) <= tol


@pytest.mark.parametrize("case", ["bottom1", "tiles", "single"])
def test_forward_matches_oracle(torch_cuda, case):
    """bottom1: B=3, N=8 -- every length is <= 8, the bottleneck is one position, the transposed conv
    starts from one position and a GroupNorm group is 8 values.  tiles: B=2, N=2072 (2072 / 1036 / 518 / 259) -- partial tiles
    everywhere and more than one 128-position tile at every level; level passed as [B].  single: one
    clip, level passed as [B, 1, 1]."""
    B, N = {"bottom1": (3, 8), "tiles": (2, 2072), "single": (1, 296)}[case]
    cond, x_t, nl = _inputs(B, N, seed=31)
    ref = O.forward(_params(), cond, x_t, nl)
    assert _clamped(ref) <= 0.25
    level = torch.from_numpy(nl).cuda()
    eps = _net()(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(),
                 level if case == "tiles" else level.reshape(B, 1, 1))
    assert tuple(eps.shape) == (B, 1, N)
    err = rms(eps.cpu().numpy(), ref)
    print(f"Waveunet2 {case} B={B} N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f}, clamped {_clamped(ref):.3f})")
    assert err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("dtype,tol", [("bfloat16", 3e-2), ("float16", 5e-3)])
def test_forward_16bit_at_the_config_length(torch_cuda, dtype, tol):
    cond, x_t, nl, ref = _big_case()
    assert _clamped(ref) <= 0.25
    eps = _net(dtype)(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), torch.from_numpy(nl).cuda())
    rel = rms(eps.cpu().numpy(), ref) / rms(ref, 0)
    emu = O.forward(_params(), cond, x_t, nl, rounding=getattr(torch, dtype))
    print(f"Waveunet2 {dtype} B=2 N=16384: relative rms vs oracle {rel:.3e} (CPU emulation {rms(emu, ref) / rms(ref, 0):.3e})")
    assert rel <= tol


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")])
def test_sampling_matches_reference(torch_cuda, nc, mode):
    """The reference's unmodified SDDM.infer: the output and every intermediate x_t; a second run is
    bit-equal."""
    z = golden("waveunet2.npz")
    k = f"inf/{nc}/{mode}"
    cond = torch.from_numpy(z["inf/cond"]).cuda()
    m = _model(mode, nc)
    out = m.infer(cond, seed=7).cpu().numpy()
    assert out.shape == z[k + "/out"].shape
    err = rms(out, z[k + "/out"])
    T = SCHED[1]
    record = torch.empty((T,) + tuple(cond.shape), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(cond)
    m._context(cond.device).sample_continuous(cond, out2, record, 1, 7, 0)
    errs = [rms(record[i].cpu().numpy(), z[k + "/steps"][i]) for i in range(T)]
    print(f"Waveunet2 {nc} {mode}: rms of the output {err:.3e}, of x_t per step {['%.2e' % e for e in errs]}")
    assert err <= 1e-3
    assert max(errs) <= 1e-3
    assert torch.equal(out2.cpu(), torch.from_numpy(out))


def test_continuous_sampling_single_clip(torch_cuda):
    z = golden("waveunet2.npz")
    cond = torch.from_numpy(z["inf/cond"][:1]).cuda()
    rec = _model("sr3").infer(cond, continuous=True, seed=7)
    assert len(rec) == 1 + SCHED[1]
    assert torch.equal(rec[0], cond)
    got = np.stack([r.cpu().numpy() for r in rec[1:]])
    assert got.shape[1:] == (1, 1, 296)
    assert rms(got, z["inf/sqrt_alpha_bar/sr3/steps"][:, :1]) <= 1e-3


def test_row_sharding_is_bit_identical(torch_cuda):
    """Rows sampled in two shards (row_offset) equal the rows of one batch."""
    m = _model("conditional", dtype="bfloat16")
    cond, _, _ = _inputs(4, 296, seed=1)
    cond = torch.from_numpy(cond).cuda()
    full = m.infer(cond, seed=11)
    a = m.infer(cond[:2].contiguous(), seed=11, row_offset=0)
    b = m.infer(cond[2:].contiguous(), seed=11, row_offset=2)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat([a, b]))


def test_rows_are_independent_of_the_batch(torch_cuda):
    net = _net("bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(5, 296, seed=2))
    full = net(cond, x_t, nl)
    parts = [net(cond[s].contiguous(), x_t[s].contiguous(), nl[s].contiguous()) for s in (slice(0, 2), slice(2, 5))]
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat(parts))


def test_rejects_bad_geometry(torch_cuda):
    net, m = _net(), _model()
    for N in (300, 4):
        z = torch.zeros(1, 1, N, device="cuda")
        with pytest.raises(AssertionError):
            net(z, z, torch.ones(1, device="cuda"))
        with pytest.raises(AssertionError):
            m.infer(z, seed=1)


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, _net(), hop_samples=8).cuda()
    with pytest.raises(NotImplementedError):
        m.infer(torch.zeros(1, 1, 8, device="cuda"), seed=1)


@pytest.mark.parametrize("change", [{"num_channels": [32, 64, 96, 128]}, {"depth": 2}, {"conv_type": "bn"},
                                    {"downconv_kernel_size": 3}, {"resample_stride": 4}, {"num_inputs": 1}])
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, change):
    import sddm_hip
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": "Waveunet2", "args": dict(O.ARGS, **change)}}
    with pytest.raises(NotImplementedError):
        sddm_hip.Context(cfg, 0)


def test_missing_params_counts_the_state_dict(torch_cuda):
    import sddm_hip
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": "Waveunet2", "args": dict(O.ARGS)}}
    ctx = sddm_hip.Context(cfg, 0)
    assert ctx.missing() == 90
    ctx.load_state_dict({"noise_estimate_model." + k: v for k, v in _params().items()})
    assert ctx.missing() == 0
    ctx.close()


def test_sddm_forward_matches_oracle(torch_cuda):
    """SDDM.forward (evaluation only): q-sample at fixed t, then the network."""
    B, N = 2, 296
    rng = np.random.default_rng(23)
    target = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, N)).astype(np.float32)).cuda()
    cond = (target + torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 1, N)).astype(np.float32)).cuda())
    noise = torch.from_numpy(rng.standard_normal((B, 1, N)).astype(np.float32)).cuda()
    t = torch.tensor([3, 1])
    r = torch.tensor([0.25, 0.75])
    m = _model()
    with torch.no_grad():
        predicted, got_noise = m(target, cond, noise=noise, t=t, random_step=r)
    assert torch.equal(got_noise, noise) and tuple(predicted.shape) == (B, 1, N)
    x_t, level, _ = m.diffusion.q_stochastic(target, noise, t=t, random_step=r)   # (x_t, noise level, step)
    ref = O.forward(_params(), cond.cpu().numpy(), x_t.cpu().numpy(), level.cpu().numpy())
    err = rms(predicted.cpu().numpy(), ref)
    print(f"Waveunet2 SDDM.forward: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


def _write_pcm16(path, x, sr=16000):
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, 1, 1, sr, 2 * sr, 2, 16,
                      b"data", len(pcm))
    with open(path, "wb") as f:
        f.write(hdr + pcm)


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    """infer.py with configs/config_waveunet2.json (chunks of 1024 samples, T = 3): WAV in, chunk,
    denoise, stitch, WAV out."""
    import infer
    import model.diffusion as D
    import model.model as M
    from data_loader import wav_io
    from parse_config import ConfigParser, read_json
    N = 1024
    rng = np.random.default_rng(4)
    for d in ("clean", "noisy"):
        os.makedirs(tmp_path / "data" / d)
    lengths = [2500, 700]
    for i, n in enumerate(lengths):
        c = 0.3 * np.sin(np.arange(n) * 0.05)
        _write_pcm16(tmp_path / "data" / "clean" / f"u{i}.wav", c)
        _write_pcm16(tmp_path / "data" / "noisy" / f"u{i}.wav", c + rng.uniform(-0.05, 0.05, n))
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_waveunet2.json"))
    assert cfg["network"]["type"] == "Waveunet2" and cfg["num_samples"] % 8 == 0
    cfg["num_samples"] = N
    cfg["diffusion"]["args"].update({"n_timestep": 3, "linear_end": 0.05})
    cfg["infer_dataset"]["args"]["data_root"] = str(tmp_path / "data")
    cfg["infer_data_loader"]["args"].update({"batch_size": 1, "num_workers": 0})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    ref_model = M.SDDM(D.GaussianDiffusion("linear", 3, 1e-4, 0.05, device="cpu"), _net())
    ck = tmp_path / "model_best.pth"
    torch.save({"arch": "SDDM", "epoch": 1,
                "state_dict": {"module." + k: v.cpu() for k, v in ref_model.state_dict().items()},
                "config": json.loads(json.dumps(cfg))}, ck)
    config = ConfigParser(cfg, resume=ck, run_id="e2e")
    log = infer.main(config, seed=100)
    assert np.isfinite(log["loss"])
    for i, n in enumerate(lengths):
        out, sr = wav_io.load(os.path.join(str(config.save_dir), "samples", "output", f"u{i}.wav"))
        assert sr == 16000 and out.shape == (1, -(-n // N) * N)
        assert out.shape[1] % N == 0 and torch.isfinite(out).all() and float(out.abs().max()) > 0
