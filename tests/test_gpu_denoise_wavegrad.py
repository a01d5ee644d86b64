"""GPU: DenoiseWaveGrad1 / DenoiseWaveGrad3 (reference model/wavegrad.py:184-242, 307-353) under
SDDM.infer (model.py:50-124) through the facade and libsddm_hip, against goldens generated from the
reference and the numpy oracle pinned by test_denoise_wavegrad.py."""
import functools
import json
import os
import struct

import numpy as np
import pytest
import torch

import _denoise_wavegrad_oracle as O
from _helpers import golden, rms
from _weights import make_params

pytestmark = pytest.mark.gpu

NETS = ("DenoiseWaveGrad1", "DenoiseWaveGrad3")
HOP = {"DenoiseWaveGrad1": 400, "DenoiseWaveGrad3": 300}
SCHED = ("linear", 3, 1e-4, 0.05)
MODES = ("original", "condition_in", "sr3", "supportive", "conditional")
_NETS = {}


@functools.lru_cache(maxsize=None)
def _params(name):
    return make_params(O.param_shapes(name), 0)


def _net(name, dtype="float32"):
    """One facade network per (name, dtype), shared by the tests (its weights never change)."""
    if (name, dtype) not in _NETS:
        import model.network as NW
        n = getattr(NW, name)()
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _params(name).items()})
        n.compute_dtype = dtype
        _NETS[name, dtype] = n.cuda()
    return _NETS[name, dtype]


def _model(name, mode="original", noise_condition="sqrt_alpha_bar", dtype="float32", sched=SCHED):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*sched, device="cuda")
    return M.SDDM(d, _net(name, dtype), noise_condition=noise_condition, p_transition=mode,
                  compute_dtype=dtype).cuda()


def _inputs(name, B, N, seed):
    rng = np.random.default_rng(seed)
    cond = np.clip(0.3 * rng.standard_normal((B, 1, N)), -1, 1).astype(np.float32)
    x_t = rng.standard_normal((B, 1, N)).astype(np.float32)
    nl = rng.uniform(0.05, 0.99, B).astype(np.float32)
    return cond, x_t, nl


def _gate(ref):
    return max(1.0, rms(ref, 0))


@pytest.mark.parametrize("dtype,tol", [("float32", 1e-4), ("bfloat16", 3e-2), ("float16", 5e-3)])
@pytest.mark.parametrize("name", NETS)
def test_forward_matches_reference(torch_cuda, name, dtype, tol):
    z = golden("denoise_wavegrad.npz")
    cond, x_t, nl = (torch.from_numpy(z[f"{name}/fw/{k}"]).cuda() for k in ("cond", "x_t", "noise_level"))
    ref = z[f"{name}/fw/eps"]
    eps = _net(name, dtype)(cond, x_t, nl).cpu().numpy()
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"{name} {dtype}: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    assert err <= tol * _gate(ref)


@pytest.mark.parametrize("case", ["bottom1", "tiles", "single"])
@pytest.mark.parametrize("name", NETS)
def test_forward_matches_oracle(torch_cuda, name, case):
    """bottom1: B=3 at one hop -- the bottom lengths are 1 and 5 (the encoder bottom is one position).
    tiles: B=2 at 16 hops (6400 / 4800 samples) -- partial 128-position tiles at every level and more
    than one tile at the top three.  single: one clip, which the reference cannot run; the output
    keeps its [1, 1, N] shape."""
    hop = HOP[name]
    B, N = {"bottom1": (3, hop), "tiles": (2, 16 * hop), "single": (1, 2 * hop)}[case]
    cond, x_t, nl = _inputs(name, B, N, seed=31)
    ref = O.forward(name, _params(name), cond, x_t, nl)
    # the noise level in the shape SDDM.infer hands over ([B, 1, 1]) and as [B]
    level = torch.from_numpy(nl).cuda()
    eps = _net(name)(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(),
                     level.reshape(B, 1, 1) if case != "tiles" else level)
    assert tuple(eps.shape) == (B, 1, N)
    err = rms(eps.cpu().numpy(), ref)
    print(f"{name} {case} B={B} N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f})")
    assert err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")])
@pytest.mark.parametrize("name", NETS)
def test_sampling_matches_reference(torch_cuda, name, nc, mode):
    """The reference's unmodified SDDM.infer: the output and every intermediate x_t."""
    z = golden("denoise_wavegrad.npz")
    k = f"{name}/inf/{nc}/{mode}"
    cond = torch.from_numpy(z[f"{name}/inf/cond"]).cuda()
    m = _model(name, mode, nc)
    out = m.infer(cond, seed=7).cpu().numpy()
    assert out.shape == z[k + "/out"].shape
    err = rms(out, z[k + "/out"])
    T = SCHED[1]
    record = torch.empty((T,) + tuple(cond.shape), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(cond)
    m._context(cond.device).sample_continuous(cond, out2, record, 1, 7, 0)
    errs = [rms(record[i].cpu().numpy(), z[k + "/steps"][i]) for i in range(T)]
    print(f"{name} {nc} {mode}: rms of the output {err:.3e}, of x_t per step {['%.2e' % e for e in errs]}")
    assert err <= 1e-3
    assert max(errs) <= 1e-3
    assert torch.equal(out2.cpu(), torch.from_numpy(out))


@pytest.mark.parametrize("name", NETS)
def test_continuous_sampling_single_clip(torch_cuda, name):
    z = golden("denoise_wavegrad.npz")
    cond = torch.from_numpy(z[f"{name}/inf/cond"][:1]).cuda()
    rec = _model(name, "sr3").infer(cond, continuous=True, seed=7)
    assert len(rec) == 1 + SCHED[1]
    assert torch.equal(rec[0], cond)
    got = np.stack([r.cpu().numpy() for r in rec[1:]])
    assert got.shape[1:] == (1, 1, 3 * HOP[name])
    assert rms(got, z[f"{name}/inf/sqrt_alpha_bar/sr3/steps"][:, :1]) <= 1e-3


def test_hoisted_encoder_equals_per_step_network(torch_cuda):
    """DenoiseWaveGrad1 runs downsample_x and upsample.0's head once per sampling call.  A loop over
    net(cond, x_t, level), which re-runs them every step, and diffusion.p_transition must give the
    same x_0 from the same draws (caller noise = the Philox stream the transitions draw from)."""
    from oracle import philox
    name, seed, B = "DenoiseWaveGrad1", 13, 2
    N = 2 * HOP[name]
    T = SCHED[1]
    cond, _, _ = _inputs(name, B, N, seed=17)
    cond = torch.from_numpy(cond).cuda()
    noise = np.stack([philox.normal(seed, d, (B, 1, N)) for d in range(T + 1)])
    m = _model(name, "original")
    got = m.infer(cond, noise=torch.from_numpy(noise).cuda())
    net, d = m.noise_estimate_model, m.diffusion
    x = torch.from_numpy(noise[0]).cuda()                                # x_T = draw 0 (model.py:68)
    for t in range(T, 0, -1):
        level = d.get_noise_level(t) * torch.ones(B, 1, 1, device="cuda")
        x = d.p_transition(x, t, net(cond, x, level), seed=seed)
    err = rms(got.cpu().numpy(), x.cpu().numpy())
    print(f"hoisted vs per-step: rms {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("name", NETS)
def test_row_sharding_is_bit_identical(torch_cuda, name):
    """Rows sampled in two shards (row_offset) equal the rows of one batch."""
    m = _model(name, "conditional", dtype="bfloat16")
    cond, _, _ = _inputs(name, 4, 2 * HOP[name], seed=1)
    cond = torch.from_numpy(cond).cuda()
    full = m.infer(cond, seed=11)
    a = m.infer(cond[:2].contiguous(), seed=11, row_offset=0)
    b = m.infer(cond[2:].contiguous(), seed=11, row_offset=2)
    assert torch.isfinite(full).all()
    assert torch.equal(full, torch.cat([a, b]))


@pytest.mark.parametrize("name", NETS)
def test_rows_are_independent_of_the_batch(torch_cuda, name):
    net = _net(name, "bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(name, 5, 2 * HOP[name], seed=2))
    full = net(cond, x_t, nl)
    parts = [net(cond[s].contiguous(), x_t[s].contiguous(), nl[s].contiguous()) for s in (slice(0, 2), slice(2, 5))]
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat(parts))


@pytest.mark.parametrize("name", NETS)
def test_rejects_bad_geometry(torch_cuda, name):
    net, m = _net(name), _model(name)
    for N in (500, HOP[name] // 2):
        z = torch.zeros(1, 1, N, device="cuda")
        with pytest.raises(AssertionError):
            net(z, z, torch.ones(1, device="cuda"))
        with pytest.raises(AssertionError):
            m.infer(z, seed=1)


@pytest.mark.parametrize("name", NETS)
def test_spectrogram_arch_is_not_implemented(torch_cuda, name):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, _net(name), hop_samples=HOP[name]).cuda()
    with pytest.raises(NotImplementedError):
        m.infer(torch.zeros(1, 1, HOP[name], device="cuda"), seed=1)


def test_denoise_wavegrad2_stays_not_implemented(torch_cuda):
    """Its 4 / 8 / 16-channel levels do not fit the MFMA convolution (Cin % 32)."""
    import sddm_hip
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": "DenoiseWaveGrad2", "args": {}}}
    with pytest.raises(NotImplementedError):
        sddm_hip.Context(cfg, 0)


@pytest.mark.parametrize("name", NETS)
def test_sddm_forward_matches_oracle(torch_cuda, name):
    """SDDM.forward (evaluation only): q-sample at fixed t, then the network."""
    B, N = 2, 2 * HOP[name]
    rng = np.random.default_rng(23)
    target = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, N)).astype(np.float32)).cuda()
    cond = (target + torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 1, N)).astype(np.float32)).cuda())
    noise = torch.from_numpy(rng.standard_normal((B, 1, N)).astype(np.float32)).cuda()
    t = torch.tensor([3, 1])
    r = torch.tensor([0.25, 0.75])
    m = _model(name)
    with torch.no_grad():
        predicted, got_noise = m(target, cond, noise=noise, t=t, random_step=r)
    assert torch.equal(got_noise, noise) and tuple(predicted.shape) == (B, 1, N)
    x_t, level, _ = m.diffusion.q_stochastic(target, noise, t=t, random_step=r)   # (x_t, noise level, step)
    ref = O.forward(name, _params(name), cond.cpu().numpy(), x_t.cpu().numpy(), level.cpu().numpy())
    err = rms(predicted.cpu().numpy(), ref)
    print(f"{name} SDDM.forward: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


def _write_pcm16(path, x, sr=16000):
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, 1, 1, sr, 2 * sr, 2, 16,
                      b"data", len(pcm))
    with open(path, "wb") as f:
        f.write(hdr + pcm)


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    """infer.py with configs/config_denoise_wavegrad1.json (chunks of 1200 samples, T = 3): WAV in,
    chunk, denoise, stitch, WAV out, with no offline feature step."""
    import infer
    import model.diffusion as D
    import model.model as M
    from data_loader import wav_io
    from parse_config import ConfigParser, read_json
    N = 1200
    rng = np.random.default_rng(4)
    for d in ("clean", "noisy"):
        os.makedirs(tmp_path / "data" / d)
    lengths = [3000, 700]
    for i, n in enumerate(lengths):
        c = 0.3 * np.sin(np.arange(n) * 0.05)
        _write_pcm16(tmp_path / "data" / "clean" / f"u{i}.wav", c)
        _write_pcm16(tmp_path / "data" / "noisy" / f"u{i}.wav", c + rng.uniform(-0.05, 0.05, n))
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_denoise_wavegrad1.json"))
    assert cfg["network"]["type"] == "DenoiseWaveGrad1" and cfg["num_samples"] % 400 == 0
    cfg["num_samples"] = N
    cfg["diffusion"]["args"].update({"n_timestep": 3, "linear_end": 0.05})
    cfg["infer_dataset"]["args"]["data_root"] = str(tmp_path / "data")
    cfg["infer_data_loader"]["args"].update({"batch_size": 1, "num_workers": 0})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    ref_model = M.SDDM(D.GaussianDiffusion("linear", 3, 1e-4, 0.05, device="cpu"), _net("DenoiseWaveGrad1"))
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
