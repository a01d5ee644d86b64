"""GPU: DenoiseWaveGrad1 / DenoiseWaveGrad3 (reference model/wavegrad.py:184-242, 307-353) under
SDDM.infer (model.py:50-124) through the facade and libsddm_hip, against goldens generated from the
reference and the numpy oracle pinned by test_denoise_wavegrad.py."""
import numpy as np
import pytest
import torch

import _net_suite as S
import _denoise_wavegrad_oracle as O
from _helpers import golden, rms

pytestmark = pytest.mark.gpu

NETS = ("DenoiseWaveGrad1", "DenoiseWaveGrad3")
HOP = {"DenoiseWaveGrad1": 400, "DenoiseWaveGrad3": 300}
SCHED = S.SCHED
CASES = {n: S.NetCase(n, O, "denoise_wavegrad.npz", 3 * HOP[n], short_len=2 * HOP[n], key=n + "/", by_name=True,
                      bad_lengths=(500, HOP[n] // 2), spec_hop=HOP[n], spec_input=(1, 1, HOP[n]), sharding_nonzero=False,
                      cli_config="config_denoise_wavegrad1.json", cli_chunk=1200, cli_lengths=(3000, 700),
                      cli_num_samples=("%", 400)) for n in NETS}
_gate = S.gate


def _params(name):
    return S.params(CASES[name])


def _net(name, dtype="float32"):
    return S.net(CASES[name], dtype=dtype)


def _model(name, mode="original"):
    return S.model(CASES[name], mode=mode)


def _inputs(name, B, N, seed):
    return S.inputs(B, N, seed)


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


@pytest.mark.parametrize("nc,mode", S.SAMPLING_CASES)
@pytest.mark.parametrize("name", NETS)
def test_sampling_matches_reference(torch_cuda, name, nc, mode):
    S.check_sampling_matches_reference(CASES[name], nc, mode)


@pytest.mark.parametrize("name", NETS)
def test_continuous_sampling_single_clip(torch_cuda, name):
    S.check_continuous_sampling_single_clip(CASES[name])


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
    S.check_row_sharding(CASES[name])


@pytest.mark.parametrize("name", NETS)
def test_rows_are_independent_of_the_batch(torch_cuda, name):
    S.check_rows_in_two_parts(CASES[name])


@pytest.mark.parametrize("name", NETS)
def test_rejects_bad_geometry(torch_cuda, name):
    S.check_rejects_bad_geometry(CASES[name])


@pytest.mark.parametrize("name", NETS)
def test_spectrogram_arch_is_not_implemented(torch_cuda, name):
    S.check_spectrogram_arch_is_not_implemented(CASES[name])


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
    S.check_sddm_forward_matches_oracle(CASES[name])


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    """infer.py with configs/config_denoise_wavegrad1.json (chunks of 1200 samples, T = 3): WAV in,
    chunk, denoise, stitch, WAV out, with no offline feature step."""
    S.check_infer_cli_end_to_end(CASES["DenoiseWaveGrad1"], tmp_path)
