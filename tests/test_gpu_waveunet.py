"""GPU: Waveunet (reference model/waveunet.py:358-506, config_waveunet.json: twelve levels, 24 ... 288
channels) under SDDM.infer (model.py:50-124) through the facade and libsddm_hip, against goldens
generated from the reference and the torch oracle pinned by test_waveunet.py.

The golden shape is B = 2, N = 2048: the level lengths are 2048, 1024, ..., 1, so levels 5 to 11 are
shorter than the conv kernel's 128-position tile and the bottleneck is one position.

16-bit bars.  A CPU emulation with conv inputs, outputs and weights rounded to the 16-bit type (the
oracle's `rounding`) gives, relative rms against the reference,
  golden shape (B=2, N=2048)   bfloat16 1.35e-2   float16 1.87e-3
  B=2, N=16384                 bfloat16 1.55e-2   float16 2.20e-3
The bar is the project's (3e-2 / 5e-3) where the emulation is at most half of it, else twice the
emulation (_bar16): 3e-2 / 5e-3 at the golden shape, 3.11e-2 / 5e-3 at N = 16384.
Measured on MI355X (rms of the difference / rms of the reference unless noted):
  forward vs golden                   float32 1.3e-6   bfloat16 1.25e-2   float16 1.76e-3
  forward at B=2, N=16384 vs oracle   bfloat16 1.45e-2  float16 2.17e-3
  float32 vs oracle, four shapes      5.3e-7 ... 5.9e-7 rms
  sampling vs golden, every x_t       <= 1.8e-7 rms
  SDDM.forward vs oracle              5.4e-7 rms
Every layer at every length runs wu_conv_kernel per batch row.  Most tests share one network per
dtype in this process; the two *_by_path tests read the forwards of one child process
(_wu_paths_child.py), in which the library is loaded and a context configured by those forwards
alone.  The output bits of this network are pinned by test_gpu_seq_digests.py.
"""
import functools
import json
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from _waveunet_film_oracle import WAVEUNET as O
import _wu_paths_child as child
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
        n = NW.Waveunet(**O.ARGS)
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


def _bar16(dtype, emu):
    """The 16-bit bar: the project's where the CPU emulation's error is at most half of it, else twice
    the emulation's."""
    project = {"bfloat16": 3e-2, "float16": 5e-3}[dtype]
    return project if emu <= 0.5 * project else 2.0 * emu


def _clamped(x):
    return float(np.mean(np.abs(x) >= 1.0))


@functools.lru_cache(maxsize=None)
def _oracle_case(B, N):
    """Inputs and the oracle's output of one shape, computed once."""
    cond, x_t, nl = _inputs(B, N, seed=31)
    return cond, x_t, nl, O.forward(_params(), cond, x_t, nl)


@functools.lru_cache(maxsize=None)
def _big_case():
    """The config's own chunk length, B = 2: inputs and the oracle's output, computed once."""
    cond, x_t, nl = _inputs(2, 16384, seed=41)
    return cond, x_t, nl, O.forward(_params(), cond, x_t, nl)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_forward_matches_reference(torch_cuda, dtype):
    """float32 is the test that sees a wrong deep layer: replacing any one deep tensor moves the
    reference's output by at least 2.5e-2 relative rms."""
    z = golden("waveunet.npz")
    cond, x_t, nl = (torch.from_numpy(z[f"fw/{k}"]).cuda() for k in ("cond", "x_t", "noise_level"))
    ref = z["fw/eps"]
    eps = _net(dtype)(cond, x_t, nl).cpu().numpy()
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"Waveunet {dtype}: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    if dtype == "float32":
        assert err <= 1e-4 * _gate(ref)
    else:
        emu = O.forward(_params(), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], rounding=getattr(torch, dtype))
        emu = rms(emu, ref) / rms(ref, 0)
        print(f"Waveunet {dtype}: CPU emulation (conv inputs, weights, outputs rounded) relative {emu:.3e}, bar {_bar16(dtype, emu):.3e}")
        assert err / rms(ref, 0) <= _bar16(dtype, emu)


# ---- the forward in a fresh process.  Explicit ids here and below ("-per_row", "-default") keep the
# ids stable that these cases are recorded under
HERE = os.path.dirname(os.path.abspath(__file__))
_CHILD = {}
_CHILD_FAILED = []


def _child_run():
    """The arrays of the child (spawned once per module).  After a child that faulted, was killed or
    failed, no further child is started."""
    if _CHILD:
        return _CHILD
    if _CHILD_FAILED:
        pytest.fail(_CHILD_FAILED[0])
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "out.npz")
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_wu_paths_child.py"), out], timeout=120,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired:
            _CHILD_FAILED.append("the child process was killed at its 120 s limit")
            pytest.fail(_CHILD_FAILED[0])
        if r.returncode != 0:
            _CHILD_FAILED.append(f"the child process ended with status {r.returncode}:\n{r.stdout[-2000:]}")
            pytest.fail(_CHILD_FAILED[0])
        with np.load(out, allow_pickle=False) as z:
            _CHILD.update({k: z[k] for k in z.files})
    return _CHILD


@pytest.mark.parametrize("dtype", [pytest.param(d, id=d + "-per_row") for d in ("float32", "bfloat16", "float16")])
def test_forward_matches_reference_by_path(torch_cuda, dtype):
    """The golden forward in a process of its own, at the bars of test_forward_matches_reference:
    every layer through wu_conv_kernel, complete on its own."""
    z = golden("waveunet.npz")
    ref = z["fw/eps"]
    eps = _child_run()[f"fw/{dtype}"]
    rel = rms(eps, ref) / rms(ref, 0)
    print(f"Waveunet {dtype}, child process: relative rms vs reference {rel:.3e}")
    assert np.isfinite(eps).all()
    if dtype == "float32":
        assert rms(eps, ref) <= 1e-4 * _gate(ref)
    else:
        emu = O.forward(_params(), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], rounding=getattr(torch, dtype))
        assert rel <= _bar16(dtype, rms(emu, ref) / rms(ref, 0))


@pytest.mark.parametrize("shape", [pytest.param((3, 6144), id="per_row")])
def test_odd_shape_matches_oracle_by_path(torch_cuda, shape):
    """B = 3, N = 6144 (lengths 96 ... 3) in float32, in the child process."""
    cond, x_t, nl = child.odd_inputs()
    assert cond.shape == (shape[0], 1, shape[1])
    odd = O.forward(_params(), cond, x_t, nl)
    err = rms(_child_run()["odd/float32"], odd)
    print(f"Waveunet, child process, B=3 N=6144: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(odd)


@pytest.mark.parametrize("B,N", [pytest.param(B, N, id=f"{B}-{N}-default") for B, N in ((3, 6144), (5, 2048), (1, 2048), (2, 4096))])
def test_forward_matches_oracle(torch_cuda, B, N):
    """Shapes at which the short levels can go wrong.  B=3, N=6144: lengths 96, 48, 24, 12, 6, 3 -- no
    powers of two, rows straddle or under-fill a 128-column tile, odd batch.  B=5, N=2048: 320
    columns of rows at L = 64.  B=1: level passed as [B, 1, 1].  B=2, N=4096."""
    cond, x_t, nl, ref = _oracle_case(B, N)
    assert _clamped(ref) <= 0.25
    level = torch.from_numpy(nl).cuda()
    eps = _net("float32")(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), level.reshape(B, 1, 1) if B == 1 else level)
    assert tuple(eps.shape) == (B, 1, N)
    err = rms(eps.cpu().numpy(), ref)
    print(f"Waveunet B={B} N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f}, clamped {_clamped(ref):.3f})")
    assert err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_forward_16bit_at_the_config_length(torch_cuda, dtype):
    cond, x_t, nl, ref = _big_case()
    assert _clamped(ref) <= 0.25
    eps = _net(dtype)(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), torch.from_numpy(nl).cuda())
    rel = rms(eps.cpu().numpy(), ref) / rms(ref, 0)
    emu = O.forward(_params(), cond, x_t, nl, rounding=getattr(torch, dtype))
    emu = rms(emu, ref) / rms(ref, 0)
    print(f"Waveunet {dtype} B=2 N=16384: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {_bar16(dtype, emu):.3e})")
    assert rel <= _bar16(dtype, emu)


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")])
def test_sampling_matches_reference(torch_cuda, nc, mode):
    """The reference's unmodified SDDM.infer: the output and every intermediate x_t; a second run is
    bit-equal."""
    z = golden("waveunet.npz")
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
    print(f"Waveunet {nc} {mode}: rms of the output {err:.3e}, of x_t per step {['%.2e' % e for e in errs]}")
    assert err <= 1e-3
    assert max(errs) <= 1e-3
    assert torch.equal(out2.cpu(), torch.from_numpy(out))


def test_continuous_sampling_single_clip(torch_cuda):
    z = golden("waveunet.npz")
    cond = torch.from_numpy(z["inf/cond"][:1]).cuda()
    rec = _model("sr3").infer(cond, continuous=True, seed=7)
    assert len(rec) == 1 + SCHED[1]
    assert torch.equal(rec[0], cond)
    got = np.stack([r.cpu().numpy() for r in rec[1:]])
    assert got.shape[1:] == (1, 1, 2048)
    assert rms(got, z["inf/sqrt_alpha_bar/sr3/steps"][:, :1]) <= 1e-3


def test_row_sharding_is_bit_identical(torch_cuda):
    """Rows sampled in two shards (row_offset) equal the rows of one batch."""
    m = _model("conditional", dtype="bfloat16")
    cond, _, _ = _inputs(4, 2048, seed=1)
    cond = torch.from_numpy(cond).cuda()
    full = m.infer(cond, seed=11)
    a = m.infer(cond[:2].contiguous(), seed=11, row_offset=0)
    b = m.infer(cond[2:].contiguous(), seed=11, row_offset=2)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat([a, b]))


@pytest.mark.parametrize("N", [pytest.param(N, id=f"{N}-default") for N in (2048, 6144)])
def test_rows_are_independent_of_the_batch(torch_cuda, N):
    """Row b of a B = 5 forward equals the same clip run alone, bit for bit (bfloat16)."""
    net = _net("bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(5, N, seed=2))
    full = net(cond, x_t, nl)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    for b in range(5):
        one = net(cond[b:b + 1].contiguous(), x_t[b:b + 1].contiguous(), nl[b:b + 1].contiguous())
        assert torch.equal(full[b:b + 1], one), b


def test_rejects_bad_geometry(torch_cuda):
    net, m = _net(), _model()
    for N in (2056, 1024, 16380):
        z = torch.zeros(1, 1, N, device="cuda")
        with pytest.raises(AssertionError):
            net(z, z, torch.ones(1, device="cuda"))
        with pytest.raises(AssertionError):
            m.infer(z, seed=1)
    z = torch.zeros(0, 1, 2048, device="cuda")              # B = 0
    with pytest.raises((AssertionError, ValueError, RuntimeError)):
        net(z, z, torch.ones(0, device="cuda"))


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, _net(), hop_samples=2048).cuda()
    with pytest.raises(NotImplementedError):
        m.infer(torch.zeros(1, 1, 8, device="cuda"), seed=1)


@pytest.mark.parametrize("change", [{"num_channels": [24, 48, 72, 96]}, {"num_channels": [24 * i for i in range(1, 14)]},
                                    {"kernel_size": 3}, {"res": "fixed"}, {"conv_type": "bn"}, {"depth": 2},
                                    {"resample_kernel_size": 6}, {"resample_stride": 4}, {"num_inputs": 1}])
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, change):
    import sddm_hip
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": "Waveunet", "args": dict(O.ARGS, **change)}}
    with pytest.raises(NotImplementedError, match=next(iter(change))):
        sddm_hip.Context(cfg, 0)


def test_missing_params_counts_the_state_dict(torch_cuda):
    import sddm_hip
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": "Waveunet", "args": dict(O.ARGS)}}
    ctx = sddm_hip.Context(cfg, 0)
    assert ctx.missing() == 314
    ctx.load_state_dict({"noise_estimate_model." + k: v for k, v in _params().items()})
    assert ctx.missing() == 0
    ctx.close()


def test_sddm_forward_matches_oracle(torch_cuda):
    """SDDM.forward (evaluation only): q-sample at fixed t, then the network."""
    B, N = 2, 2048
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
    print(f"Waveunet SDDM.forward: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


def _write_pcm16(path, x, sr=16000):
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, 1, 1, sr, 2 * sr, 2, 16,
                      b"data", len(pcm))
    with open(path, "wb") as f:
        f.write(hdr + pcm)


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    """infer.py with configs/config_waveunet.json (chunks of 2048 samples, T = 3): WAV in, chunk,
    denoise, stitch, WAV out."""
    import infer
    import model.diffusion as D
    import model.model as M
    from data_loader import wav_io
    from parse_config import ConfigParser, read_json
    N = 2048
    rng = np.random.default_rng(4)
    for d in ("clean", "noisy"):
        os.makedirs(tmp_path / "data" / d)
    lengths = [4500, 700]
    for i, n in enumerate(lengths):
        c = 0.3 * np.sin(np.arange(n) * 0.05)
        _write_pcm16(tmp_path / "data" / "clean" / f"u{i}.wav", c)
        _write_pcm16(tmp_path / "data" / "noisy" / f"u{i}.wav", c + rng.uniform(-0.05, 0.05, n))
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_waveunet.json"))
    assert cfg["network"]["type"] == "Waveunet" and cfg["num_samples"] % 2048 == 0
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
