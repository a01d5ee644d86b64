"""GPU: UNetTST (reference model/UNetTST.py:270-392, config_unettst.json) and its Dual_Transformer
(UNetTST.py:184-233) under SDDM.infer (model.py:50-124) through the facade and libsddm_hip, against
goldens generated from the reference and the torch oracle pinned by test_unettst.py.

The test that pins the block's wiring is test_dual_transformer_matches_reference: float32, the block
alone, relative rms <= 2e-5.  Swapping the r / z gates of the last column GRU moves the block's output
by 3.9e-4 ... 8.0e-4 relative at dim2 >= 2 (test_unettst.py prints it) and the whole network's by at
most 2.5e-4, which the float32 network bar (1e-4 x max(1, rms)) does not always see.

16-bit bars (_bar16, as test_gpu_waveunet.py): the project's 3e-2 (bfloat16) / 5e-3 (float16) where
the CPU emulation (the oracle's `rounding`: what the kernels round) is at most half of it, else twice
the emulation.  The emulation rounds the block's matrix weights, its output and, since the kernel's
16-bit MFMAs take them so, the activations where they enter a matrix product.  CPU emulation, relative
rms against the float64 oracle:
  Dual_Transformer (2,4) / (8,4)   bfloat16 3.83e-3 / 4.07e-3   float16 5.00e-4 / 5.01e-4
  forward B=2, N=4160 / 16448      bfloat16 1.11e-2 / 1.12e-2   float16 1.41e-3 / 1.41e-3
so every bar is the project's.  Measured on MI355X (rms of the difference / rms of the reference
unless noted):
  Dual_Transformer vs golden, float32, five shapes   3.4e-7 ... 3.8e-7   (bar 2e-5)
  Dual_Transformer vs oracle (2,4) / (8,4)           bfloat16 3.82e-3 / 4.07e-3   float16 5.01e-4 / 5.02e-4
  Dual_Transformer(160, 160, 0, 2) alone, 5x4, B=3   3.0e-7
  forward vs golden, B=2, N=4160                     float32 8.6e-7 rms   bfloat16 1.10e-2   float16 1.45e-3
  forward vs oracle, float32, N=2112 / 6208 / 16448  6.4e-7 / 7.0e-7 / 7.2e-7 rms
  forward vs oracle, B=2, N=16448                    bfloat16 1.13e-2   float16 1.39e-3
  sampling vs golden, every x_t, six cases           <= 3.1e-7 rms
  SDDM.forward vs oracle                             8.1e-7 rms;   n_TSTB=1 vs oracle 6.9e-7 rms
  rows                                               bit-equal in the three dtypes, forward and block
  res_blocks=2 vs oracle, N=4160 / 16448             float32 6.0e-7 / 6.1e-7 rms   bfloat16 1.01e-2   float16 1.28e-3
  res_blocks=3 vs oracle, N=2112                     float32 5.7e-7 rms
"""
import functools
import json
import os
import struct

import numpy as np
import pytest
import torch

import _unettst_oracle as O
from _helpers import golden, rms
from _weights import make_params

pytestmark = pytest.mark.gpu

SCHED = ("linear", 3, 1e-4, 0.05)
MODES = ("original", "condition_in", "sr3", "supportive", "conditional")
DT_SHAPES = ((1, 4), (2, 4), (3, 4), (8, 4), (2, 8))
DTYPES = ("float32", "bfloat16", "float16")
_NETS = {}


def _args(**change):
    return dict(O.ARGS, **change)


@functools.lru_cache(maxsize=None)
def _params(res_blocks=1, n_tstb=6):
    return make_params(O.param_shapes(_args(res_blocks=res_blocks, n_TSTB=n_tstb)), 0)


def _net(N, dtype="float32", res_blocks=1, n_tstb=6):
    """One facade network per (length, dtype, variant), shared by the tests (its weights never change)."""
    key = (N, dtype, res_blocks, n_tstb)
    if key not in _NETS:
        import model.network as NW
        n = NW.UNetTST(num_samples=N, **_args(res_blocks=res_blocks, n_TSTB=n_tstb))
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _params(res_blocks, n_tstb).items()})
        n.compute_dtype = dtype
        n.mid.compute_dtype = dtype
        _NETS[key] = n.cuda()
    return _NETS[key]


def _model(N, mode="original", noise_condition="sqrt_alpha_bar", dtype="float32"):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    return M.SDDM(d, _net(N, dtype), noise_condition=noise_condition, p_transition=mode, compute_dtype=dtype).cuda()


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


def _run(net, cond, x_t, nl):
    return net(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), torch.from_numpy(nl).cuda()).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _oracle_case(B, N, res_blocks=1, n_tstb=6):
    cond, x_t, nl = _inputs(B, N, seed=31)
    return cond, x_t, nl, O.forward(_params(res_blocks, n_tstb), cond, x_t, nl, args=_args(res_blocks=res_blocks, n_TSTB=n_tstb))


# ---- 1, 2: the block alone
@pytest.mark.parametrize("dim2,dim1", DT_SHAPES)
def test_dual_transformer_matches_reference(torch_cuda, dim2, dim1):
    z = golden("unettst.npz")
    x, ref = z[f"dt/{dim2}x{dim1}/x"], z[f"dt/{dim2}x{dim1}/y"]
    y = _net(4160).mid(torch.from_numpy(x).cuda()).cpu().numpy()
    assert y.shape == ref.shape
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x{dim1} float32: relative rms vs reference {rel:.3e}")
    assert np.isfinite(y).all() and rel <= 2e-5


@pytest.mark.parametrize("dim2,dim1", [(2, 4), (8, 4)])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_dual_transformer_16bit_matches_oracle(torch_cuda, dtype, dim2, dim1):
    z = golden("unettst.npz")
    x = z[f"dt/{dim2}x{dim1}/x"]
    ref = O.dual_transformer(_params(), x)
    emu = rms(O.dual_transformer(_params(), x, rounding=getattr(torch, dtype)), ref) / rms(ref, 0)
    y = _net(4160, dtype).mid(torch.from_numpy(x).cuda()).cpu().numpy()
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x{dim1} {dtype}: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {_bar16(dtype, emu):.3e})")
    assert np.isfinite(y).all() and rel <= _bar16(dtype, emu)


def test_dual_transformer_alone_as_a_module(torch_cuda):
    """A stand-alone Dual_Transformer(160, 160, 0, 2) (its own context; only mid.* is loaded)."""
    import model.network as NW
    shapes = {k[4:]: s for k, s in O.dual_transformer_shapes(160, 2).items()}
    P = make_params(shapes, 3)
    m = NW.Dual_Transformer(160, 160, 0, 2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    x = np.random.default_rng(5).standard_normal((3, 160, 5, 4)).astype(np.float32)
    ref = O.dual_transformer(P, x, n_tstb=2, prefix="")
    y = m.cuda()(torch.from_numpy(x).cuda()).cpu().numpy()
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer(160, 160, 0, 2) alone, 5x4, B=3: relative rms vs oracle {rel:.3e}")
    assert rel <= 2e-5
    with pytest.raises(NotImplementedError, match="tokens"):
        m(torch.zeros(1, 160, 17, 4, device="cuda"))


# ---- 3: the whole forward
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_matches_reference(torch_cuda, dtype):
    z = golden("unettst.npz")
    ref = z["fw/eps"]
    eps = _run(_net(4160, dtype), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape and np.isfinite(eps).all()
    err = rms(eps, ref)
    print(f"UNetTST {dtype} B=2 N=4160: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    if dtype == "float32":
        assert err <= 1e-4 * _gate(ref)
    else:
        emu = O.forward(_params(), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], rounding=getattr(torch, dtype))
        emu = rms(emu, ref) / rms(ref, 0)
        print(f"UNetTST {dtype}: CPU emulation relative {emu:.3e}, bar {_bar16(dtype, emu):.3e}")
        assert err / rms(ref, 0) <= _bar16(dtype, emu)


@pytest.mark.parametrize("B,N", [(3, 2112), (3, 6208), (2, 16448)])
def test_forward_matches_oracle(torch_cuda, B, N):
    """mid sees [B,160,1,4], [B,160,3,4] and, at the config's length (the shipped tuning table applies
    under SDDM; the facade network alone plans by the heuristics), [B,160,8,4]."""
    cond, x_t, nl, ref = _oracle_case(B, N)
    eps = _run(_net(N), cond, x_t, nl)
    err = rms(eps, ref)
    print(f"UNetTST float32 B={B} N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f})")
    assert eps.shape == (B, 1, N) and err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_forward_16bit_at_the_config_length(torch_cuda, dtype):
    """B = 2, N = 16448 through SDDM's context, i.e. on the shipped tuning table (its chain and mid.0
    entries are ignored for UNetTST)."""
    cond, x_t, nl, ref = _oracle_case(2, 16448)
    m = _model(16448, dtype=dtype)
    eps = torch.empty(2, 1, 16448, device="cuda")
    m._context(eps.device).network_forward(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(),
                                           torch.from_numpy(nl).cuda(), eps)
    rel = rms(eps.cpu().numpy(), ref) / rms(ref, 0)
    emu = rms(O.forward(_params(), cond, x_t, nl, rounding=getattr(torch, dtype)), ref) / rms(ref, 0)
    print(f"UNetTST {dtype} B=2 N=16448: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {_bar16(dtype, emu):.3e})")
    assert rel <= _bar16(dtype, emu)


# ---- 4: rows are bit-identical
@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_are_independent_of_the_batch(torch_cuda, dtype):
    net = _net(6208, dtype)
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(3, 6208, seed=2))
    full = net(cond, x_t, nl)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((3, 160, 3, 4)).astype(np.float32)).cuda()
    blk = net.mid(x)
    assert torch.isfinite(blk).all() and float(blk.abs().max()) > 0
    for b in range(3):
        one = net(cond[b:b + 1].contiguous(), x_t[b:b + 1].contiguous(), nl[b:b + 1].contiguous())
        assert torch.equal(full[b:b + 1], one), b
        assert torch.equal(blk[b:b + 1], net.mid(x[b:b + 1].contiguous())), b


# ---- 5: sampling
@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")])
def test_sampling_matches_reference(torch_cuda, nc, mode):
    """The reference's unmodified SDDM.infer: the output and every intermediate x_t; a second run is
    bit-equal."""
    z = golden("unettst.npz")
    steps = z[f"inf/{nc}/{mode}/steps"]
    cond = torch.from_numpy(z["inf/cond"]).cuda()
    m = _model(4160, mode, nc)
    out = m.infer(cond, seed=7).cpu().numpy()
    assert out.shape == steps[-1].shape
    err = rms(out, steps[-1])
    T = SCHED[1]
    record = torch.empty((T,) + tuple(cond.shape), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(cond)
    m._context(cond.device).sample_continuous(cond, out2, record, 1, 7, 0)
    errs = [rms(record[i].cpu().numpy(), steps[i]) for i in range(T)]
    print(f"UNetTST {nc} {mode}: rms of the output {err:.3e}, of x_t per step {['%.2e' % e for e in errs]}")
    assert err <= 1e-3
    assert max(errs) <= 1e-3
    assert torch.equal(out2.cpu(), torch.from_numpy(out))


def test_continuous_sampling_single_clip(torch_cuda):
    z = golden("unettst.npz")
    cond = torch.from_numpy(z["inf/cond"][:1]).cuda()
    rec = _model(4160, "sr3").infer(cond, continuous=True, seed=7)
    assert len(rec) == 1 + SCHED[1]
    assert torch.equal(rec[0], cond)
    got = np.stack([r.cpu().numpy() for r in rec[1:]])
    assert rms(got, z["inf/sqrt_alpha_bar/sr3/steps"][:, :1]) <= 1e-3


def test_row_sharding_is_bit_identical(torch_cuda):
    """Rows sampled in two shards (row_offset) equal the rows of one batch; sharded_infer without a
    process group is model.infer."""
    import model.model as M
    m = _model(4160, "conditional", dtype="bfloat16")
    cond = torch.from_numpy(_inputs(4, 4160, seed=1)[0]).cuda()
    full = m.infer(cond, seed=11)
    a = m.infer(cond[:2].contiguous(), seed=11, row_offset=0)
    b = m.infer(cond[2:].contiguous(), seed=11, row_offset=2)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat([a, b]))
    assert torch.equal(M.sharded_infer(m, cond, seed=11), full)


def test_sddm_forward_matches_oracle(torch_cuda):
    """SDDM.forward (evaluation only): q-sample at fixed t, then the network."""
    B, N = 2, 4160
    rng = np.random.default_rng(23)
    target = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, N)).astype(np.float32)).cuda()
    cond = (target + torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 1, N)).astype(np.float32)).cuda())
    noise = torch.from_numpy(rng.standard_normal((B, 1, N)).astype(np.float32)).cuda()
    m = _model(N)
    with torch.no_grad():
        predicted, got_noise = m(target, cond, noise=noise, t=torch.tensor([3, 1]), random_step=torch.tensor([0.25, 0.75]))
    assert torch.equal(got_noise, noise) and tuple(predicted.shape) == (B, 1, N)
    x_t, level, _ = m.diffusion.q_stochastic(target, noise, t=torch.tensor([3, 1]), random_step=torch.tensor([0.25, 0.75]))
    ref = O.forward(_params(), cond.cpu().numpy(), x_t.cpu().numpy(), level.cpu().numpy())
    err = rms(predicted.cpu().numpy(), ref)
    print(f"UNetTST SDDM.forward: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, _net(4160), hop_samples=256).cuda()
    with pytest.raises(NotImplementedError):
        m.infer(torch.zeros(1, 513, 8, device="cuda"), seed=1)


# ---- 6: configure-time refusals, and variants that must build
def _cfg(num_samples=4160, **change):
    return {"arch": {"type": "SDDM", "args": {}},
            "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
            "network": {"type": "UNetTST", "args": _args(**change)}, "num_samples": num_samples}


@pytest.mark.parametrize("name,cfg", [("channel_mults", _cfg(channel_mults=[1, 2, 3, 4, 6])),
                                      ("channel_mults", _cfg(channel_mults=[1, 2, 3, 4])),
                                      ("inner_channel", _cfg(inner_channel=64, channel_mults=[1, 1, 2, 2, 2])),
                                      ("n_TSTB", _cfg(n_TSTB=0)),
                                      ("res_blocks", _cfg(res_blocks=0)),
                                      ("num_samples", _cfg(num_samples=34880))])
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, name, cfg):
    import sddm_hip
    with pytest.raises(NotImplementedError, match=name):
        sddm_hip.Context(cfg, 0)


def test_the_token_budget_admits_64(torch_cuda):
    import sddm_hip
    ctx = sddm_hip.Context(_cfg(num_samples=32832), 0)          # mid sees [B, 160, 16, 4]
    assert ctx.missing() == 454
    ctx.close()


@pytest.mark.parametrize("res_blocks,n_tstb", [(1, 1), (2, 6)])
def test_variants_build_and_match_oracle(torch_cuda, res_blocks, n_tstb):
    """n_TSTB = 1 and res_blocks = 2 must build and match the oracle.  At res_blocks = 2 four decoder
    blocks read cat(128, 160), cat(96, 128), cat(64, 96) and cat(32, 64) channels, whose GroupNorm
    groups of 9, 7, 5 and 3 channels straddle the concatenation: the plan copies those into one
    tensor with statistics of its own (concat_kernel) before the block's first conv."""
    cond, x_t, nl, ref = _oracle_case(2, 4160, res_blocks, n_tstb)
    eps = _run(_net(4160, "float32", res_blocks, n_tstb), cond, x_t, nl)
    err = rms(eps, ref)
    print(f"UNetTST res_blocks={res_blocks} n_TSTB={n_tstb}: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("res_blocks,B,N", [(3, 2, 2112), (2, 1, 16448)])
def test_more_res_blocks_match_oracle(torch_cuda, res_blocks, B, N):
    """The reference's default res_blocks = 3 at the smallest length, and res_blocks = 2 at the
    config's length (the concatenations at 128 x 64 ... 16 x 8 positions)."""
    cond, x_t, nl, ref = _oracle_case(B, N, res_blocks, 6)
    eps = _run(_net(N, "float32", res_blocks, 6), cond, x_t, nl)
    err = rms(eps, ref)
    print(f"UNetTST res_blocks={res_blocks} B={B} N={N}: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * _gate(ref)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_res_blocks_2_in_16bit(torch_cuda, dtype):
    """The concatenated decoder inputs of res_blocks = 2 through the 16-bit kernels, and row 0 alone
    bit-equal to row 0 of the batch."""
    cond, x_t, nl, ref = _oracle_case(2, 4160, 2, 6)
    net = _net(4160, dtype, 2, 6)
    eps = _run(net, cond, x_t, nl)
    rel = rms(eps, ref) / rms(ref, 0)
    emu = O.forward(_params(2, 6), cond, x_t, nl, rounding=getattr(torch, dtype), args=_args(res_blocks=2))
    emu = rms(emu, ref) / rms(ref, 0)
    print(f"UNetTST res_blocks=2 {dtype}: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {_bar16(dtype, emu):.3e})")
    assert np.isfinite(eps).all() and rel <= _bar16(dtype, emu)
    assert np.array_equal(_run(net, cond[:1], x_t[:1], nl[:1]), eps[:1])


# ---- 7: infer.py
def _write_pcm16(path, x, sr=16000):
    pcm = np.clip(np.round(x * 32768), -32768, 32767).astype("<i2").tobytes()
    hdr = struct.pack("<4sI4s4sIHHIIHH4sI", b"RIFF", 36 + len(pcm), b"WAVE", b"fmt ", 16, 1, 1, sr, 2 * sr, 2, 16,
                      b"data", len(pcm))
    with open(path, "wb") as f:
        f.write(hdr + pcm)


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    """infer.py with configs/config_unettst.json at chunks of 4160 samples and T = 3: WAV in, chunk,
    denoise, stitch, WAV out."""
    import infer
    import model.diffusion as D
    import model.model as M
    from data_loader import wav_io
    from parse_config import ConfigParser, read_json
    N = 4160
    rng = np.random.default_rng(4)
    for d in ("clean", "noisy"):
        os.makedirs(tmp_path / "data" / d)
    lengths = [9000, 700]
    for i, n in enumerate(lengths):
        c = 0.3 * np.sin(np.arange(n) * 0.05)
        _write_pcm16(tmp_path / "data" / "clean" / f"u{i}.wav", c)
        _write_pcm16(tmp_path / "data" / "noisy" / f"u{i}.wav", c + rng.uniform(-0.05, 0.05, n))
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_unettst.json"))
    assert cfg["network"]["type"] == "UNetTST" and cfg["num_samples"] == 16448
    cfg["num_samples"] = N
    cfg["diffusion"]["args"].update({"n_timestep": 3, "linear_end": 0.05})
    cfg["infer_dataset"]["args"]["data_root"] = str(tmp_path / "data")
    cfg["infer_data_loader"]["args"].update({"batch_size": 1, "num_workers": 0})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    ref_model = M.SDDM(D.GaussianDiffusion("linear", 3, 1e-4, 0.05, device="cpu"), _net(N))
    ck = tmp_path / "model_best.pth"
    torch.save({"arch": "SDDM", "epoch": 1,
                "state_dict": {"module." + k: v.cpu() for k, v in ref_model.state_dict().items()},
                "config": json.loads(json.dumps(cfg))}, ck)
    config = ConfigParser(cfg, resume=ck, run_id="e2e")
    log = infer.main(config, seed=100)
    assert np.isfinite(log["loss"])
    for i, n in enumerate(lengths):
        out, sr = wav_io.load(os.path.join(str(config.save_dir), "samples", "output", f"u{i}.wav"))
        assert sr == 16000 and out.shape[1] % N == 0 and out.shape[1] >= n
        assert torch.isfinite(out).all() and float(out.abs().max()) > 0
