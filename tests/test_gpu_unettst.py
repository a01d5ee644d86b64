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

import numpy as np
import pytest
import torch

import _net_suite as S
import _unettst_oracle as O
from _helpers import golden, rms
from _weights import make_params

pytestmark = pytest.mark.gpu

DT_SHAPES = ((1, 4), (2, 4), (3, 4), (8, 4), (2, 8))
DTYPES = ("float32", "bfloat16", "float16")
CASE = S.NetCase("UNetTST", O, "unettst.npz", 4160, dual_transformer=True, rounding=True, emulated_bar16=True,
                 refusal_match=True, spec_hop=256, spec_input=(1, 513, 8), continuous_shape=False, sharded_infer=True,
                 cli_config="config_unettst.json", cli_chunk=4160, cli_lengths=(9000, 700), cli_num_samples=("==", 16448),
                 cli_exact_shape=False)
_args, _inputs, _gate, _bar16, _run = functools.partial(S.args, CASE), S.inputs, S.gate, S.bar16, S.run


def _params(res_blocks=1, n_tstb=6):
    return S.params(CASE, res_blocks=res_blocks, n_TSTB=n_tstb)


def _net(N, dtype="float32", res_blocks=1, n_tstb=6):
    return S.net(CASE, N, dtype, res_blocks=res_blocks, n_TSTB=n_tstb)


def _model(N, mode="original", noise_condition="sqrt_alpha_bar", dtype="float32"):
    return S.model(CASE, N, mode, noise_condition, dtype)


def _oracle_case(B, N, res_blocks=1, n_tstb=6):
    return S.oracle_case(CASE, B, N, res_blocks=res_blocks, n_TSTB=n_tstb)


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
@pytest.mark.parametrize("nc,mode", S.SAMPLING_CASES)
def test_sampling_matches_reference(torch_cuda, nc, mode):
    S.check_sampling_matches_reference(CASE, nc, mode)


def test_continuous_sampling_single_clip(torch_cuda):
    S.check_continuous_sampling_single_clip(CASE)


def test_row_sharding_is_bit_identical(torch_cuda):
    S.check_row_sharding(CASE)


def test_sddm_forward_matches_oracle(torch_cuda):
    S.check_sddm_forward_matches_oracle(CASE)


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    S.check_spectrogram_arch_is_not_implemented(CASE)


# ---- 6: configure-time refusals, and variants that must build
def _cfg(num_samples=4160, **change):
    return S.config(CASE, num_samples, **change)


@pytest.mark.parametrize("name,cfg", [("channel_mults", _cfg(channel_mults=[1, 2, 3, 4, 6])),
                                      ("channel_mults", _cfg(channel_mults=[1, 2, 3, 4])),
                                      ("inner_channel", _cfg(inner_channel=64, channel_mults=[1, 1, 2, 2, 2])),
                                      ("n_TSTB", _cfg(n_TSTB=0)),
                                      ("res_blocks", _cfg(res_blocks=0)),
                                      ("num_samples", _cfg(num_samples=34880))])
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, name, cfg):
    S.check_refused_at_configure(CASE, cfg, name)


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
def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    S.check_infer_cli_end_to_end(CASE, tmp_path)
