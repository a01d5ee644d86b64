"""GPU: UNetModified (reference model/UNetModified.py:192-323, config_unetmodified.json) and its
SelfAttention (UNetModified.py:140-169) under SDDM.infer (model.py:50-124) through the facade and
libsddm_hip, against goldens generated from the reference and the torch oracle pinned by
test_unetmodified.py.  Every weight set is make_params with the q / k rows of the attention's qkv weights
times QK_SCALE (the oracle's `sharpen`): _net_suite builds its weights with make_params alone, so this
module wraps that one function while its tests run.

The tests that pin the attention are the block alone in float32: the golden shapes cover P = 1 (the
softmax is 1), 16 and 24 (below one MFMA tile), C = 160, P = 65 (one past a tile edge: query tiles of 13,
a key tile of one key) and P = 128; P = 512 and 2048 need 16 and 64 key tiles and as many rescales; with
the q / k rows times 12 the logits reach 204, which exp without a running maximum turns into inf.

16-bit bars (_bar16, as test_gpu_unettst.py): the project's 3e-2 (bfloat16) / 5e-3 (float16) where the
CPU emulation (the oracle's `rounding`: what the kernels round) is at most half of it, else twice the
emulation.

CPU emulation, relative rms against the float64 oracle:
  SelfAttention 256x16x8 / 128x32x16   bfloat16 2.99e-3 / 2.86e-3   float16 3.56e-4 / 3.50e-4
  forward B=2, N=16448                 bfloat16 1.79e-2 (so the bar is twice it, 3.58e-2)   float16 2.17e-3
Measured on MI355X (rms of the difference / rms of the reference unless noted):
  SelfAttention vs golden, float32, five shapes       1.4e-7 ... 2.7e-7   (bar 2e-5)
  SelfAttention vs oracle, float32, P = 512 / 2048    1.9e-7 / 1.9e-7
  SelfAttention, q / k rows x 12 (max |logit| 204)    1.34e-6; the reference's own float32 result 1.35e-6, bar 2e-5
  SelfAttention vs oracle 256x16x8 / 128x32x16        bfloat16 2.98e-3 / 2.86e-3   float16 3.57e-4 / 3.50e-4
  forward vs golden, B=2, N=2112                      float32 1.7e-6 rms   bfloat16 1.73e-2   float16 2.23e-3
  forward vs oracle, res_blocks 2, attn [3, 4], N=3136  float32 1.2e-6 rms
  forward vs oracle, B=2, N=16448                     bfloat16 1.72e-2   float16 2.20e-3
  sampling vs golden, every x_t, six cases            <= 7.0e-7 rms
  SDDM.forward vs oracle                              1.9e-6 rms
  rows                                                bit-equal (bfloat16 forward and block, sharded sampling)
"""
import functools

import numpy as np
import pytest
import torch

import _net_suite as S
import _unetmodified_oracle as O
from _helpers import golden, rms
from _weights import make_params

pytestmark = pytest.mark.gpu

AT_SHAPES = ((256, 1, 1), (256, 2, 8), (160, 3, 8), (256, 5, 13), (256, 16, 8))
DTYPES = ("float32", "bfloat16", "float16")
CASE = S.NetCase("UNetModified", O, "unetmodified.npz", 2112, dual_transformer=True, rounding=True, emulated_bar16=True,
                 state_dict_count=242, refusal_match=True, spec_hop=256, spec_input=(1, 513, 8), sharded_infer=True,
                 cli_config="config_unetmodified.json", cli_chunk=2112, cli_lengths=(5000, 700),
                 cli_num_samples=("==", 16448), cli_exact_shape=False)
WIDE = {"res_blocks": 2, "attn_layer": [3, 4]}      # the variant of test_forward_res_blocks_2_matches_oracle
_NETS, _ATTN = {}, {}


@pytest.fixture(autouse=True, scope="module")
def _sharpened_weights():
    """_net_suite's weights of this module's case get QK_SCALE (other cases have no attn.qkv.weight)."""
    plain = S.make_params
    S.make_params = lambda shapes, seed=0: O.sharpen(plain(shapes, seed))
    yield
    S.make_params = plain


def _net(N, dtype="float32"):
    return S.net(CASE, N, dtype)


@functools.lru_cache(maxsize=None)
def _wide_params():
    return O.make_params(dict(O.ARGS, **WIDE))


@functools.lru_cache(maxsize=None)
def _wide_case(B, N):
    """Inputs and the oracle's output of the WIDE variant (its lists do not fit _net_suite's variant keys)."""
    cond, x_t, nl = S.inputs(B, N, seed=31)
    return cond, x_t, nl, O.forward(_wide_params(), cond, x_t, nl, args=dict(O.ARGS, **WIDE))


def _wide_net(N, dtype="float32"):
    if (N, dtype) not in _NETS:
        import model.network as NW
        n = NW.UNetModified(num_samples=N, **dict(O.ARGS, **WIDE))
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _wide_params().items()})
        n.compute_dtype = dtype
        _NETS[(N, dtype)] = n.cuda()
    return _NETS[(N, dtype)]


def _attn_params(C, scale=O.QK_SCALE):
    shapes = O.param_shapes() if C == 256 else O.attention_shapes(C, "mid.0.attn.")
    return O.sharpen({k: v for k, v in make_params(shapes, 0).items() if k.startswith("mid.0.attn.")}, scale)


def _attention(C, dtype="float32", scale=O.QK_SCALE):
    """A stand-alone SelfAttention(C) carrying the mid.0.attn weights of that width."""
    key = (C, dtype, scale)
    if key not in _ATTN:
        import model.network as NW
        m = NW.SelfAttention(C)
        m.load_state_dict({k[len("mid.0.attn."):]: torch.from_numpy(v) for k, v in _attn_params(C, scale).items()})
        m.compute_dtype = dtype
        _ATTN[key] = m.cuda()
    return _ATTN[key]


def _run_block(m, x):
    return m(torch.from_numpy(x).cuda()).cpu().numpy()


# ---- 1: the block alone
@pytest.mark.parametrize("C,H,W", AT_SHAPES)
def test_self_attention_matches_reference(torch_cuda, C, H, W):
    """float32 against the reference's output; C = 256 runs the network's own mid.0.attn module."""
    z = golden("unetmodified.npz")
    x, ref = z[f"at/{C}x{H}x{W}/x"], z[f"at/{C}x{H}x{W}/y"]
    m = _net(2112).mid[0].attn if C == 256 else _attention(C)
    y = _run_block(m, x)
    assert y.shape == ref.shape
    rel = rms(y, ref) / rms(ref, 0)
    print(f"SelfAttention {C}x{H}x{W} float32: relative rms vs reference {rel:.3e}")
    assert np.isfinite(y).all() and rel <= 2e-5


@pytest.mark.parametrize("C,H,W", [(128, 32, 16), (64, 64, 32)])
def test_self_attention_many_key_tiles_matches_oracle(torch_cuda, C, H, W):
    """P = 512 and 2048: 16 and 64 key tiles, 8 and 32 query tiles per image."""
    x = np.random.default_rng(17).standard_normal((2, C, H, W)).astype(np.float32)
    ref = O.self_attention(_attn_params(C), "mid.0.attn.", x)
    y = _run_block(_attention(C), x)
    rel = rms(y, ref) / rms(ref, 0)
    std, pmax, amax = O.logit_stats(_attn_params(C), "mid.0.attn.", x)
    print(f"SelfAttention {C}x{H}x{W} float32: relative rms vs oracle {rel:.3e} (logit std {std:.2f}, row-max probability {pmax:.3f})")
    assert np.isfinite(y).all() and rel <= 2e-5


def test_self_attention_large_logits(torch_cuda):
    """q / k rows times 12: max |logit| 204, beyond what exp holds in float32 without the running
    maximum.  Bar: 4 x the relative error of the reference's own float32 CPU result (the golden's at12/)
    against the float64 oracle on the same input, at least 2e-5; the factor allows for another summation order."""
    z = golden("unetmodified.npz")
    x, ref32 = z["at/256x16x8/x"], z["at12/256x16x8/y"]
    P = _attn_params(256, 12.0)
    ref = O.self_attention(P, "mid.0.attn.", x)
    std, pmax, amax = O.logit_stats(P, "mid.0.attn.", x)
    own = rms(ref32, ref) / rms(ref, 0)
    y = _run_block(_attention(256, scale=12.0), x)
    assert np.isfinite(y).all()
    rel = rms(y, ref) / rms(ref, 0)
    print(f"SelfAttention 256x16x8, q / k rows x 12 (max |logit| {amax:.0f}): relative rms vs float64 oracle {rel:.3e}; "
          f"the reference's float32 CPU result {own:.3e}, bar {max(4 * own, 2e-5):.3e}")
    assert amax > 128 and rel <= max(4 * own, 2e-5)


@pytest.mark.parametrize("C,H,W", [(256, 16, 8), (128, 32, 16)])
@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_self_attention_16bit_matches_oracle(torch_cuda, dtype, C, H, W):
    x = golden("unetmodified.npz")["at/256x16x8/x"] if C == 256 else \
        np.random.default_rng(17).standard_normal((2, C, H, W)).astype(np.float32)
    P = _attn_params(C)
    ref = O.self_attention(P, "mid.0.attn.", x)
    emu = rms(O.self_attention(P, "mid.0.attn.", x, rounding=getattr(torch, dtype)), ref) / rms(ref, 0)
    y = _run_block(_attention(C, dtype), x)
    rel = rms(y, ref) / rms(ref, 0)
    print(f"SelfAttention {C}x{H}x{W} {dtype}: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {S.bar16(dtype, emu):.3e})")
    assert np.isfinite(y).all() and rel <= S.bar16(dtype, emu)


def test_self_attention_refusals(torch_cuda):
    import sddm_hip
    m = _attention(128)
    with pytest.raises(AssertionError):
        m(torch.zeros(1, 64, 2, 2, device="cuda"))
    ctx = m._context(torch.device("cuda", 0))
    x = torch.zeros(1, 128, 2, 2, device="cuda")
    with pytest.raises(ValueError, match="no attention layer"):
        ctx.self_attention("downs.0.attn", x, torch.empty_like(x))
    with pytest.raises(NotImplementedError, match="512 channels"):
        sddm_hip.Context(S.config(CASE, 2112, channel_mults=[1, 2, 4, 8, 16]), 0)


# ---- 2: the whole forward
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_matches_reference(torch_cuda, dtype):
    z = golden("unetmodified.npz")
    ref = z["fw/eps"]
    eps = S.run(_net(2112, dtype), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape and np.isfinite(eps).all()
    err = rms(eps, ref)
    print(f"UNetModified {dtype} B=2 N=2112: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    if dtype == "float32":
        assert err <= 1e-4 * S.gate(ref)
    else:
        emu = S.oracle_forward(CASE, z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], rounding=dtype)
        emu = rms(emu, ref) / rms(ref, 0)
        print(f"UNetModified {dtype}: CPU emulation relative {emu:.3e}, bar {S.bar16(dtype, emu):.3e}")
        assert err / rms(ref, 0) <= S.bar16(dtype, emu)


def test_forward_res_blocks_2_matches_oracle(torch_cuda):
    """res_blocks 2, attn_layer [3, 4], N = 3136, B = 2: levels of 48 x 128 ... 3 x 8, attention over 96 and
    24 positions (query tiles of 48 and 24), and real concatenations where a GroupNorm group straddles
    cat(x, skip)."""
    cond, x_t, nl, ref = _wide_case(2, 3136)
    eps = S.run(_wide_net(3136), cond, x_t, nl)
    err = rms(eps, ref)
    print(f"UNetModified res_blocks=2 attn_layer=[3, 4] float32 B=2 N=3136: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f})")
    assert eps.shape == (2, 1, 3136) and err <= 1e-4 * S.gate(ref)


@pytest.mark.parametrize("dtype", ["bfloat16", "float16"])
def test_forward_16bit_at_the_config_length(torch_cuda, dtype):
    cond, x_t, nl, ref = S.oracle_case(CASE, 2, 16448)
    eps = S.run(_net(16448, dtype), cond, x_t, nl)
    rel = rms(eps, ref) / rms(ref, 0)
    emu = rms(S.oracle_forward(CASE, cond, x_t, nl, rounding=dtype), ref) / rms(ref, 0)
    print(f"UNetModified {dtype} B=2 N=16448: relative rms vs oracle {rel:.3e} (CPU emulation {emu:.3e}, bar {S.bar16(dtype, emu):.3e})")
    assert np.isfinite(eps).all() and rel <= S.bar16(dtype, emu)


# ---- 3: rows are bit-identical
def test_rows_in_two_parts(torch_cuda):
    """A B = 5 forward equals its rows 0-1 and 2-4 run on their own, bit for bit (bfloat16), and so does the block."""
    n = _net(2112, "bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in S.inputs(5, 2112, seed=2))
    full = n(cond, x_t, nl)
    parts = [n(cond[s].contiguous(), x_t[s].contiguous(), nl[s].contiguous()) for s in (slice(0, 2), slice(2, 5))]
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat(parts))
    m = _attention(256, "bfloat16")
    x = torch.from_numpy(np.random.default_rng(9).standard_normal((5, 256, 5, 13)).astype(np.float32)).cuda()
    blk = m(x)
    assert torch.equal(blk, torch.cat([m(x[:2].contiguous()), m(x[2:].contiguous())]))


def test_row_sharding_is_bit_identical(torch_cuda):
    S.check_row_sharding(CASE)


# ---- 4: sampling
@pytest.mark.parametrize("nc,mode", S.SAMPLING_CASES)
def test_sampling_matches_reference(torch_cuda, nc, mode):
    S.check_sampling_matches_reference(CASE, nc, mode)


def test_continuous_sampling_single_clip(torch_cuda):
    S.check_continuous_sampling_single_clip(CASE)


def test_sddm_forward_matches_oracle(torch_cuda):
    S.check_sddm_forward_matches_oracle(CASE)


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    S.check_spectrogram_arch_is_not_implemented(CASE)


def test_missing_params(torch_cuda):
    S.check_missing_params(CASE)


# ---- 5: refusals
def test_rejects_bad_geometry(torch_cuda):
    n, m = _net(2112), S.model(CASE, 2112)
    for N in (2100, 2176):                        # not whole frames; not the length the network was built for
        z = torch.zeros(1, 1, N, device="cuda")
        with pytest.raises(AssertionError):
            n(z, z, torch.ones(1, device="cuda"))
        with pytest.raises(AssertionError):
            m.infer(z, seed=1)


@pytest.mark.parametrize("name,cfg", [("attn_layer", S.config(CASE, 2112, attn_layer=4)),
                                      ("with_noise_level_emb", S.config(CASE, 2112, with_noise_level_emb=False)),
                                      ("inner_channel", S.config(CASE, 2112, inner_channel=64)),
                                      ("num_samples", S.config(CASE, 128 + 30 * 64))])
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, name, cfg):
    import sddm_hip
    with pytest.raises((NotImplementedError, ValueError, AssertionError), match=name if name != "num_samples" else "n_frames"):
        sddm_hip.Context(cfg, 0)


# ---- 6: infer.py
def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    S.check_infer_cli_end_to_end(CASE, tmp_path)
