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
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _net_suite as S
import _wu_paths_child as child
from _waveunet_film_oracle import WAVEUNET as O
from _helpers import golden, rms

pytestmark = pytest.mark.gpu

REFUSED = ({"num_channels": [24, 48, 72, 96]}, {"num_channels": [24 * i for i in range(1, 14)]},
           {"kernel_size": 3}, {"res": "fixed"}, {"conv_type": "bn"}, {"depth": 2},
           {"resample_kernel_size": 6}, {"resample_stride": 4}, {"num_inputs": 1})
CASE = S.NetCase("Waveunet", O, "waveunet.npz", 2048, rounding=True, emulated_bar16=True, state_dict_count=314,
                 refusal_match=True, bad_lengths=(2056, 1024, 16380), rejects_empty_batch=True, spec_hop=2048,
                 cli_config="config_waveunet.json", cli_chunk=2048, cli_lengths=(4500, 700), cli_num_samples=("%", 2048))
_gate, _bar16, _clamped = S.gate, S.bar16, S.clamped


def _params():
    return S.params(CASE)


def _net(dtype="float32"):
    return S.net(CASE, dtype=dtype)


def _oracle_case(B, N):
    return S.oracle_case(CASE, B, N)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
def test_forward_matches_reference(torch_cuda, dtype):
    """float32 is the test that sees a wrong deep layer: replacing any one deep tensor moves the
    reference's output by at least 2.5e-2 relative rms."""
    S.check_forward_matches_reference(CASE, dtype)


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
    S.check_forward_16bit_at_the_config_length(CASE, dtype)


@pytest.mark.parametrize("nc,mode", S.SAMPLING_CASES)
def test_sampling_matches_reference(torch_cuda, nc, mode):
    S.check_sampling_matches_reference(CASE, nc, mode)


def test_continuous_sampling_single_clip(torch_cuda):
    S.check_continuous_sampling_single_clip(CASE)


def test_row_sharding_is_bit_identical(torch_cuda):
    S.check_row_sharding(CASE)


@pytest.mark.parametrize("N", [pytest.param(N, id=f"{N}-default") for N in (2048, 6144)])
def test_rows_are_independent_of_the_batch(torch_cuda, N):
    """Row b of a B = 5 forward equals the same clip run alone, bit for bit (bfloat16)."""
    net = _net("bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in S.inputs(5, N, seed=2))
    full = net(cond, x_t, nl)
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    for b in range(5):
        one = net(cond[b:b + 1].contiguous(), x_t[b:b + 1].contiguous(), nl[b:b + 1].contiguous())
        assert torch.equal(full[b:b + 1], one), b


def test_rejects_bad_geometry(torch_cuda):
    S.check_rejects_bad_geometry(CASE)


def test_spectrogram_arch_is_not_implemented(torch_cuda):
    S.check_spectrogram_arch_is_not_implemented(CASE)


@pytest.mark.parametrize("change", REFUSED)
def test_unsupported_arguments_are_refused_at_configure(torch_cuda, change):
    S.check_refused_at_configure(CASE, S.config(CASE, **change), next(iter(change)))


def test_missing_params_counts_the_state_dict(torch_cuda):
    S.check_missing_params(CASE)


def test_sddm_forward_matches_oracle(torch_cuda):
    S.check_sddm_forward_matches_oracle(CASE)


def test_infer_cli_end_to_end(torch_cuda, tmp_path):
    S.check_infer_cli_end_to_end(CASE, tmp_path)
