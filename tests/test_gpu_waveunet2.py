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
import pytest
import torch

import _net_suite as S
from _waveunet_film_oracle import WAVEUNET2 as O
from _helpers import rms

pytestmark = pytest.mark.gpu

REFUSED = ({"num_channels": [32, 64, 96, 128]}, {"depth": 2}, {"conv_type": "bn"},
              {"downconv_kernel_size": 3}, {"resample_stride": 4}, {"num_inputs": 1})
CASE = S.NetCase("Waveunet2", O, "waveunet2.npz", 296, rounding=True, state_dict_count=90, bad_lengths=(300, 4), spec_hop=8,
                 cli_config="config_waveunet2.json", cli_chunk=1024, cli_lengths=(2500, 700), cli_num_samples=("%", 8))


@pytest.mark.parametrize("dtype,tol", [("float32", 1e-4), ("bfloat16", 3e-2), ("float16", 5e-3)])
def test_forward_matches_reference(torch_cuda, dtype, tol):
    S.check_forward_matches_reference(CASE, dtype, tol)


@pytest.mark.parametrize("case", ["bottom1", "tiles", "single"])
def test_forward_matches_oracle(torch_cuda, case):
    """bottom1: B=3, N=8 -- every length is <= 8, the bottleneck is one position, the transposed conv
    starts from one position and a GroupNorm group is 8 values.  tiles: B=2, N=2072 (2072 / 1036 / 518 / 259) -- partial tiles
    everywhere and more than one 128-position tile at every level; level passed as [B].  single: one
    clip, level passed as [B, 1, 1]."""
    B, N = {"bottom1": (3, 8), "tiles": (2, 2072), "single": (1, 296)}[case]
    cond, x_t, nl = S.inputs(B, N, seed=31)
    ref = S.oracle_forward(CASE, cond, x_t, nl)
    assert S.clamped(ref) <= 0.25
    level = torch.from_numpy(nl).cuda()
    eps = S.net(CASE)(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(),
                      level if case == "tiles" else level.reshape(B, 1, 1))
    assert tuple(eps.shape) == (B, 1, N)
    err = rms(eps.cpu().numpy(), ref)
    print(f"Waveunet2 {case} B={B} N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f}, clamped {S.clamped(ref):.3f})")
    assert err <= 1e-4 * S.gate(ref)


@pytest.mark.parametrize("dtype,tol", [("bfloat16", 3e-2), ("float16", 5e-3)])
def test_forward_16bit_at_the_config_length(torch_cuda, dtype, tol):
    S.check_forward_16bit_at_the_config_length(CASE, dtype, tol)


@pytest.mark.parametrize("nc,mode", S.SAMPLING_CASES)
def test_sampling_matches_reference(torch_cuda, nc, mode):
    S.check_sampling_matches_reference(CASE, nc, mode)


def test_continuous_sampling_single_clip(torch_cuda):
    S.check_continuous_sampling_single_clip(CASE)


def test_row_sharding_is_bit_identical(torch_cuda):
    S.check_row_sharding(CASE)


def test_rows_are_independent_of_the_batch(torch_cuda):
    S.check_rows_in_two_parts(CASE)


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
