"""Child process of tests/test_gpu_diffwave_paths.py (not a test module).

    python _dw_paths_child.py OUT.npz [extras]

The DiffWave launch knobs (SDDM_DW_NOPP / NOCHAIN / CHSEG / NOFUSE) are read once per process by
the library, so each knob set is one fresh interpreter with the knob in its environment.  It runs the
facade DiffWave (30 layers, cycle 10, 513 bins, the test weights) on every case and writes one npz:

  fw/<dtype>/<B>x<F>      eps of one forward, (B, F) in FW_CASES, bf16 and fp16
  many/<kind>             bf16 forward at F = 63 with B = many_batch(kind, CU count): batches at which
                          a block of dw_layer_chain_kernel takes a second segment
  sample/<dtype>          SDDM_spectrogram.infer, SAMPLE_SCHED, time_step, seed 7, spec (2, 513, 63)
  ncu                     multi_processor_count of the device

extras: comma-separated 'many32' / 'many8' (which fw_many batches to run) and 'f32' (also the fp32
sample, the figure the 16-bit drift is printed against).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FW_CASES = ((3, 1), (3, 2), (3, 5), (2, 63))
DTYPES = ("bfloat16", "float16")
SAMPLE_SCHED = ("linear", 200, 1e-4, 0.02)
SAMPLE_SHAPE = (2, 63)
F_MANY = 63


def dw_rows(B, F, seed):
    """The inputs of test_gpu_diffwave.py::_dw_rows."""
    rng = np.random.default_rng(seed)
    spec = rng.uniform(0, 1, (B, 513, F)).astype(np.float32)
    audio = rng.standard_normal((B, 1, 256 * F)).astype(np.float32)
    steps = rng.integers(1, 201, B).astype(np.float32)
    return spec, audio, steps


def fw_seed(B, F):
    return 100 + 10 * B + F


def many_batch(kind, ncu):
    """many32: 4 segments per clip at 32 (and 8 at 16) tiles per segment; many8: 16 per clip."""
    return {"many32": ncu // 4 + 8, "many8": ncu // 16 + 4}[kind]


def many_seed(kind):
    return {"many32": 61, "many8": 62}[kind]


def _paths():
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "speech-denoising-diffusion-model-2_amd"))


def main(out_path, extras):
    _paths()
    import torch
    import model.diffusion as D
    import model.model as M
    import model.network as NW
    from _helpers import diffwave_params

    params = {k: torch.from_numpy(v) for k, v in diffwave_params().items()}

    def net(dtype):
        n = NW.DiffWave(num_samples=-1, num_timesteps=3, freq_bins=513, residual_channels=64, residual_layers=30,
                        dilation_cycle_length=10)
        n.load_state_dict(params)
        n.compute_dtype = dtype
        return n.cuda()

    def forward(n, rows):
        spec, audio, steps = rows
        return n(torch.from_numpy(spec).cuda(), torch.from_numpy(audio).cuda(),
                 torch.from_numpy(steps).reshape(-1, 1, 1).cuda()).cpu().numpy()

    def sample(dtype):
        d = D.GaussianDiffusion(*SAMPLE_SCHED, device="cuda")
        m = M.SDDM_spectrogram(d, net(dtype), hop_samples=256, noise_condition="time_step", compute_dtype=dtype).cuda()
        spec = dw_rows(*SAMPLE_SHAPE, 63)[0]
        return m.infer(torch.from_numpy(spec).cuda(), seed=7).cpu().numpy()

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    res = {"ncu": np.array(ncu)}
    for dtype in DTYPES:
        n = net(dtype)
        for B, F in FW_CASES:
            res[f"fw/{dtype}/{B}x{F}"] = forward(n, dw_rows(B, F, fw_seed(B, F)))
        if dtype == "bfloat16":
            for kind in ("many32", "many8"):
                if kind in extras:
                    res[f"many/{kind}"] = forward(n, dw_rows(many_batch(kind, ncu), F_MANY, many_seed(kind)))
        del n
        res[f"sample/{dtype}"] = sample(dtype)
    if "f32" in extras:
        res["sample/float32"] = sample("float32")
    torch.cuda.synchronize()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2].split(",") if len(sys.argv) > 2 else [])
