"""CPU: the Waveunet2 facade (reference model/waveunet2.py:226-324) -- state-dict layout, the
reference's config_waveunet2.json through build_from_config, the constructor's asserts, the torch
oracle the GPU tests rely on (one forward and SDDM.infer in every mode), and infer.py's chunk-length
check."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from _helpers import GOLDEN, golden, rms, tables_from_golden
from _weights import make_params

MODES = ("original", "condition_in", "sr3", "supportive", "conditional")


def _keys():
    with open(os.path.join(GOLDEN, "waveunet2_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_waveunet2.json")) as f:
        return json.load(f)


def test_facade_state_dict_matches_reference():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    net = NW.Waveunet2(**args, num_samples=16384)       # init_obj's keyword is accepted and ignored
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 90 and got == _keys()
    assert sum(v.numel() for v in net.state_dict().values()) == 449473
    assert net.config_args == args and NW.Waveunet2.hop_samples == 8
    assert net.library_config()["network"] == {"type": "Waveunet2", "args": args}


def test_reference_config_builds(tmp_path):
    """config_waveunet2.json unchanged: no arch args, no infer_dataset."""
    from parse_config import ConfigParser
    import model.diffusion as module_diffusion
    import model.model as module_arch
    import model.network as module_network
    cfg = copy.deepcopy(_reference_config())
    assert cfg["num_samples"] == 16384 and cfg["arch"]["args"] == {} and "infer_dataset" not in cfg
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    diffusion, network, model = module_arch.build_from_config(config, module_diffusion, module_network,
                                                              module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "Waveunet2"
    assert model.noise_estimate_model is network and model.num_timesteps == 1000
    lib = model.library_config()
    assert lib["arch"]["type"] == "SDDM" and lib["arch"]["args"]["p_transition"] == "original"
    assert lib["network"] == {"type": "Waveunet2", "args": cfg["network"]["args"]}
    assert lib["diffusion"]["args"]["n_timestep"] == 1000


def test_shipped_config_is_the_reference_config_plus_infer_dataset():
    import infer
    with open(os.path.join(os.path.dirname(infer.__file__), "configs", "config_waveunet2.json")) as f:
        cfg = json.load(f)
    ref = _reference_config()
    for k in ("num_samples", "sample_rate", "arch", "diffusion", "network"):
        assert cfg[k] == ref[k], k
    assert cfg["infer_dataset"]["type"] == "InferDataset"


def test_constructor_asserts():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    for change in ({"downconv_kernel_size": 4}, {"upconv_kernel_size": 4},      # only odd filter kernels
                   {"downsample_kernel_size": 5}, {"upsample_kernel_size": 3},  # parity of the resample kernels
                   {"num_channels": [24, 48, 76, 96]}):                         # GroupNorm groups of 8
        with pytest.raises(AssertionError):
            NW.Waveunet2(**dict(args, **change))
    NW.Waveunet2(**{k: v for k, v in args.items() if k not in ("depth", "downsample_kernel_size",
                                                               "upsample_kernel_size", "resample_stride")})


def test_facade_needs_the_hip_device():
    import model.network as NW
    net = NW.Waveunet2(**_reference_config()["network"]["args"])
    z = torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    from _waveunet_film_oracle import WAVEUNET2 as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    assert O.ARGS == _reference_config()["network"]["args"]
    z = golden("waveunet2.npz")
    ref = z["fw/eps"]
    eps = O.forward(make_params(shapes, 0), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"Waveunet2: oracle vs reference rms {err:.3e} (reference rms {rms(ref, 0):.3f})")
    assert err <= 1e-5
    one = O.forward(make_params(shapes, 0), z["fw/cond"][:1], z["fw/x_t"][:1], z["fw/noise_level"][:1])   # B = 1
    assert rms(one, ref[:1]) <= 1e-5


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")])
def test_oracle_sampling_matches_reference(nc, mode):
    """The oracle looped by the oracle sampler against the reference's unmodified SDDM.infer: the
    output and every intermediate x_t."""
    from _waveunet_film_oracle import WAVEUNET2 as O
    from oracle import sampler
    z = golden("waveunet2.npz")
    P = make_params(O.param_shapes(), 0)
    k = f"inf/{nc}/{mode}"
    rec = []
    out = sampler.infer(lambda c, x, nl: O.forward(P, c, x, nl), tables_from_golden("linear_3_0.0001_0.05"),
                        z["inf/cond"], mode=mode, noise_condition=nc, seed=7, record=rec)
    errs = [rms(a, b) for a, b in zip(rec[1:], z[k + "/steps"])]
    print(f"Waveunet2 {nc} {mode}: oracle sampler vs reference, output {rms(out, z[k + '/out']):.3e}, "
          f"x_t per step {['%.2e' % e for e in errs]}")
    assert rms(out, z[k + "/out"]) <= 1e-5
    assert rms(np.stack(rec[1:]), z[k + "/steps"]) <= 1e-5


def test_infer_rejects_chunks_off_the_multiple_of_8(tmp_path):
    """16380 is no multiple of 8: infer.py fails before it touches the data (the data_root does not
    exist) and names the multiple; 16384 passes the check."""
    from parse_config import ConfigParser
    import infer
    cfg = copy.deepcopy(_reference_config())
    cfg.update({"num_samples": 16380,
                "infer_dataset": {"type": "InferDataset", "args": {"data_root": str(tmp_path / "absent"),
                                                                    "datatype": ".wav"}}})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    with pytest.raises(ValueError, match=r"multiple of its hop \(8 samples\)"):
        infer.main(ConfigParser(cfg, run_id="x"))
    cfg["num_samples"] = 16384
    infer.check_num_samples(ConfigParser(cfg, run_id="y"))
    for bad in (0, -8, 4, None):
        cfg["num_samples"] = bad
        with pytest.raises(ValueError):
            infer.check_num_samples(cfg)
