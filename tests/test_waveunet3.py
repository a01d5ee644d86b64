"""CPU: the Waveunet3 facade (reference model/waveunet3.py:314-416) -- state-dict layout, the
reference's config_waveunet3.json through build_from_config, the constructor's refusals, the torch
oracle the GPU tests rely on, and infer.py's chunk-length check."""
import copy
import json
import os

import pytest
import torch

from _helpers import GOLDEN, golden, rms
from _weights import make_params


def _keys():
    with open(os.path.join(GOLDEN, "waveunet3_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_waveunet3.json")) as f:
        return json.load(f)


def test_facade_state_dict_matches_reference():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    net = NW.Waveunet3(**args, num_samples=16384)       # init_obj's keyword is accepted and ignored
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 180 and got == _keys()
    assert net.config_args == args
    assert net.library_config()["network"] == {"type": "Waveunet3", "args": args}


def test_reference_config_builds(tmp_path):
    """config_waveunet3.json unchanged: no arch args, no infer_dataset."""
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
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "Waveunet3"
    assert model.noise_estimate_model is network and model.num_timesteps == 1000
    lib = model.library_config()
    assert lib["arch"]["type"] == "SDDM" and lib["arch"]["args"]["p_transition"] == "original"
    assert lib["network"] == {"type": "Waveunet3", "args": cfg["network"]["args"]}
    assert lib["diffusion"]["args"]["n_timestep"] == 1000


def test_shipped_config_is_the_reference_config_plus_infer_dataset():
    import infer
    with open(os.path.join(os.path.dirname(infer.__file__), "configs", "config_waveunet3.json")) as f:
        cfg = json.load(f)
    ref = _reference_config()
    for k in ("num_samples", "sample_rate", "arch", "diffusion", "network"):
        assert cfg[k] == ref[k], k
    assert cfg["infer_dataset"]["type"] == "InferDataset"


def test_unsupported_arguments_raise():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    with pytest.raises(NotImplementedError):
        NW.Waveunet3(**dict(args, with_attn=True))
    with pytest.raises(NotImplementedError):
        NW.Waveunet3(**dict(args, with_noise_level_emb=True))
    with pytest.raises(NotImplementedError):
        NW.Waveunet3(**{k: v for k, v in args.items() if k != "with_attn"})   # the reference's default is True
    with pytest.raises(AssertionError):
        NW.Waveunet3(**dict(args, norm_groups=16))                            # num_channels[0] == norm_groups
    with pytest.raises(AssertionError):
        NW.Waveunet3(**dict(args, downsample_kernel_size=5))                  # parity of the resample kernels
    with pytest.raises(AssertionError):
        NW.Waveunet3(**dict(args, upsample_kernel_size=3))


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    import _waveunet3_oracle as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    assert O.ARGS == _reference_config()["network"]["args"]
    z = golden("waveunet3.npz")
    ref = z["fw/eps"]
    eps = O.forward(make_params(shapes, 0), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape
    rel = rms(eps, ref) / rms(ref, 0)
    print(f"Waveunet3: oracle vs reference relative rms {rel:.3e}")
    assert rel <= 1e-5


def test_infer_rejects_chunks_off_the_multiple_of_8(tmp_path):
    """16388 is no multiple of 8: infer.py fails before it touches the data (the data_root does not
    exist) and names the multiple; 16384 passes the check."""
    from parse_config import ConfigParser
    import infer
    cfg = copy.deepcopy(_reference_config())
    cfg.update({"num_samples": 16388,
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


def test_facade_needs_the_hip_device():
    import model.network as NW
    net = NW.Waveunet3(**_reference_config()["network"]["args"])
    z = torch.zeros(1, 1, 8)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))
