"""CPU: the DenoiseWaveGrad1 / DenoiseWaveGrad3 facade (reference model/wavegrad.py:184-242, 307-353)
-- state-dict layout, the reference's default config.json through build_from_config, the registry,
the numpy oracle the GPU tests rely on, and infer.py's chunk-length check."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from _helpers import GOLDEN, golden, rms
from _weights import make_params

NETS = ("DenoiseWaveGrad1", "DenoiseWaveGrad3")


def _keys():
    with open(os.path.join(GOLDEN, "denoise_wavegrad_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_denoise_wavegrad1.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", NETS)
def test_facade_state_dict_matches_reference(name):
    import model.network as NW
    net = getattr(NW, name)(num_samples=32000)          # init_obj's keyword is accepted and ignored
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert got == _keys()[name]
    assert net.hop_samples == {"DenoiseWaveGrad1": 400, "DenoiseWaveGrad3": 300}[name]
    assert net.config_args == {}


def test_reference_default_config_builds(tmp_path):
    """The settings of the reference's config.json: no num_samples, no arch args, no infer_dataset."""
    from parse_config import ConfigParser
    import model.diffusion as module_diffusion
    import model.model as module_arch
    import model.network as module_network
    cfg = copy.deepcopy(_reference_config())
    assert "num_samples" not in cfg and cfg["arch"]["args"] == {} and "infer_dataset" not in cfg
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    diffusion, network, model = module_arch.build_from_config(config, module_diffusion, module_network,
                                                              module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "DenoiseWaveGrad1"
    assert model.noise_estimate_model is network and model.num_timesteps == 2000
    lib = model.library_config()
    assert lib["arch"]["type"] == "SDDM" and lib["network"] == {"type": "DenoiseWaveGrad1", "args": {}}
    assert lib["arch"]["args"]["p_transition"] == "original"
    assert lib["diffusion"]["args"]["n_timestep"] == 2000


def test_denoise_wavegrad2_is_not_registered():
    import model.network as NW
    assert hasattr(NW, "DenoiseWaveGrad1") and hasattr(NW, "DenoiseWaveGrad3")
    assert not hasattr(NW, "DenoiseWaveGrad2")


@pytest.mark.parametrize("name", NETS)
def test_oracle_matches_reference_forward(name):
    """Pins the numpy restatement that the larger GPU cases are checked against."""
    import _denoise_wavegrad_oracle as O
    shapes = O.param_shapes(name)
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys()[name])
    P = make_params(shapes, 0)
    z = golden("denoise_wavegrad.npz")
    ref = z[f"{name}/fw/eps"]
    eps = O.forward(name, P, z[f"{name}/fw/cond"], z[f"{name}/fw/x_t"], z[f"{name}/fw/noise_level"])
    assert eps.shape == ref.shape
    rel = rms(eps, ref) / rms(ref, 0)
    print(f"{name}: oracle vs reference relative rms {rel:.3e}")
    assert rel <= 1e-5


def test_infer_rejects_chunks_off_the_hop(tmp_path):
    """16448 (the UNet configs' chunk) is no multiple of DenoiseWaveGrad1's 400: infer.py fails before
    it touches the data (the data_root does not exist) and names the hop."""
    from parse_config import ConfigParser
    import infer
    cfg = copy.deepcopy(_reference_config())
    cfg.update({"num_samples": 16448,
                "infer_dataset": {"type": "InferDataset", "args": {"data_root": str(tmp_path / "absent"),
                                                                    "datatype": ".wav"}}})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    with pytest.raises(ValueError, match="400"):
        infer.main(ConfigParser(cfg, run_id="x"))
    cfg["num_samples"] = 16400
    infer.check_num_samples(ConfigParser(cfg, run_id="y"))
    for bad in (0, -400, 200, None):
        cfg["num_samples"] = bad
        with pytest.raises(ValueError):
            infer.check_num_samples(cfg)
