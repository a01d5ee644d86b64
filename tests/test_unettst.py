"""CPU: the UNetTST facade (reference model/UNetTST.py:270-392) -- state-dict layout, the shipped
config against the reference's config_unettst.json, build_from_config, the refusal of host tensors,
and the torch oracle the GPU tests rely on: the whole forward, the Dual_Transformer alone at the five
golden shapes, and SDDM.infer in one mode per noise condition."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from _helpers import GOLDEN, golden, rms, tables_from_golden
from _weights import make_params

DT_SHAPES = ((1, 4), (2, 4), (3, 4), (8, 4), (2, 8))


def _keys():
    with open(os.path.join(GOLDEN, "unettst_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_unettst.json")) as f:
        return json.load(f)


def test_facade_state_dict_matches_reference():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    net = NW.UNetTST(num_samples=16448, **args)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 454 and got == _keys()
    assert sum(v.numel() for v in net.state_dict().values()) == 8201395
    assert sum(v.numel() for k, v in net.state_dict().items() if k.startswith("mid.")) == 3438642
    assert net.library_config()["network"] == {"type": "UNetTST", "args": args}
    assert net.library_config()["num_samples"] == 16448
    assert isinstance(net.mid, NW.Dual_Transformer)
    alone = NW.Dual_Transformer(160, 160, 0, 6)
    assert [["mid." + k, list(v.shape)] for k, v in alone.state_dict().items()] == [e for e in _keys() if e[0].startswith("mid.")]


def test_shipped_config_is_the_reference_config_plus_infer_dataset():
    import infer
    with open(os.path.join(os.path.dirname(infer.__file__), "configs", "config_unettst.json")) as f:
        cfg = json.load(f)
    ref = _reference_config()
    for k in ("num_samples", "sample_rate", "arch", "diffusion", "network"):
        assert cfg[k] == ref[k], k
    assert cfg["infer_dataset"]["type"] == "InferDataset"


def test_shipped_config_builds(tmp_path):
    from parse_config import ConfigParser, read_json
    import infer
    import model.diffusion as module_diffusion
    import model.model as module_arch
    import model.network as module_network
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_unettst.json"))
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    _, network, model = module_arch.build_from_config(config, module_diffusion, module_network, module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "UNetTST"
    assert model.num_timesteps == 1000 and len(model.state_dict()) == 454 + 14
    lib = model.library_config()
    assert lib["network"] == {"type": "UNetTST", "args": cfg["network"]["args"]} and lib["num_samples"] == 16448
    assert lib["arch"]["args"]["p_transition"] == "original"


def test_facade_refuses_what_the_reference_refuses_and_host_tensors():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    with pytest.raises(AssertionError):
        NW.UNetTST(num_samples=2100, **args)                    # (2100 - 128) % 64 != 0 (UNetTST.py:13)
    net = NW.UNetTST(num_samples=2112, **args)
    z = torch.zeros(1, 1, 2112)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))
    with pytest.raises(RuntimeError):
        net.mid(torch.zeros(1, 160, 1, 4))
    with pytest.raises(NotImplementedError, match="input_size"):
        NW.Dual_Transformer(128, 128, 0, 1).library_config()
    from model.UNetTST import TransformerEncoderLayer
    for change in ({"bidirectional": False}, {"activation": "gelu"}):
        with pytest.raises(NotImplementedError):
            TransformerEncoderLayer(80, 4, **change)


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    import _unettst_oracle as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    assert O.ARGS == _reference_config()["network"]["args"]
    z = golden("unettst.npz")
    ref = z["fw/eps"]
    P = make_params(shapes, 0)
    eps = O.forward(P, z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"UNetTST: oracle vs reference rms {err:.3e} (reference rms {rms(ref, 0):.3f})")
    assert err <= 1e-5
    one = O.forward(P, z["fw/cond"][:1], z["fw/x_t"][:1], z["fw/noise_level"][:1])   # B = 1
    assert rms(one, ref[:1]) <= 1e-5


@pytest.mark.parametrize("dim2,dim1", DT_SHAPES)
def test_oracle_matches_reference_dual_transformer(dim2, dim1):
    import _unettst_oracle as O
    z = golden("unettst.npz")
    x, ref = z[f"dt/{dim2}x{dim1}/x"], z[f"dt/{dim2}x{dim1}/y"]
    P = make_params(O.param_shapes(), 0)
    y = O.dual_transformer(P, x)
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x{dim1}: oracle vs reference relative rms {rel:.3e}")
    assert y.shape == ref.shape and rel <= 2e-6
    # the wiring the GPU test has to see: swapping the r / z gates of one late column GRU
    Q = dict(P)
    w = Q["mid.col_trans.5.gru.weight_hh_l0"].copy()
    w[:160], w[160:320] = P["mid.col_trans.5.gru.weight_hh_l0"][160:320], P["mid.col_trans.5.gru.weight_hh_l0"][:160]
    Q["mid.col_trans.5.gru.weight_hh_l0"] = w
    moved = rms(O.dual_transformer(Q, x), ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x{dim1}: r / z of col_trans.5's weight_hh swapped moves the output by {moved:.3e}")
    assert moved >= (1e-4 if dim2 >= 2 else 0.0)


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", "sr3"), ("time_step", "original")])
def test_oracle_sampling_matches_reference(nc, mode):
    import _unettst_oracle as O
    from oracle import sampler
    z = golden("unettst.npz")
    P = make_params(O.param_shapes(), 0)
    rec = []
    out = sampler.infer(lambda c, x, nl: O.forward(P, c, x, nl), tables_from_golden("linear_3_0.0001_0.05"),
                        z["inf/cond"], mode=mode, noise_condition=nc, seed=7, record=rec)
    steps = z[f"inf/{nc}/{mode}/steps"]
    errs = [rms(a, b) for a, b in zip(rec[1:], steps)]
    print(f"UNetTST {nc} {mode}: oracle sampler vs reference, x_t per step {['%.2e' % e for e in errs]}")
    assert rms(out, steps[-1]) <= 1e-5 and max(errs) <= 1e-5


def test_emulation_rounds_the_transformer():
    """The 16-bit emulation moves the block's output by about the rounding of its weights."""
    import _unettst_oracle as O
    z = golden("unettst.npz")
    x, ref = z["dt/2x4/x"], z["dt/2x4/y"]
    P = make_params(O.param_shapes(), 0)
    for dtype, lo, hi in ((torch.bfloat16, 1e-3, 3e-2), (torch.float16, 1e-4, 5e-3)):
        rel = rms(O.dual_transformer(P, x, rounding=dtype), ref) / rms(ref, 0)
        print(f"Dual_Transformer 2x4 {dtype}: emulation vs reference relative rms {rel:.3e}")
        assert lo <= rel <= hi
