"""CPU: the CAUNet facade (reference model/CAUNet.py:307-374) -- state-dict layout, the shipped config
against the reference's config_caunet.json, build_from_config, the refusals, and the torch oracle the
GPU tests rely on: the whole forward (use_affine_level false and true, B = 2 and B = 1), the
Dual_Transformer alone at the six golden shapes, and SDDM.infer in one mode per noise condition."""
import json
import os

import numpy as np
import pytest
import torch

from _helpers import GOLDEN, golden, rms, tables_from_golden
from _weights import make_params

DT_DIM2 = (1, 2, 3, 10, 17, 70)


def _keys():
    with open(os.path.join(GOLDEN, "caunet_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_caunet.json")) as f:
        return json.load(f)


def test_facade_state_dict_matches_reference():
    import model.network as NW
    import model.CAUNet as C
    args = _reference_config()["network"]["args"]
    net = NW.CAUNet(num_samples=16448, **args)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 450 and got == _keys()
    assert sum(v.numel() for v in net.state_dict().values()) == 2258049
    assert sum(v.numel() for k, v in net.state_dict().items() if k.startswith("mid.")) == 558400
    assert net.library_config()["network"] == {"type": "CAUNet", "args": args}
    assert net.library_config()["num_samples"] == 16448
    assert isinstance(net.mid, C.Dual_Transformer)
    alone = C.Dual_Transformer(64, 64, 0, 6)
    assert [["mid." + k, list(v.shape)] for k, v in alone.state_dict().items()] == [e for e in _keys() if e[0].startswith("mid.")]
    affine = NW.CAUNet(num_samples=704, **dict(args, use_affine_level=True))
    assert tuple(affine.downs[0].noise_func.noise_func[2].weight.shape) == (128, 256)


def test_shipped_config_is_the_reference_config_plus_infer_dataset():
    import infer
    with open(os.path.join(os.path.dirname(infer.__file__), "configs", "config_caunet.json")) as f:
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
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_caunet.json"))
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    _, network, model = module_arch.build_from_config(config, module_diffusion, module_network, module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "CAUNet"
    assert model.num_timesteps == 1000 and len(model.state_dict()) == 450 + 14
    lib = model.library_config()
    assert lib["network"] == {"type": "CAUNet", "args": cfg["network"]["args"]} and lib["num_samples"] == 16448
    assert lib["arch"]["args"]["p_transition"] == "original"


def test_facade_refuses_what_the_reference_refuses_and_host_tensors():
    import model.network as NW
    import model.CAUNet as C
    args = _reference_config()["network"]["args"]
    with pytest.raises(AssertionError):
        NW.CAUNet(num_samples=700, **args)                      # (700 - 128) % 64 != 0 (CAUNet.py:13)
    net = NW.CAUNet(num_samples=704, **args)
    z = torch.zeros(1, 1, 704)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))
    with pytest.raises(RuntimeError):
        net.mid(torch.zeros(1, 64, 1, 8))
    with pytest.raises(NotImplementedError, match="input_size"):
        C.Dual_Transformer(128, 128, 0, 1).library_config()


@pytest.mark.parametrize("name,value", [("inner_channel", 32), ("n_encode_layers", 3), ("dense_depth", 4), ("segment_len", 256),
                                        ("segment_stride", 32), ("n_TSTB", 0), ("use_affine_level", 2)])
def test_arguments_outside_the_accepted_set_are_refused_by_name(name, value):
    import model.network as NW
    args = dict(_reference_config()["network"]["args"], **{name: value})
    with pytest.raises(NotImplementedError, match=name):
        NW.CAUNet(num_samples=704, **args)


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    import _caunet_oracle as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    assert O.ARGS == _reference_config()["network"]["args"]
    z = golden("caunet.npz")
    for tag, args in (("fw", O.ARGS), ("fwa", dict(O.ARGS, use_affine_level=True))):
        ref = z[tag + "/eps"]
        P = make_params(O.param_shapes(args), 0)
        eps = O.forward(P, z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], args=args)
        assert eps.shape == ref.shape
        err = rms(eps, ref)
        print(f"CAUNet {tag}: oracle vs reference rms {err:.3e} (reference rms {rms(ref, 0):.3f})")
        assert err <= 1e-5
        one = O.forward(P, z["fw/cond"][:1], z["fw/x_t"][:1], z["fw/noise_level"][:1], args=args)   # B = 1
        assert rms(one, ref[:1]) <= 1e-5


@pytest.mark.parametrize("dim2", DT_DIM2)
def test_oracle_matches_reference_dual_transformer(dim2):
    import _caunet_oracle as O
    z = golden("caunet.npz")
    x, ref = z[f"dt/{dim2}x8/x"], z[f"dt/{dim2}x8/y"]
    P = make_params(O.param_shapes(), 0)
    y = O.dual_transformer(P, x)
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x8: oracle vs reference relative rms {rel:.3e}")
    assert y.shape == ref.shape and rel <= 2e-6
    # the wiring the GPU test has to see: swapping the r / z gates of one late column GRU
    Q = dict(P)
    w0 = P["mid.col_trans.5.gru.weight_hh_l0"]
    w = w0.copy()
    w[:64], w[64:128] = w0[64:128], w0[:64]
    Q["mid.col_trans.5.gru.weight_hh_l0"] = w
    moved = rms(O.dual_transformer(Q, x), y) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x8: r / z of col_trans.5's weight_hh swapped moves the output by {moved:.3e}")
    if dim2 >= 2:
        assert moved >= 1e-4
    else:
        assert moved == 0.0                                      # one frame: h0 = 0, weight_hh never matters


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", "sr3"), ("time_step", "original")])
def test_oracle_sampling_matches_reference(nc, mode):
    import _caunet_oracle as O
    from oracle import sampler
    z = golden("caunet.npz")
    P = make_params(O.param_shapes(), 0)
    rec = []
    out = sampler.infer(lambda c, x, nl: O.forward(P, c, x, nl), tables_from_golden("linear_3_0.0001_0.05"),
                        z["inf/cond"], mode=mode, noise_condition=nc, seed=7, record=rec)
    steps = z[f"inf/{nc}/{mode}/steps"]
    errs = [rms(a, b) for a, b in zip(rec[1:], steps)]
    print(f"CAUNet {nc} {mode}: oracle sampler vs reference, x_t per step {['%.2e' % e for e in errs]}")
    assert rms(out, steps[-1]) <= 1e-5 and max(errs) <= 1e-5


def test_emulation_rounds_the_transformer():
    """The 16-bit emulation moves the block's output by about the rounding of its operands.  Measured
    on the CPU at (2, 8): bfloat16 3.73e-3, float16 4.59e-4 relative rms; the brackets are a third
    and three times those, rounded."""
    import _caunet_oracle as O
    z = golden("caunet.npz")
    x, ref = z["dt/2x8/x"], z["dt/2x8/y"]
    P = make_params(O.param_shapes(), 0)
    for dtype, lo, hi in ((torch.bfloat16, 1.2e-3, 1.1e-2), (torch.float16, 1.5e-4, 1.4e-3)):
        rel = rms(O.dual_transformer(P, x, rounding=dtype), ref) / rms(ref, 0)
        print(f"Dual_Transformer 2x8 {dtype}: emulation vs reference relative rms {rel:.3e}")
        assert lo <= rel <= hi
