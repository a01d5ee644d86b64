"""CPU: the TSTNN facade (reference model/tstnn.py:216-299) -- state-dict layout, the shipped config
against the reference's config_tstnn.json, build_from_config, the refusals, and the torch oracle the
GPU tests rely on: the whole forward (B = 2 and B = 1), the Dual_Transformer alone at the four golden
shapes, SDDM.infer in one mode per noise condition, the three wirings the GPU bars have to see, and
that the test weights leave neither the mask nor eps degenerate."""
import json
import os

import numpy as np
import pytest
import torch

import _net_suite as S
from _helpers import GOLDEN, golden, rms, tables_from_golden
from _weights import make_params

DT_SHAPES = ((1, 16), (2, 33), (5, 40), (3, 256))
# the float32 bars of test_gpu_tstnn.py: the whole forward (rms, times max(1, rms of the reference)) and the
# block alone (relative rms)
FW_BAR, BLOCK_BAR = 3.5e-5, 2e-5


def _keys():
    with open(os.path.join(GOLDEN, "tstnn_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_tstnn.json")) as f:
        return json.load(f)


def _params():
    import _tstnn_oracle as O
    return make_params(O.param_shapes(), 0)


def test_facade_state_dict_matches_reference():
    import model.network as NW
    import model.tstnn as T
    args = _reference_config()["network"]["args"]
    net = NW.TSTNN(num_samples=16384, **args)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 229 and got == _keys()
    assert sum(v.numel() for v in net.state_dict().values()) == 924835
    assert sum(v.numel() for k, v in net.state_dict().items() if k.startswith("dual_transformer.")) == 373602
    assert net.library_config()["network"] == {"type": "TSTNN", "args": args}
    assert net.library_config()["num_samples"] == 16384
    assert isinstance(net.dual_transformer, T.Dual_Transformer)
    alone = T.Dual_Transformer(64, 64, num_layers=4)
    assert [["dual_transformer." + k, list(v.shape)] for k, v in alone.state_dict().items()] == \
        [e for e in _keys() if e[0].startswith("dual_transformer.")]
    assert sorted(alone.library_params()) == sorted(e[0] for e in _keys() if e[0].startswith("dual_transformer."))
    assert NW.TSTNN(16384).library_config() == net.library_config()          # the constructor's defaults are the config's


def test_shipped_config_is_the_reference_config_plus_infer_dataset():
    import infer
    with open(os.path.join(os.path.dirname(infer.__file__), "configs", "config_tstnn.json")) as f:
        cfg = json.load(f)
    ref = _reference_config()
    for k in ("num_samples", "sample_rate", "arch", "diffusion", "network"):
        assert cfg[k] == ref[k], k
    assert cfg["infer_dataset"]["type"] == "InferDataset"
    assert cfg["infer_data_loader"]["type"] == "InferDataLoader" and "save_dir" in cfg["trainer"]


def test_shipped_config_builds(tmp_path):
    from parse_config import ConfigParser, read_json
    import infer
    import model.diffusion as module_diffusion
    import model.model as module_arch
    import model.network as module_network
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_tstnn.json"))
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    _, network, model = module_arch.build_from_config(config, module_diffusion, module_network, module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "TSTNN"
    assert model.num_timesteps == 1000 and len(model.state_dict()) == 229 + 14
    lib = model.library_config()
    assert lib["network"] == {"type": "TSTNN", "args": cfg["network"]["args"]} and lib["num_samples"] == 16384
    assert lib["arch"]["args"]["p_transition"] == "original"


def test_facade_refuses_what_the_reference_refuses_and_host_tensors():
    import model.network as NW
    import model.tstnn as T
    with pytest.raises(AssertionError):
        NW.TSTNN(num_samples=700)                                # (700 - 512) % 256 != 0 (tstnn.py:13)
    net = NW.TSTNN(num_samples=768)
    z = torch.zeros(1, 1, 768)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))
    with pytest.raises(RuntimeError):
        net.dual_transformer(torch.zeros(1, 64, 1, 8))
    with pytest.raises(NotImplementedError, match="input_size"):
        T.Dual_Transformer(128, 128, 0, 1).library_config()
    with pytest.raises(NotImplementedError, match="num_layers"):
        T.Dual_Transformer(64, 64, 0, 0).library_config()


@pytest.mark.parametrize("name,value", [("F", 256), ("stride", 128), ("n_channels", 32)])
def test_arguments_outside_the_accepted_set_are_refused_by_name(name, value):
    import model.network as NW
    with pytest.raises(NotImplementedError, match=name):
        NW.TSTNN(num_samples=768, **{name: value})


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    import _tstnn_oracle as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    assert O.ARGS == _reference_config()["network"]["args"]
    z = golden("tstnn.npz")
    ref = z["fw/eps"]
    P = _params()
    eps = O.forward(P, z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"TSTNN fw: oracle vs reference rms {err:.3e} (reference rms {rms(ref, 0):.3f})")
    assert err <= 1e-5
    one = O.forward(P, z["fw/cond"][:1], z["fw/x_t"][:1], z["fw/noise_level"][:1])   # B = 1
    assert rms(one, ref[:1]) <= 1e-5
    assert np.array_equal(O.forward(P, z["fw/cond"], z["fw/x_t"], 1.0 - z["fw/noise_level"]), eps)   # the level is not used


@pytest.mark.parametrize("dim2,dim1", DT_SHAPES)
def test_oracle_matches_reference_dual_transformer(dim2, dim1):
    import _tstnn_oracle as O
    z = golden("tstnn_dt.npz")
    x, ref = z[f"dt/{dim2}x{dim1}/x"], z[f"dt/{dim2}x{dim1}/y"]
    y = O.dual_transformer(_params(), x)
    rel = rms(y, ref) / rms(ref, 0)
    print(f"Dual_Transformer {dim2}x{dim1}: oracle vs reference relative rms {rel:.3e}")
    assert y.shape == ref.shape and rel <= 2e-6


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", "sr3"), ("time_step", "original")])
def test_oracle_sampling_matches_reference(nc, mode):
    import _tstnn_oracle as O
    from oracle import sampler
    z = golden("tstnn.npz")
    P = _params()
    rec = []
    out = sampler.infer(lambda c, x, nl: O.forward(P, c, x, nl), tables_from_golden("linear_3_0.0001_0.05"),
                        z["inf/cond"], mode=mode, noise_condition=nc, seed=7, record=rec)
    steps = z[f"inf/{nc}/{mode}/steps"]
    errs = [rms(a, b) for a, b in zip(rec[1:], steps)]
    print(f"TSTNN {nc} {mode}: oracle sampler vs reference, x_t per step {['%.2e' % e for e in errs]}")
    assert rms(out, steps[-1]) <= 1e-5 and max(errs) <= 1e-5


def test_wirings_move_the_output_ten_bars():
    """Three mistakes a kernel or the packing could make, applied to the oracle at the golden forward
    (B = 2, N = 2816, reference rms 0.892, so the forward's bar is FW_BAR x 1).  Measured on the CPU,
    rms of the change of eps:
      r / z gates of col_trans.3's weight_hh_l0 swapped          3.94e-4
      output1.0 and output2.0 swapped (tanh <-> sigmoid)         8.06e-1
      the block's output PReLU after its conv, not before        2.03e-1
    The first is under ten times the project's 1e-4, so the GPU forward bar is FW_BAR = 3.5e-5, a tenth
    of it rounded down.  On the block alone that swap moves the output by 2.08e-4 (2,33), 3.26e-4 (5,40)
    and 2.81e-4 (3,256) relative, ten times BLOCK_BAR; at dim2 = 1 the column GRU has one step and
    weight_hh never matters."""
    import _tstnn_oracle as O
    z, zd = golden("tstnn.npz"), golden("tstnn_dt.npz")
    P = _params()
    cond, x_t, nl, ref = z["fw/cond"], z["fw/x_t"], z["fw/noise_level"], z["fw/eps"]
    eps = O.forward(P, cond, x_t, nl)
    bar = FW_BAR * S.gate(ref)
    swapped = dict(P)
    w0 = P["dual_transformer.col_trans.3.gru.weight_hh_l0"]
    w = w0.copy()
    w[:64], w[64:128] = w0[64:128], w0[:64]
    swapped["dual_transformer.col_trans.3.gru.weight_hh_l0"] = w
    gates = dict(P)
    for s in ("weight", "bias"):
        gates["output1.0." + s], gates["output2.0." + s] = P["output2.0." + s], P["output1.0." + s]
    moved = {"r / z of col_trans.3 swapped": rms(O.forward(swapped, cond, x_t, nl), eps),
             "output1 / output2 swapped": rms(O.forward(gates, cond, x_t, nl), eps),
             "output PReLU after the conv": rms(O.forward(P, cond, x_t, nl, prelu_after=True), eps)}
    for what, m in moved.items():
        print(f"TSTNN B=2 N=2816: {what} moves eps by {m:.3e} rms (bar {bar:.3e})")
        assert m >= 10 * bar, what
    for dim2, dim1 in DT_SHAPES[1:]:
        x = zd[f"dt/{dim2}x{dim1}/x"]
        y = O.dual_transformer(P, x)
        rel = rms(O.dual_transformer(swapped, x), y) / rms(y, 0)
        after = rms(O.dual_transformer(P, x, prelu_after=True), y) / rms(y, 0)
        print(f"Dual_Transformer {dim2}x{dim1}: r / z swapped moves the output by {rel:.3e}, the PReLU after the conv by {after:.3e} relative")
        assert rel >= 10 * BLOCK_BAR and after >= 10 * BLOCK_BAR


@pytest.mark.parametrize("N", [512, 1280, 2816, 16384])
def test_test_inputs_leave_the_mask_and_eps_alive(N):
    """The GPU parity cannot pass on a zeroed branch: with the seed-0 weights and the harness's inputs
    about half of the mask's ReLU outputs are positive (measured 0.494, 0.506, 0.504, 0.505 at these
    lengths) and eps has rms 0.59, 0.82, 0.90, 0.95."""
    import _tstnn_oracle as O
    cond, x_t, nl = S.inputs(2, N, 31)
    taps = {}
    eps = O.forward(_params(), cond, x_t, nl, taps=taps)
    share = float((taps["mask"] > 0).double().mean())
    print(f"TSTNN B=2 N={N}: positive share of the mask {share:.3f}, eps rms {rms(eps, 0):.3f}, clamp share {S.clamped(eps):.3f}")
    assert 0.3 <= share <= 0.7
    assert 0.4 <= rms(eps, 0) <= 1.2


def test_emulation_rounds_the_transformer():
    """The 16-bit emulation moves the block's output by about the rounding of its operands.  Measured
    on the CPU at (2, 33): bfloat16 3.80e-3, float16 4.80e-4 relative rms; the brackets are a third
    and three times those, rounded.  (The whole forward at B = 2, N = 2816: 1.05e-2 and 1.30e-3.)"""
    import _tstnn_oracle as O
    z = golden("tstnn_dt.npz")
    x, ref = z["dt/2x33/x"], z["dt/2x33/y"]
    for dtype, lo, hi in ((torch.bfloat16, 1.3e-3, 1.1e-2), (torch.float16, 1.6e-4, 1.4e-3)):
        rel = rms(O.dual_transformer(_params(), x, rounding=dtype), ref) / rms(ref, 0)
        print(f"Dual_Transformer 2x33 {dtype}: emulation vs reference relative rms {rel:.3e}")
        assert lo <= rel <= hi
