"""CPU: the UNetModified facade (reference model/UNetModified.py:192-323) -- state-dict layout, the
refusals the reference makes, the refusal of host tensors, the shipped config, the device-free plans
(UNetModified in three dtypes; UNetModified2 at the wide widths float32 could not plan before), and the
torch oracle the GPU tests rely on: the whole forward, the SelfAttention alone at the five golden shapes
and SDDM.infer in one mode per noise condition.

Measured here (oracle in float64 against the reference's float32 on the CPU):
  forward B=2, N=2112                rms 8.9e-7 (reference rms 0.593); without QK_SCALE the output moves by 1.3e-1
  SelfAttention, five shapes         relative rms 1.2e-7 ... 2.4e-7; without 1 / sqrt(C) it moves by 1.4e-1 ... 2.0e-1
  sampling, every x_t                <= 2.1e-7
  golden attention inputs            logit std 3.05 ... 4.00, max |logit| 2.9 ... 12.8, mean row-max probability
                                     0.64 / 0.55 / 0.53 / 0.44 at 16 / 24 / 65 / 128 positions
  16-bit emulation, 256x16x8         bfloat16 3.0e-3, float16 3.6e-4 relative

The issue that asked for this network counts "6" attention steps at res_blocks 1, attn_layer [4]; the
reference module has four there (downs.9, mid.0, ups.0, ups.1: unetmodified_keys.json), so the plan test
asserts one step per attention layer of the reference's key list.
"""
import json
import os

import numpy as np
import pytest
import torch

from _helpers import GOLDEN, golden, rms, tables_from_golden

AT_SHAPES = ((256, 1, 1), (256, 2, 8), (160, 3, 8), (256, 5, 13), (256, 16, 8))


def _keys():
    with open(os.path.join(GOLDEN, "unetmodified_keys.json")) as f:
        return json.load(f)


def _reference_config():
    with open(os.path.join(GOLDEN, "reference_config_unetmodified.json")) as f:
        return json.load(f)


def _attn_params(C):
    """The block's weights under mid.0.attn.*: the network's own at 256 channels, else seed-0 weights of the same names."""
    import _unetmodified_oracle as O
    from _weights import make_params
    return O.make_params() if C == 256 else O.sharpen(make_params(O.attention_shapes(C, "mid.0.attn."), 0))


def _plan_config(network, N, **args):
    base = {"in_channel": 2, "out_channel": 1, "inner_channel": 32, "norm_groups": 32, "res_blocks": 1, "dropout": 0,
            "segment_len": 128, "segment_stride": 64}
    return {"arch": {"type": "SDDM", "args": {}}, "diffusion": {"type": "GaussianDiffusion", "args": {"n_timestep": 3}},
            "network": {"type": network, "args": dict(base, **args)}, "num_samples": N}


def test_facade_state_dict_matches_reference():
    import model.network as NW
    import _unetmodified_oracle as O
    args = _reference_config()["network"]["args"]
    assert args == O.ARGS
    net = NW.UNetModified(num_samples=16448, **args)
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert len(got) == 242 and got == _keys()
    assert sum(v.numel() for v in net.state_dict().values()) == 16715937
    assert list(net.mid[0].attn.qkv.weight.shape) == [768, 256, 1, 1] and net.mid[0].attn.qkv.bias is None
    for rb, al, n_keys, n_par in ((2, [3, 4], 387, 25787009), (3, [4], 482, 32228961)):
        sd = NW.UNetModified(num_samples=2112, **dict(args, res_blocks=rb, attn_layer=al)).state_dict()
        assert (len(sd), sum(v.numel() for v in sd.values())) == (n_keys, n_par)
        assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(dict(args, res_blocks=rb, attn_layer=al))
    alone = NW.SelfAttention(256)
    assert [["mid.0.attn." + k, list(v.shape)] for k, v in alone.state_dict().items()] == [e for e in _keys() if e[0].startswith("mid.0.attn.")]
    assert sorted(alone.library_params()) == sorted(e[0] for e in _keys() if e[0].startswith("mid.0.attn."))


def test_library_config_round_trips_the_args():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    net = NW.UNetModified(num_samples=16448, **args)
    assert net.library_config()["network"] == {"type": "UNetModified", "args": args}
    assert net.library_config()["num_samples"] == 16448
    net = NW.UNetModified(num_samples=2112, **dict(args, channel_mults=(1, 2, 4), attn_layer=(1, 2)))
    assert net.library_config()["network"]["args"] == dict(args, channel_mults=[1, 2, 4], attn_layer=[1, 2])
    lib = NW.SelfAttention(160).library_config()
    assert lib["network"] == {"type": "UNetModified", "args": {"inner_channel": 32, "norm_groups": 32, "channel_mults": [5],
                                                               "attn_layer": [0], "res_blocks": 1}}
    for bad in (dict(in_channel=288), dict(in_channel=48, norm_groups=16), dict(in_channel=64, n_head=2)):
        with pytest.raises(NotImplementedError):
            NW.SelfAttention(**bad).library_config()


def test_facade_refuses_what_the_reference_refuses_and_host_tensors():
    import model.network as NW
    args = _reference_config()["network"]["args"]
    with pytest.raises(TypeError):
        NW.UNetModified(num_samples=2112, **dict(args, attn_layer=4))       # `ind in 4` (UNetModified.py:238)
    with pytest.raises(TypeError):
        NW.UNetModified(num_samples=2112)                                   # the class default (4) is an int
    with pytest.raises(TypeError):
        NW.UNetModified(num_samples=2112, with_noise_level_emb=False, **args)   # nn.Linear(None, ...) (UNetModified.py:67)
    with pytest.raises(AssertionError):
        NW.UNetModified(num_samples=2100, **args)                           # (2100 - 128) % 64 != 0 (UNetModified.py:13)
    net = NW.UNetModified(num_samples=2112, **args)
    z = torch.zeros(1, 1, 2112)
    with pytest.raises(RuntimeError):
        net(z, z, torch.ones(1))
    with pytest.raises(RuntimeError):
        net.mid[0].attn(torch.zeros(1, 256, 2, 8))


def test_shipped_config_builds(tmp_path):
    from parse_config import ConfigParser, read_json
    import infer
    import model.diffusion as module_diffusion
    import model.model as module_arch
    import model.network as module_network
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", "config_unetmodified.json"))
    assert cfg["network"]["args"] == _reference_config()["network"]["args"] and cfg["num_samples"] == 16448
    cfg["trainer"]["save_dir"] = str(tmp_path)
    config = ConfigParser(cfg, run_id="b")
    _, network, model = module_arch.build_from_config(config, module_diffusion, module_network, module_arch, "cpu")
    assert type(model).__name__ == "SDDM" and type(network).__name__ == "UNetModified"
    assert model.num_timesteps == 1000 and len(model.state_dict()) == 242 + 14
    lib = model.library_config()
    assert lib["network"] == {"type": "UNetModified", "args": cfg["network"]["args"]} and lib["num_samples"] == 16448


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("N", [2112, 16448])
def test_unetmodified_plans_in_every_dtype(N, dtype):
    """One attention step per attention layer, named <layer>.attn, and a kernel for every conv."""
    import sddm_hip
    import _unetmodified_oracle as O
    plan = sddm_hip.unet_plan(_plan_config("UNetModified", N, **{k: O.ARGS[k] for k in ("channel_mults", "attn_layer")}), None, dtype)
    layers = sorted(e[0][:-len(".qkv.weight")] for e in _keys() if e[0].endswith(".attn.qkv.weight"))
    attn = [s for s in plan if s["type"] == "attention"]
    assert sorted(s["name"] for s in attn) == layers == ["downs.9.attn", "mid.0.attn", "ups.0.attn", "ups.1.attn"]
    F = (N - 128) // 64 + 1
    for s in attn:
        assert (s["P"], s["C"]) == ((F // 16) * 8, 256) and s["P"] % s["QT"] == 0 and s["QT"] <= 64
        assert s["out"] == {"C": 256, "H": F // 16, "W": 8, "tiles": s["P"] // s["QT"], "n_tile": s["QT"]}
    convs = [s for s in plan if s["type"] == "conv"]
    assert len(convs) == 2 * 17 + 4 + 4                      # 17 ResnetBlocks (5 + 2 + 10), 4 Downsamples, 4 Upsamples
    for s in convs:
        assert sddm_hip.planned_kernel(s).split(":")[0] in ("strip", "tile", "deep", "wide"), s
        assert s["n_tiles"] * s["TR"] * s["TW"] == s["Ho"] * s["Wo"], s
    for s in convs:                                          # the strip kernel's res_conv holds 128 input channels
        assert not (s["kernel"] == "strip" and s["res"] == 2 and s["RCA"] + s["RCB"] > 128), s
    wide = [s["name"] for s in convs if s["kernel"] == "wide"]
    assert bool(wide) == (dtype == "float32")                # the 512-channel concats need the K-chunked kernel in float32 only
    assert [s["type"] for s in plan[:1] + plan[-1:]] == ["conv_in", "final"]


@pytest.mark.parametrize("N", [2112, 3136, 16448])
def test_wide_unetmodified2_plans_in_float32(N):
    """channel_mults [1, 2, 4, 8]: float32 used to fail with `no tile for downs.7`; the 16-bit plans have
    no wide kernel and the narrow float32 plan ([1, 2, 3, 4, 5]) has none either."""
    import sddm_hip
    plan = sddm_hip.unet_plan(_plan_config("UNetModified2", N, channel_mults=[1, 2, 4, 8]), None, "float32")
    wide = {s["name"]: sddm_hip.planned_kernel(s) for s in plan if s["type"] == "conv" and s["kernel"] == "wide"}
    assert "downs.7.block2" in wide and all(v.startswith("wide:") for v in wide.values())
    for s in plan:
        if s["type"] == "conv" and s["kernel"] == "wide":
            assert s["TR"] * s["TW"] == s["mt"] <= 64 and s["Ho"] % s["TR"] == 0 and s["Wo"] % s["TW"] == 0
    for dtype in ("bfloat16", "float16"):
        assert not [s for s in sddm_hip.unet_plan(_plan_config("UNetModified2", N, channel_mults=[1, 2, 4, 8]), None, dtype)
                    if s.get("kernel") == "wide"]
    if N != 3136:                                # 48 frames: the five-level default needs multiples of 32
        assert not [s for s in sddm_hip.unet_plan(_plan_config("UNetModified2", N, channel_mults=[1, 2, 3, 4, 5]), None, "float32")
                    if s.get("kernel") == "wide"]


def test_plan_refusals():
    import sddm_hip
    with pytest.raises(ValueError, match="attn_layer"):
        sddm_hip.unet_plan(_plan_config("UNetModified", 2112, channel_mults=[1, 2, 4, 8, 8], attn_layer=4))
    with pytest.raises(NotImplementedError, match="512 channels"):
        sddm_hip.unet_plan(_plan_config("UNetModified", 2112, channel_mults=[1, 2, 4, 8, 16], attn_layer=[4]))
    with pytest.raises(NotImplementedError, match="with_noise_level_emb"):
        sddm_hip.unet_plan(_plan_config("UNetModified", 2112, channel_mults=[1, 2], attn_layer=[], with_noise_level_emb=False))
    with pytest.raises(AssertionError):          # 31 frames: not a multiple of 2^(levels - 1) = 16
        sddm_hip.unet_plan(_plan_config("UNetModified", 128 + 30 * 64, channel_mults=[1, 2, 4, 8, 8], attn_layer=[4]))
    sddm_hip.unet_plan(_plan_config("UNetModified", 128 + 15 * 64, channel_mults=[1, 2, 4, 8, 8], attn_layer=[4]))   # 16 frames


def test_oracle_matches_reference_forward():
    """Pins the torch restatement that the larger GPU cases are checked against."""
    import _unetmodified_oracle as O
    shapes = O.param_shapes()
    assert [[k, list(s)] for k, s in sorted(shapes.items())] == sorted(_keys())
    z = golden("unetmodified.npz")
    ref = z["fw/eps"]
    P = O.make_params()
    eps = O.forward(P, z["fw/cond"], z["fw/x_t"], z["fw/noise_level"])
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"UNetModified: oracle vs reference rms {err:.3e} (reference rms {rms(ref, 0):.3f})")
    assert err <= 1e-5
    one = O.forward(P, z["fw/cond"][:1], z["fw/x_t"][:1], z["fw/noise_level"][:1])   # B = 1
    assert rms(one, ref[:1]) <= 1e-5
    from _weights import make_params
    flat = rms(O.forward(make_params(shapes, 0), z["fw/cond"], z["fw/x_t"], z["fw/noise_level"]), ref)
    print(f"UNetModified: the same without QK_SCALE moves the output by {flat:.3e}")
    assert flat >= 1e-3                          # the sharpened attention is part of what the golden pins


@pytest.mark.parametrize("C,H,W", AT_SHAPES)
def test_oracle_matches_reference_self_attention(C, H, W):
    import _unetmodified_oracle as O
    z = golden("unetmodified.npz")
    x, ref = z[f"at/{C}x{H}x{W}/x"], z[f"at/{C}x{H}x{W}/y"]
    P = _attn_params(C)
    y = O.self_attention(P, "mid.0.attn.", x)
    rel = rms(y, ref) / rms(ref, 0)
    std, pmax, amax = O.logit_stats(P, "mid.0.attn.", x)
    print(f"SelfAttention {C}x{H}x{W}: oracle vs reference relative rms {rel:.3e}; logit std {std:.2f}, "
          f"mean row-max probability {pmax:.3f}, max |logit| {amax:.1f}")
    assert y.shape == ref.shape and rel <= 2e-6
    assert std >= 2.0                            # a sharp attention: a wrong scale or a missing maximum shows
    # what the GPU test has to see: the scale 1 / sqrt(C) left out
    Q = dict(P)
    Q["mid.0.attn.qkv.weight"] = P["mid.0.attn.qkv.weight"].copy()
    Q["mid.0.attn.qkv.weight"][:C] *= np.float32(np.sqrt(C))
    moved = rms(O.self_attention(Q, "mid.0.attn.", x), ref) / rms(ref, 0)
    print(f"SelfAttention {C}x{H}x{W}: without the 1 / sqrt(C) scale the output moves by {moved:.3e}")
    assert moved >= (1e-2 if H * W > 1 else 0.0)


@pytest.mark.parametrize("nc,mode", [("sqrt_alpha_bar", "sr3"), ("time_step", "original")])
def test_oracle_sampling_matches_reference(nc, mode):
    import _unetmodified_oracle as O
    from oracle import sampler
    z = golden("unetmodified.npz")
    P = O.make_params()
    rec = []
    out = sampler.infer(lambda c, x, nl: O.forward(P, c, x, nl), tables_from_golden("linear_3_0.0001_0.05"),
                        z["inf/cond"], mode=mode, noise_condition=nc, seed=7, record=rec)
    steps = z[f"inf/{nc}/{mode}/steps"]
    errs = [rms(a, b) for a, b in zip(rec[1:], steps)]
    print(f"UNetModified {nc} {mode}: oracle sampler vs reference, x_t per step {['%.2e' % e for e in errs]}")
    assert rms(out, steps[-1]) <= 1e-5 and max(errs) <= 1e-5


def test_emulation_rounds_the_attention():
    """The 16-bit emulation moves the block's output by about the rounding of its operands."""
    import _unetmodified_oracle as O
    z = golden("unetmodified.npz")
    x, ref = z["at/256x16x8/x"], z["at/256x16x8/y"]
    P = _attn_params(256)
    for dtype, lo, hi in ((torch.bfloat16, 1e-3, 3e-2), (torch.float16, 1e-4, 5e-3)):
        rel = rms(O.self_attention(P, "mid.0.attn.", x, rounding=dtype), ref) / rms(ref, 0)
        print(f"SelfAttention 256x16x8 {dtype}: emulation vs reference relative rms {rel:.3e}")
        assert lo <= rel <= hi
