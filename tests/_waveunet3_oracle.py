"""ORACLE (test infrastructure only) -- Waveunet3 forward restated with torch functionals on the CPU.

Restates the reference's model/waveunet3.py (314-416) at the arguments of config_waveunet3.json
(channels [32, 64, 96, 128], 5-tap convs, 4-tap stride-2 resampling, GroupNorm conv layers, no
attention, no noise-level embedding) in float64; the result is rounded to float32.  Weights: dict of
numpy arrays keyed like the reference state_dict without the ``noise_estimate_model.`` prefix.
"""
import numpy as np
import torch
import torch.nn.functional as F

CHANNELS = (32, 64, 96, 128)
ARGS = {"num_inputs": 2, "num_channels": list(CHANNELS), "downconv_kernel_size": 5, "upconv_kernel_size": 5,
        "bottleneck_kernel_size": 5, "conv_stride": 1, "conv_type": "gn", "downsample_kernel_size": 4,
        "upsample_kernel_size": 4, "resample_stride": 2, "with_noise_level_emb": False, "norm_groups": 32,
        "with_attn": False, "dropout": 0}


def _blocks():
    """(key prefix, cin, cout, groups of block1's GroupNorm) of every ResnetBlock, in forward order,
    interleaved with the resampling layers ('down' / 'up', prefix, channels)."""
    C, seq = CHANNELS, []
    for i in range(3):
        p = f"waveunet.downsampling_blocks.{i}."
        cin, g = (2, 2) if i == 0 else (C[i], 32)
        seq.append(("res", p + "pre_shortcut.0.res_block.", cin, C[i], g))
        seq.append(("res", p + "post_shortcut.0.res_block.", C[i], C[i + 1], g))
        seq.append(("down", p + "downconv.down.", C[i + 1]))
    for j in range(2):
        seq.append(("res", f"waveunet.bottlenecks.{j}.res_block.", C[3], C[3], 32))
    for j, i in enumerate((3, 2, 1)):
        p = f"waveunet.upsampling_blocks.{j}."
        seq.append(("up", p + "upconv.up.", C[i]))
        seq.append(("res", p + "pre_shortcut.0.res_block.", C[i], C[i - 1], 32))
        seq.append(("res", p + "post_shortcut.0.res_block.", C[i - 1], C[i - 1], 32))
    return seq


def param_shapes():
    """State-dict shapes without the module prefix (180 tensors)."""
    s = {}
    for item in _blocks():
        if item[0] == "res":
            _, p, ci, co, _ = item
            s[p + "noise_func.noise_func.0.weight"], s[p + "noise_func.noise_func.0.bias"] = (co, 1), (co,)
            for b, c in (("block1", ci), ("block2", co)):
                s[p + b + ".block.0.weight"], s[p + b + ".block.0.bias"] = (c,), (c,)
                s[p + b + ".block.3.weight"], s[p + b + ".block.3.bias"] = (co, c, 5), (co,)
            if ci != co:
                s[p + "res_conv.weight"], s[p + "res_conv.bias"] = (co, ci, 1), (co,)
        else:
            _, p, c = item
            s[p + "filter.weight"], s[p + "filter.bias"] = (c, c, 4), (c,)
            s[p + "norm.weight"], s[p + "norm.bias"] = (c,), (c,)
    s["waveunet.output_conv.weight"], s["waveunet.output_conv.bias"] = (1, 32, 1), (1,)
    return s


def _resnet(W, p, x, level, ci, co, g1):
    h = F.silu(F.group_norm(x, g1, W[p + "block1.block.0.weight"], W[p + "block1.block.0.bias"]))
    h = F.conv1d(h, W[p + "block1.block.3.weight"], W[p + "block1.block.3.bias"], padding=2)
    h = h + F.linear(level, W[p + "noise_func.noise_func.0.weight"], W[p + "noise_func.noise_func.0.bias"]).transpose(1, 2)
    # block2's GroupNorm takes the block's norm_groups too (waveunet3.py:80-81): the first
    # DownsamplingBlock is built with norm_groups = num_inputs = 2 (waveunet3.py:339-342), so all four
    # of its GroupNorms have 2 groups (GroupNorm(2, 2), (2, 32), (2, 32), (2, 64))
    h = F.silu(F.group_norm(h, g1, W[p + "block2.block.0.weight"], W[p + "block2.block.0.bias"]))
    h = F.conv1d(h, W[p + "block2.block.3.weight"], W[p + "block2.block.3.bias"], padding=2)
    res = F.conv1d(x, W[p + "res_conv.weight"], W[p + "res_conv.bias"]) if ci != co else x
    return h + res


def forward(P, x, y_t, noise_level):
    """forward(x, y_t, noise_level): x (condition), y_t [B, 1, N], noise level [B] -> [B, 1, N]."""
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items()}
    x = torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), 1, -1))
    y_t = torch.from_numpy(np.asarray(y_t, np.float64).reshape(len(y_t), 1, -1))
    level = torch.from_numpy(np.asarray(noise_level, np.float64).reshape(-1, 1, 1))
    assert x.shape == y_t.shape and x.shape[2] % 8 == 0 and x.shape[2] >= 8
    out, shorts = torch.cat([x, y_t], dim=1), []
    for item in _blocks():
        if item[0] == "res":
            _, p, ci, co, g = item
            if "upsampling" in p and "post_shortcut" in p:
                out = out + shorts.pop()
            out = _resnet(W, p, out, level, ci, co, g)
            if "downsampling" in p and "pre_shortcut" in p:
                shorts.append(out)
        else:
            kind, p, c = item
            conv = F.conv1d if kind == "down" else F.conv_transpose1d
            out = conv(out, W[p + "filter.weight"], W[p + "filter.bias"], stride=2, padding=1)
            out = F.relu(F.group_norm(out, c // 8, W[p + "norm.weight"], W[p + "norm.bias"]))
    out = F.conv1d(out, W["waveunet.output_conv.weight"], W["waveunet.output_conv.bias"])
    return out.clamp(-1.0, 1.0).numpy().astype(np.float32)
