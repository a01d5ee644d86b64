"""ORACLE (test infrastructure only) -- the FiLM Wave-U-Nets' forward restated with torch functionals on the CPU.

One implementation, two instances.  ``WAVEUNET`` restates the reference's model/waveunet.py (358-506) at
the arguments of config_waveunet.json (twelve levels, channels 24, 48, ..., 288, res 'learned'), and
``WAVEUNET2`` its model/waveunet2.py (226-324) at those of config_waveunet2.json (channels [24, 48, 72,
96]).  Both: 5-tap convs, learned 4-tap stride-2 resampling, GroupNorm conv layers, depth 1, FiLM blocks
on the shortcuts, in float64; the result is rounded to float32.  They differ in the argument names, the
key of the learned resampling convs (``downconv.`` / ``upconv.`` against ``downconv.down.`` /
``upconv.up.``) and the number of levels.  Weights: dict of numpy arrays keyed like the reference
state_dict without the ``noise_estimate_model.`` prefix.  Any batch size, 1 included (the reference's
PositionalEncoding squeezes a single level to 0-d and fails).

``forward(..., rounding=torch.bfloat16 / torch.float16)`` is the CPU emulation of the 16-bit paths:
every convolution's input, weight and output are rounded to that type (the arithmetic stays float64).
"""
import numpy as np
import torch
import torch.nn.functional as F


def _encoding(level, dim):
    """PositionalEncoding._build_encoding (waveunet.py:34-39, waveunet2.py:34-39): level [B] -> [B, dim, 1]."""
    count = dim // 2
    step = torch.arange(count, dtype=torch.float64) / count
    e = level.reshape(-1, 1) * torch.exp(-np.log(1e4) * step.unsqueeze(0))
    return torch.cat([torch.sin(e), torch.cos(e)], dim=-1)[:, :, None]


class _FilmWaveunet:
    def __init__(self, channels, args, down_key, up_key):
        self.CHANNELS = tuple(channels)
        self.HOP = 2 ** (len(self.CHANNELS) - 1)
        self.ARGS = dict(args, num_channels=list(self.CHANNELS))
        self._down_key, self._up_key = down_key, up_key

    def _layers(self):
        """(kind, key prefix, cin, cout) of every ConvLayer in forward order; kind is 'pre' (its output is
        the shortcut, the FiLM block follows), 'conv', 'down', 'up' or 'post' (its input takes the FiLM)."""
        C, seq = self.CHANNELS, []
        n = len(C) - 1
        for i in range(n):
            p = f"waveunet.downsampling_blocks.{i}."
            seq.append(("pre", p + "pre_shortcut_convs.0.", 2 if i == 0 else C[i], C[i]))
            seq.append(("conv", p + "post_shortcut_convs.0.", C[i], C[i + 1]))
            seq.append(("down", p + self._down_key, C[i + 1], C[i + 1]))
        seq.append(("conv", "waveunet.bottlenecks.0.", C[n], C[n]))
        for j, i in enumerate(range(n, 0, -1)):
            p = f"waveunet.upsampling_blocks.{j}."
            seq.append(("up", p + self._up_key, C[i], C[i]))
            seq.append(("conv", p + "pre_shortcut_convs.0.", C[i], C[i - 1]))
            seq.append(("post", p + "post_shortcut_convs.0.", C[i - 1], C[i - 1]))
        return seq

    def param_shapes(self):
        """State-dict shapes without the module prefix (314 tensors for Waveunet, 90 for Waveunet2)."""
        s = {}
        for kind, p, ci, co in self._layers():
            k = 4 if kind in ("down", "up") else 5
            s[p + "filter.weight"], s[p + "filter.bias"] = (co, ci, k), (co,)       # ConvTranspose1d: [ci][co][k], ci == co
            s[p + "norm.weight"], s[p + "norm.bias"] = (co,), (co,)
        for i in range(len(self.CHANNELS) - 1):
            p, c = f"waveunet.film_blocks.{i}.", self.CHANNELS[i]
            s[p + "input_conv.weight"], s[p + "input_conv.bias"] = (c, c, 3), (c,)
            s[p + "output_conv.weight"], s[p + "output_conv.bias"] = (2 * c, c, 3), (2 * c,)
        s["waveunet.output_conv.weight"], s["waveunet.output_conv.bias"] = (1, self.CHANNELS[0], 1), (1,)
        return s

    def forward(self, P, x, y_t, noise_level, rounding=None):
        """forward(x, y_t, noise_level): x (condition), y_t [B, 1, N], noise level [B] -> [B, 1, N]."""
        def q(t):
            return t if rounding is None else t.to(rounding).to(torch.float64)

        def conv(fn, t, w, b, **kw):
            return q(fn(q(t), q(w), b, **kw))
        W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items()}
        x = torch.from_numpy(np.asarray(x, np.float64).reshape(len(x), 1, -1))
        y_t = torch.from_numpy(np.asarray(y_t, np.float64).reshape(len(y_t), 1, -1))
        level = torch.from_numpy(np.asarray(noise_level, np.float64).reshape(-1))
        assert x.shape == y_t.shape and x.shape[2] % self.HOP == 0 and x.shape[2] >= self.HOP and len(level) == len(x)
        out, films = torch.cat([x, y_t], dim=1), []
        for kind, p, ci, co in self._layers():
            if kind == "post":
                shift, scale = films.pop()
                out = scale * out + shift
            if kind == "down":
                out = conv(F.conv1d, out, W[p + "filter.weight"], W[p + "filter.bias"], stride=2, padding=1)
            elif kind == "up":
                out = conv(F.conv_transpose1d, out, W[p + "filter.weight"], W[p + "filter.bias"], stride=2, padding=1)
            else:
                out = conv(F.conv1d, out, W[p + "filter.weight"], W[p + "filter.bias"], padding=2)
            out = F.relu(F.group_norm(out, co // 8, W[p + "norm.weight"], W[p + "norm.bias"], eps=1e-5))
            if kind == "pre":
                f = "waveunet.film_blocks.%d." % len(films)
                h = conv(F.conv1d, out, W[f + "input_conv.weight"], W[f + "input_conv.bias"], padding=1)
                h = F.leaky_relu(h, 0.2) + _encoding(level, co)
                h = conv(F.conv1d, h, W[f + "output_conv.weight"], W[f + "output_conv.bias"], padding=1)
                films.append(torch.chunk(h, 2, dim=1))
        out = conv(F.conv1d, out, W["waveunet.output_conv.weight"], W["waveunet.output_conv.bias"])
        return out.clamp(-1.0, 1.0).numpy().astype(np.float32)


WAVEUNET = _FilmWaveunet(
    (24 * (i + 1) for i in range(12)),
    {"num_inputs": 2, "num_channels": None, "kernel_size": 5, "conv_type": "gn", "res": "learned", "depth": 1,
     "resample_kernel_size": 4, "resample_stride": 2},
    "downconv.", "upconv.")
WAVEUNET2 = _FilmWaveunet(
    (24, 48, 72, 96),
    {"num_inputs": 2, "num_channels": None, "downconv_kernel_size": 5, "upconv_kernel_size": 5,
     "bottleneck_kernel_size": 5, "conv_stride": 1, "conv_type": "gn", "depth": 1, "downsample_kernel_size": 4,
     "upsample_kernel_size": 4, "resample_stride": 2},
    "downconv.down.", "upconv.up.")
