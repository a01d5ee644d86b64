"""Waveunet3 facade (reference model/waveunet3.py:314-416, config_waveunet3.json).

The module tree only holds the parameters under the reference's state-dict keys
(``waveunet.downsampling_blocks.0.pre_shortcut.0.res_block.block1.block.3.weight`` ...); the forward
runs in libsddm_hip (csrc/waveunet.hip, the conv and stem kernels it shares with Waveunet2 in
csrc/wu_conv_impl.h, wu_runtime.h).  Supported: the arguments of
config_waveunet3.json -- channels [32, 64, 96, 128], 5-tap convs, 4-tap stride-2 resampling,
conv_type 'gn', no attention, no noise-level embedding.  The chunk length is any positive multiple
of 8 (three stride-2 levels).
"""
from torch import nn

from ._facade import StrictFacade


def _block(dim, dim_out, kernel_size, groups):
    """GroupNorm -> SiLU -> (dropout slot) -> Conv1d, parameters at block.0 / block.3."""
    m = nn.Module()
    m.block = nn.Sequential(nn.GroupNorm(groups, dim), nn.SiLU(), nn.Identity(),
                            nn.Conv1d(dim, dim_out, kernel_size, padding="same"))
    return m


def _resnet_block(dim, dim_out, kernel_size, norm_groups):
    """res_block of a ResnetBlocWithAttn without attention (waveunet3.py:73-89, 124-137)."""
    holder, r = nn.Module(), nn.Module()
    r.noise_func = nn.Module()
    r.noise_func.noise_func = nn.Sequential(nn.Linear(1, dim_out))
    r.block1 = _block(dim, dim_out, kernel_size, norm_groups)
    r.block2 = _block(dim_out, dim_out, kernel_size, norm_groups)
    r.res_conv = nn.Conv1d(dim, dim_out, 1) if dim != dim_out else nn.Identity()
    holder.res_block = r
    return holder


def _resample(channels, kernel_size, stride, transpose):
    """ConvLayer with conv_type 'gn' (waveunet3.py:140-179): filter + GroupNorm over groups of 8."""
    m = nn.Module()
    pad = (kernel_size - stride) // 2
    conv = nn.ConvTranspose1d if transpose else nn.Conv1d
    m.filter = conv(channels, channels, kernel_size, stride, padding=pad)
    m.norm = nn.GroupNorm(channels // 8, channels)
    return m


class Waveunet3(StrictFacade):
    """forward(x, y_t, noise_level): x (condition) and y_t [B, 1, N], N a positive multiple of 8;
    noise_level [B] or [B, 1, 1] -> clamp(output_conv(...), -1, 1) [B, 1, N] (waveunet3.py:383-416, eval mode)."""

    hop_samples = 8                      # 2 ** (levels - 1): chunks are positive multiples of it

    def __init__(self, num_inputs, num_channels, downconv_kernel_size, upconv_kernel_size, bottleneck_kernel_size,
                 conv_stride, conv_type, downsample_kernel_size=4, upsample_kernel_size=4, resample_stride=2,
                 with_noise_level_emb=False, norm_groups=32, with_attn=True, dropout=0, num_samples=-1):
        super().__init__()
        assert (downsample_kernel_size - resample_stride) % 2 == 0
        assert (upsample_kernel_size - resample_stride) % 2 == 0
        assert num_channels[0] == norm_groups
        if with_noise_level_emb:
            raise NotImplementedError
        if with_attn:
            raise NotImplementedError("Waveunet3 with self-attention (with_attn=True) has no HIP kernels")
        self._init_facade({
            "num_inputs": num_inputs, "num_channels": list(num_channels), "downconv_kernel_size": downconv_kernel_size,
            "upconv_kernel_size": upconv_kernel_size, "bottleneck_kernel_size": bottleneck_kernel_size,
            "conv_stride": conv_stride, "conv_type": conv_type, "downsample_kernel_size": downsample_kernel_size,
            "upsample_kernel_size": upsample_kernel_size, "resample_stride": resample_stride,
            "with_noise_level_emb": bool(with_noise_level_emb), "norm_groups": norm_groups, "with_attn": bool(with_attn),
            "dropout": dropout})
        C, n = list(num_channels), len(num_channels)
        self.noise_level_mlp = None
        w = nn.Module()
        w.downsampling_blocks = nn.ModuleList()
        w.upsampling_blocks = nn.ModuleList()
        for i in range(n - 1):
            cin, g = (num_inputs, num_inputs) if i == 0 else (C[i], norm_groups)
            d = nn.Module()
            d.pre_shortcut = nn.ModuleList([_resnet_block(cin, C[i], downconv_kernel_size, g)])
            d.post_shortcut = nn.ModuleList([_resnet_block(C[i], C[i + 1], downconv_kernel_size, g)])
            d.downconv = nn.Module()
            d.downconv.down = _resample(C[i + 1], downsample_kernel_size, resample_stride, False)
            w.downsampling_blocks.append(d)
        for i in range(n - 1, 0, -1):
            u = nn.Module()
            u.upconv = nn.Module()
            u.upconv.up = _resample(C[i], upsample_kernel_size, resample_stride, True)
            u.pre_shortcut = nn.ModuleList([_resnet_block(C[i], C[i - 1], upconv_kernel_size, norm_groups)])
            u.post_shortcut = nn.ModuleList([_resnet_block(C[i - 1], C[i - 1], upconv_kernel_size, norm_groups)])
            w.upsampling_blocks.append(u)
        w.bottlenecks = nn.ModuleList([_resnet_block(C[-1], C[-1], bottleneck_kernel_size, norm_groups) for _ in range(2)])
        w.output_conv = nn.Conv1d(C[0], 1, 1)
        self.waveunet = w
