"""Waveunet2 facade (reference model/waveunet2.py:226-324, config_waveunet2.json).

The module tree only holds the parameters under the reference's state-dict keys
(``waveunet.downsampling_blocks.0.pre_shortcut_convs.0.filter.weight`` ...); the forward runs in
libsddm_hip (csrc/waveunet2.hip, the conv and stem kernels it shares with Waveunet3 in
csrc/wu_conv_impl.h, wu2_runtime.h).  Supported: the arguments of config_waveunet2.json
-- channels [24, 48, 72, 96], 5-tap convs, 4-tap stride-2 resampling, conv_type 'gn', depth 1, two
inputs; everything else is refused by the library when the context is configured.  The chunk length
is any positive multiple of 8 (three stride-2 levels).  The output is always clamped to [-1, 1]:
there is no training mode here.
"""
import torch
from torch import nn


def _conv_layer(n_inputs, n_outputs, kernel_size, stride, conv_type, padding="same", transpose=False):
    """ConvLayer (waveunet2.py:64-103): filter, and with conv_type 'gn' a GroupNorm over groups of 8."""
    m = nn.Module()
    if transpose:
        m.filter = nn.ConvTranspose1d(n_inputs, n_outputs, kernel_size, stride, padding=(kernel_size - stride) // 2)
    else:
        m.filter = nn.Conv1d(n_inputs, n_outputs, kernel_size, stride, padding=padding)
    if conv_type == "gn":
        assert n_outputs % 8 == 0
        m.norm = nn.GroupNorm(n_outputs // 8, n_outputs)
    elif conv_type == "bn":
        m.norm = nn.BatchNorm1d(n_outputs, momentum=0.01)
    return m


def _film(size):
    """FiLM(size, size) (waveunet2.py:42-61): the encoding has no parameters."""
    m = nn.Module()
    m.input_conv = nn.Conv1d(size, size, 3, padding=1)
    m.output_conv = nn.Conv1d(size, size * 2, 3, padding=1)
    return m


class Waveunet2(nn.Module):
    hop_samples = 8                      # 2 ** (levels - 1): chunks are positive multiples of it

    def __init__(self, num_inputs, num_channels, downconv_kernel_size, upconv_kernel_size, bottleneck_kernel_size,
                 conv_stride, conv_type, depth=1, downsample_kernel_size=4, upsample_kernel_size=4, resample_stride=2,
                 num_samples=-1):
        super().__init__()
        assert downconv_kernel_size % 2 == 1                                 # only odd filter kernels
        assert upconv_kernel_size % 2 == 1
        assert (downsample_kernel_size - resample_stride) % 2 == 0
        assert (upsample_kernel_size - resample_stride) % 2 == 0
        assert resample_stride > 1
        self.config_args = {
            "num_inputs": num_inputs, "num_channels": list(num_channels), "downconv_kernel_size": downconv_kernel_size,
            "upconv_kernel_size": upconv_kernel_size, "bottleneck_kernel_size": bottleneck_kernel_size,
            "conv_stride": conv_stride, "conv_type": conv_type, "depth": depth,
            "downsample_kernel_size": downsample_kernel_size, "upsample_kernel_size": upsample_kernel_size,
            "resample_stride": resample_stride}
        C, n = list(num_channels), len(num_channels)

        def convs(first, rest, count, k):
            return nn.ModuleList([_conv_layer(*first, k, 1, conv_type)] +
                                 [_conv_layer(*rest, k, 1, conv_type) for _ in range(count - 1)])
        w = nn.Module()
        w.downsampling_blocks = nn.ModuleList()
        w.upsampling_blocks = nn.ModuleList()
        w.film_blocks = nn.ModuleList()
        for i in range(n - 1):
            cin, k = (num_inputs if i == 0 else C[i]), downconv_kernel_size
            d = nn.Module()
            d.pre_shortcut_convs = convs((cin, C[i]), (C[i], C[i]), depth, k)
            d.post_shortcut_convs = convs((C[i], C[i + 1]), (C[i + 1], C[i + 1]), depth, k)
            d.downconv = nn.Module()
            d.downconv.down = _conv_layer(C[i + 1], C[i + 1], downsample_kernel_size, resample_stride, conv_type,
                                          padding=(downsample_kernel_size - resample_stride) // 2)
            w.downsampling_blocks.append(d)
            w.film_blocks.append(_film(C[i]))
        for i in range(n - 1, 0, -1):
            k = upconv_kernel_size
            u = nn.Module()
            u.upconv = nn.Module()
            u.upconv.up = _conv_layer(C[i], C[i], upsample_kernel_size, resample_stride, conv_type, transpose=True)
            u.pre_shortcut_convs = convs((C[i], C[i - 1]), (C[i - 1], C[i - 1]), depth, k)
            u.post_shortcut_convs = nn.ModuleList([_conv_layer(C[i - 1], C[i - 1], k, 1, conv_type) for _ in range(depth)])
            w.upsampling_blocks.append(u)
        w.bottlenecks = nn.ModuleList([_conv_layer(C[-1], C[-1], bottleneck_kernel_size, 1, conv_type)
                                       for _ in range(depth)])
        w.output_conv = nn.Conv1d(C[0], 1, 1)
        self.waveunet = w
        self.num_samples = -1
        self.compute_dtype = "float32"
        self._ctx = None
        self._ctx_key = None

    def library_config(self):
        return {"arch": {"type": "SDDM", "args": {}},
                "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 1}},
                "network": {"type": "Waveunet2", "args": self.config_args}, "num_samples": -1}

    def _context(self, device):
        import sddm_hip
        sd = dict(self.state_dict())
        key = (device.index or 0, self.compute_dtype) + tuple((k, v.data_ptr(), v._version) for k, v in sd.items())
        if self._ctx is None or self._ctx_key != key:
            ctx = sddm_hip.Context(self.library_config(), device.index or 0, self.compute_dtype)
            ctx.load_state_dict(sd)
            self._ctx, self._ctx_key = ctx, key
        return self._ctx

    @torch.no_grad()
    def forward(self, x, y_t, noise_level):
        """x (condition) and y_t [B, 1, N], N a positive multiple of 8; noise_level [B] or [B, 1, 1]
        -> clamp(output_conv(...), -1, 1) [B, 1, N] (waveunet2.py:293-324, eval mode)."""
        if not y_t.is_cuda:
            raise RuntimeError("Waveunet2 runs on the HIP device; move the tensors to cuda")
        B = y_t.shape[0]
        cond = x.reshape(B, 1, -1).contiguous().float()
        yt = y_t.reshape(B, 1, -1).contiguous().float()
        if cond.shape != yt.shape:
            raise RuntimeError(f"condition {tuple(x.shape)} and y_t {tuple(y_t.shape)} differ in size")
        nl = noise_level.reshape(-1).contiguous().float()
        if nl.numel() != B:
            raise RuntimeError(f"noise_level has {nl.numel()} elements for batch {B}")
        out = torch.empty_like(yt)
        self._context(yt.device).network_forward(cond, yt, nl, out)
        return out
