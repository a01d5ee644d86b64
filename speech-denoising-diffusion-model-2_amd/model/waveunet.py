"""The FiLM Wave-U-Net facades: Waveunet (reference model/waveunet.py:358-506, config_waveunet.json)
and Waveunet2 (reference model/waveunet2.py:226-324, config_waveunet2.json).

They are the same network at two sizes, as csrc/wu2_runtime.h (wu2::Net) says: they differ in the
constructor's argument names, the key of the learned resampling convs in their blocks
(``downconv.filter.*`` / ``upconv.filter.*`` for Waveunet, ``downconv.down.filter.*`` /
``upconv.up.filter.*`` for Waveunet2) and the number of levels -- twelve of 24, 48, ..., 288 channels
against four of [24, 48, 72, 96].  The module tree only holds the parameters under the reference's
state-dict keys (``waveunet.downsampling_blocks.0.pre_shortcut_convs.0.filter.weight`` ...); the
forward runs in libsddm_hip (the layer sequence of csrc/wu2_runtime.h over the conv kernel of
csrc/wu_conv_impl.h: csrc/waveunet2.hip, and for Waveunet csrc/waveunet1.hip with the layer's output
channels split over the grid).  Supported: the arguments of the two configs -- 5-tap convs, learned
4-tap stride-2 resampling (Waveunet: res 'learned'), conv_type 'gn', depth 1, two inputs; everything
else is refused by the library when the context is configured.  The chunk length is any positive
multiple of ``hop_samples`` (one stride-2 level less than there are channel counts).  The output is
always clamped to [-1, 1]: there is no training mode here.
"""
from torch import nn

from ._facade import StrictFacade


def _conv_layer(n_inputs, n_outputs, kernel_size, stride, conv_type, padding="same", transpose=False):
    """ConvLayer (waveunet.py:206-245, waveunet2.py:64-103): filter, and with conv_type 'gn' a GroupNorm over groups of 8."""
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
    """FiLM(size, size) (waveunet.py:42-61, waveunet2.py:42-61): the encoding has no parameters."""
    m = nn.Module()
    m.input_conv = nn.Conv1d(size, size, 3, padding=1)
    m.output_conv = nn.Conv1d(size, size * 2, 3, padding=1)
    return m


def _film_waveunet(num_inputs, C, k_down, k_up, k_bottleneck, k_downsample, k_upsample, stride, conv_type, depth,
                   nested):
    """The parameter tree of a FiLM Wave-U-Net over the channel counts C.  nested: the learned
    resampling convs sit at ``downconv.down`` / ``upconv.up`` (Waveunet2), else at ``downconv`` /
    ``upconv`` themselves (Waveunet)."""
    def convs(first, rest, count, k):
        return nn.ModuleList([_conv_layer(*first, k, 1, conv_type)] +
                             [_conv_layer(*rest, k, 1, conv_type) for _ in range(count - 1)])

    def resample(layer, name):
        if not nested:
            return layer
        m = nn.Module()
        setattr(m, name, layer)
        return m
    n = len(C)
    w = nn.Module()
    w.downsampling_blocks = nn.ModuleList()
    w.upsampling_blocks = nn.ModuleList()
    w.film_blocks = nn.ModuleList()
    for i in range(n - 1):
        cin = num_inputs if i == 0 else C[i]
        d = nn.Module()
        d.pre_shortcut_convs = convs((cin, C[i]), (C[i], C[i]), depth, k_down)
        d.post_shortcut_convs = convs((C[i], C[i + 1]), (C[i + 1], C[i + 1]), depth, k_down)
        d.downconv = resample(_conv_layer(C[i + 1], C[i + 1], k_downsample, stride, conv_type,
                                          padding=(k_downsample - stride) // 2), "down")
        w.downsampling_blocks.append(d)
        w.film_blocks.append(_film(C[i]))
    for i in range(n - 1, 0, -1):
        u = nn.Module()
        u.upconv = resample(_conv_layer(C[i], C[i], k_upsample, stride, conv_type, transpose=True), "up")
        u.pre_shortcut_convs = convs((C[i], C[i - 1]), (C[i - 1], C[i - 1]), depth, k_up)
        u.post_shortcut_convs = nn.ModuleList([_conv_layer(C[i - 1], C[i - 1], k_up, 1, conv_type) for _ in range(depth)])
        w.upsampling_blocks.append(u)
    w.bottlenecks = nn.ModuleList([_conv_layer(C[-1], C[-1], k_bottleneck, 1, conv_type) for _ in range(depth)])
    w.output_conv = nn.Conv1d(C[0], 1, 1)
    return w


class Waveunet(StrictFacade):
    """forward(x, y_t, noise_level): x (condition) and y_t [B, 1, N], N a positive multiple of 2048;
    noise_level [B] or [B, 1, 1] -> clamp(output_conv(...), -1, 1) [B, 1, N] (waveunet.py:475-506, eval mode)."""

    hop_samples = 2048                   # 2 ** (levels - 1) at the config's twelve levels: chunks are positive multiples of it

    def __init__(self, num_inputs, num_channels, kernel_size, input_size=-1, conv_type="gn", res="learned", depth=1,
                 resample_kernel_size=4, resample_stride=2, num_samples=-1):
        """The reference's signature and argument order; ``input_size`` has a default because the
        reference's own infer.py passes ``num_samples=`` instead (which is accepted and ignored)."""
        super().__init__()
        assert kernel_size % 2 == 1                                          # only odd filter kernels
        assert (resample_kernel_size - resample_stride) % 2 == 0
        assert resample_stride > 1
        self._init_facade({
            "num_inputs": num_inputs, "num_channels": list(num_channels), "kernel_size": kernel_size,
            "conv_type": conv_type, "res": res, "depth": depth, "resample_kernel_size": resample_kernel_size,
            "resample_stride": resample_stride})
        self.waveunet = _film_waveunet(num_inputs, list(num_channels), kernel_size, kernel_size, kernel_size,
                                       resample_kernel_size, resample_kernel_size, resample_stride, conv_type, depth,
                                       nested=False)
        # check_output_size (waveunet.py:401-426) without its prints: every level halves the length
        # exactly (floor((L + 2 - 4 + 2) / 2) = L / 2 needs an even L) and doubles it on the way up
        hop = 2 ** (len(num_channels) - 1)
        if input_size >= 0 and (input_size < hop or input_size % hop):
            raise AssertionError(f"input_size {input_size} is not a positive multiple of {hop}")


class Waveunet2(StrictFacade):
    """forward(x, y_t, noise_level): x (condition) and y_t [B, 1, N], N a positive multiple of 8;
    noise_level [B] or [B, 1, 1] -> clamp(output_conv(...), -1, 1) [B, 1, N] (waveunet2.py:293-324, eval mode)."""

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
        self._init_facade({
            "num_inputs": num_inputs, "num_channels": list(num_channels), "downconv_kernel_size": downconv_kernel_size,
            "upconv_kernel_size": upconv_kernel_size, "bottleneck_kernel_size": bottleneck_kernel_size,
            "conv_stride": conv_stride, "conv_type": conv_type, "depth": depth,
            "downsample_kernel_size": downsample_kernel_size, "upsample_kernel_size": upsample_kernel_size,
            "resample_stride": resample_stride})
        self.waveunet = _film_waveunet(num_inputs, list(num_channels), downconv_kernel_size, upconv_kernel_size,
                                       bottleneck_kernel_size, downsample_kernel_size, upsample_kernel_size,
                                       resample_stride, conv_type, depth, nested=True)
