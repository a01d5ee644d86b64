"""Waveunet facade (reference model/waveunet.py:358-506, config_waveunet.json).

The module tree only holds the parameters under the reference's state-dict keys
(``waveunet.downsampling_blocks.0.pre_shortcut_convs.0.filter.weight`` ...; the learned resampling
convs are ``downconv.filter.*`` and ``upconv.filter.*`` directly); the forward runs in libsddm_hip
(csrc/waveunet1.hip, the conv kernel of csrc/wu_conv_impl.h with the layer's output channels split
over the grid; the layer sequence is csrc/wu2_runtime.h, shared with Waveunet2).  Supported: the arguments of config_waveunet.json -- twelve levels of
24, 48, ..., 288 channels, 5-tap convs, learned 4-tap stride-2 resampling (res 'learned'), conv_type
'gn', depth 1, two inputs; everything else is refused by the library when the context is
configured.  The chunk length is any positive multiple of 2048 (eleven stride-2 levels).  The output
is always clamped to [-1, 1]: there is no training mode here.
"""
import torch
from torch import nn


def _conv_layer(n_inputs, n_outputs, kernel_size, stride, conv_type, padding="same", transpose=False):
    """ConvLayer (waveunet.py:206-245): filter, and with conv_type 'gn' a GroupNorm over groups of 8."""
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
    """FiLM(size, size) (waveunet.py:42-61): the encoding has no parameters."""
    m = nn.Module()
    m.input_conv = nn.Conv1d(size, size, 3, padding=1)
    m.output_conv = nn.Conv1d(size, size * 2, 3, padding=1)
    return m


class Waveunet(nn.Module):
    hop_samples = 2048                   # 2 ** (levels - 1) at the config's twelve levels: chunks are positive multiples of it

    def __init__(self, num_inputs, num_channels, kernel_size, input_size=-1, conv_type="gn", res="learned", depth=1,
                 resample_kernel_size=4, resample_stride=2, num_samples=-1):
        """The reference's signature and argument order; ``input_size`` has a default because the
        reference's own infer.py passes ``num_samples=`` instead (which is accepted and ignored)."""
        super().__init__()
        assert kernel_size % 2 == 1                                          # only odd filter kernels
        assert (resample_kernel_size - resample_stride) % 2 == 0
        assert resample_stride > 1
        self.config_args = {
            "num_inputs": num_inputs, "num_channels": list(num_channels), "kernel_size": kernel_size,
            "conv_type": conv_type, "res": res, "depth": depth, "resample_kernel_size": resample_kernel_size,
            "resample_stride": resample_stride}
        C, n, k = list(num_channels), len(num_channels), kernel_size

        def convs(first, rest, count):
            return nn.ModuleList([_conv_layer(*first, k, 1, conv_type)] +
                                 [_conv_layer(*rest, k, 1, conv_type) for _ in range(count - 1)])
        w = nn.Module()
        w.downsampling_blocks = nn.ModuleList()
        w.upsampling_blocks = nn.ModuleList()
        w.film_blocks = nn.ModuleList()
        for i in range(n - 1):
            cin = num_inputs if i == 0 else C[i]
            d = nn.Module()
            d.pre_shortcut_convs = convs((cin, C[i]), (C[i], C[i]), depth)
            d.post_shortcut_convs = convs((C[i], C[i + 1]), (C[i + 1], C[i + 1]), depth)
            d.downconv = _conv_layer(C[i + 1], C[i + 1], resample_kernel_size, resample_stride, conv_type,
                                     padding=(resample_kernel_size - resample_stride) // 2)
            w.downsampling_blocks.append(d)
            w.film_blocks.append(_film(C[i]))
        for i in range(n - 1, 0, -1):
            u = nn.Module()
            u.upconv = _conv_layer(C[i], C[i], resample_kernel_size, resample_stride, conv_type, transpose=True)
            u.pre_shortcut_convs = convs((C[i], C[i - 1]), (C[i - 1], C[i - 1]), depth)
            u.post_shortcut_convs = nn.ModuleList([_conv_layer(C[i - 1], C[i - 1], k, 1, conv_type) for _ in range(depth)])
            w.upsampling_blocks.append(u)
        w.bottlenecks = nn.ModuleList([_conv_layer(C[-1], C[-1], k, 1, conv_type) for _ in range(depth)])
        w.output_conv = nn.Conv1d(C[0], 1, 1)
        self.waveunet = w
        # check_output_size (waveunet.py:401-426) without its prints: every level halves the length
        # exactly (floor((L + 2 - 4 + 2) / 2) = L / 2 needs an even L) and doubles it on the way up
        if input_size >= 0 and (input_size < 2 ** (n - 1) or input_size % 2 ** (n - 1)):
            raise AssertionError(f"input_size {input_size} is not a positive multiple of {2 ** (n - 1)}")
        self.num_samples = -1
        self.compute_dtype = "float32"
        self._ctx = None
        self._ctx_key = None

    def library_config(self):
        return {"arch": {"type": "SDDM", "args": {}},
                "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 1}},
                "network": {"type": "Waveunet", "args": self.config_args}, "num_samples": -1}

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
        """x (condition) and y_t [B, 1, N], N a positive multiple of 2048; noise_level [B] or [B, 1, 1]
        -> clamp(output_conv(...), -1, 1) [B, 1, N] (waveunet.py:475-506, eval mode)."""
        if not y_t.is_cuda:
            raise RuntimeError("Waveunet runs on the HIP device; move the tensors to cuda")
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
