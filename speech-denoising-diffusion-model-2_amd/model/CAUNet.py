"""CAUNet facade (reference model/CAUNet.py:307-374): a causal dense-block U-Net over the 128 / 64
frames of (condition, y_t) with a Dual_Transformer (CAUNet.py:152-201) at d_model 32 as ``mid``.

As in UNetTST.py, the module tree only *holds parameters*, laid out so that ``state_dict()`` has the
reference's keys and shapes (450 tensors at config_caunet.json) and a reference checkpoint loads
unchanged; ``nn.Conv2d``, ``nn.LayerNorm``, ``nn.PReLU``, ``nn.GRU`` and ``nn.MultiheadAttention``
serve as holders.  ``forward`` never computes in torch: ``CAUNet.forward`` runs the whole denoiser in
libsddm_hip and ``Dual_Transformer.forward`` runs the block alone (sddm_dual_transformer).
"""
from torch import nn

from ._facade import DualTransformerFacade, LenientFacade
from .UNetModified2 import PositionalEncoding, SignalToFrames
from .UNetTST import TransformerEncoderLayer

# the arguments the HIP kernels are built for (sddm_configure refuses anything else by name as well)
_FIXED = {"inner_channel": 64, "n_encode_layers": 4, "dense_depth": 3, "segment_len": 128, "segment_stride": 64}


class FeatureWiseAffine(nn.Module):
    """Linear 64 -> 256, PReLU(256), Linear 256 -> 64 (128: gamma | beta) of the noise encoding (CAUNet.py:60-79)."""

    def __init__(self, noise_level_channels, out_channels, use_affine_level=False):
        super().__init__()
        self.use_affine_level = use_affine_level
        n = noise_level_channels * 4
        self.noise_func = nn.Sequential(nn.Linear(noise_level_channels, n), nn.PReLU(n),
                                        nn.Linear(n, out_channels * (1 + self.use_affine_level)))


class Dual_Transformer(DualTransformerFacade):
    """Conv1x1 + PReLU(input_size / 2), num_layers x (row encoder, GroupNorm, residual, column encoder,
    GroupNorm, residual), Conv1x1 + PReLU(output_size) (CAUNet.py:152-201).  The HIP kernels are built
    for input_size = output_size = 64; dim2 and dim1 are free."""

    network_type = "CAUNet"

    def __init__(self, input_size, output_size, dropout=0, num_layers=1):
        super().__init__()
        self._init_facade({"n_TSTB": num_layers}, 704)
        self.input_size, self.output_size, self.num_layers = input_size, output_size, num_layers
        d = input_size // 2
        self.input = nn.Sequential(nn.Conv2d(input_size, d, kernel_size=1), nn.PReLU(d))
        self.row_trans = nn.ModuleList([])
        self.col_trans = nn.ModuleList([])
        self.row_norm = nn.ModuleList([])
        self.col_norm = nn.ModuleList([])
        for _ in range(num_layers):
            self.row_trans.append(TransformerEncoderLayer(d_model=d, nhead=4, dropout=dropout, bidirectional=True))
            self.col_trans.append(TransformerEncoderLayer(d_model=d, nhead=4, dropout=dropout, bidirectional=True))
            self.row_norm.append(nn.GroupNorm(1, d, eps=1e-8))
            self.col_norm.append(nn.GroupNorm(1, d, eps=1e-8))
        self.output = nn.Sequential(nn.Conv2d(d, output_size, 1), nn.PReLU(output_size))

    def library_config(self):
        """A CAUNet context around this block (only its mid.* parameters get loaded)."""
        if self.input_size != 64 or self.output_size != 64:
            raise NotImplementedError(f"CAUNet Dual_Transformer on HIP: input_size / output_size 64, got "
                                      f"{self.input_size} / {self.output_size}")
        if self.num_layers < 1:
            raise NotImplementedError(f"CAUNet Dual_Transformer on HIP: num_layers {self.num_layers} (at least 1)")
        return super().library_config()


class SPConvTranspose2d(nn.Module):
    """Sub-pixel upsampling along the frame: a (1,3) conv to out_channels * r (CAUNet.py:204-219)."""

    def __init__(self, in_channels, out_channels, kernel_size, r=1):
        super().__init__()
        self.out_channels, self.r = out_channels, r
        self.conv = nn.Conv2d(in_channels, out_channels * r, kernel_size=kernel_size, stride=(1, 1), padding=(0, 1))


class DenseBlock(nn.Module):
    """depth x ((2,3) conv with frame dilation 2^i over the concatenation so far, LayerNorm over the
    frame, PReLU) (CAUNet.py:222-249)."""

    def __init__(self, input_size, depth=5, in_channels=64):
        super().__init__()
        self.depth, self.in_channels = depth, in_channels
        for i in range(depth):
            setattr(self, f"conv{i + 1}", nn.Conv2d(in_channels * (i + 1), in_channels, kernel_size=(2, 3), dilation=(2 ** i, 1)))
            setattr(self, f"norm{i + 1}", nn.LayerNorm(input_size))
            setattr(self, f"prelu{i + 1}", nn.PReLU(in_channels))


class EncodeLayer(nn.Module):
    def __init__(self, n_in_channels, frame_length, n_out_channels, noise_level_channels, depth=5, use_affine_level=False):
        super().__init__()
        self.dense = DenseBlock(frame_length, depth, n_in_channels)
        self.noise_func = FeatureWiseAffine(noise_level_channels, n_in_channels, use_affine_level)
        self.downsample = nn.Sequential(nn.Conv2d(n_in_channels, n_out_channels, (1, 3), (1, 2), (0, 1)),
                                        nn.LayerNorm(frame_length // 2), nn.PReLU(n_out_channels))


class DecodeLayer(nn.Module):
    def __init__(self, n_in_channels, frame_length, n_out_channels, noise_level_channels, depth=5, use_affine_level=False):
        super().__init__()
        self.dense = DenseBlock(frame_length, depth, n_in_channels)
        self.noise_func = FeatureWiseAffine(noise_level_channels, n_in_channels, use_affine_level)
        self.upsample = nn.Sequential(SPConvTranspose2d(n_in_channels * 2, n_out_channels, (1, 3), r=2),
                                      nn.LayerNorm(frame_length * 2), nn.PReLU(n_out_channels))


class CAUNet(LenientFacade):
    """forward(x, y_t, noise_level): the noise level is a vector of B entries (the reference's squeeze()
    breaks at B = 1)."""

    def __init__(self, num_samples, inner_channel=64, n_encode_layers=4, dense_depth=3, n_TSTB=6, segment_len=128,
                 segment_stride=64, use_affine_level=False):
        super().__init__()
        given = {"inner_channel": inner_channel, "n_encode_layers": n_encode_layers, "dense_depth": dense_depth,
                 "segment_len": segment_len, "segment_stride": segment_stride}
        for k, want in _FIXED.items():
            if given[k] != want:
                raise NotImplementedError(f"CAUNet on HIP: {k} {want}, got {given[k]}")
        if not isinstance(n_TSTB, int) or n_TSTB < 1:
            raise NotImplementedError(f"CAUNet on HIP: n_TSTB at least 1, got {n_TSTB}")
        if not isinstance(use_affine_level, bool):
            raise NotImplementedError(f"CAUNet on HIP: use_affine_level false or true, got {use_affine_level!r}")
        self._init_facade(dict(given, n_TSTB=n_TSTB, use_affine_level=use_affine_level), num_samples)
        self.noise_encoding = PositionalEncoding(inner_channel)
        self.segment = SignalToFrames(num_samples, segment_len, segment_stride)          # asserts (num_samples - 128) % 64 == 0
        self.first_conv = nn.Conv2d(2, inner_channel, kernel_size=(1, 1), stride=(1, 1))
        self.downs = nn.ModuleList([])
        length = segment_len
        for _ in range(n_encode_layers):
            self.downs.append(EncodeLayer(inner_channel, length, inner_channel, inner_channel, dense_depth, use_affine_level))
            length //= 2
        self.mid = Dual_Transformer(inner_channel, inner_channel, 0, n_TSTB)
        self.ups = nn.ModuleList([])
        for _ in range(n_encode_layers):
            self.ups.append(DecodeLayer(inner_channel, length, inner_channel, inner_channel, dense_depth, use_affine_level))
            length *= 2
        self.final_conv = nn.Conv2d(inner_channel, 1, kernel_size=(1, 1))
