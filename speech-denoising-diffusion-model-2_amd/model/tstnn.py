"""TSTNN facade (reference model/tstnn.py:216-299): the two-stage transformer denoiser over the
512 / 256 frames of (condition, y_t) -- a depth-4 dense block at frame width 512, a strided conv to
width 256, a Dual_Transformer (tstnn.py:114-164) at d_model 32 with four layers, a gated mask on the
encoder's output, a depth-4 dense block at width 256 and a sub-pixel conv back to 512.

As in CAUNet.py, the module tree only *holds parameters*, laid out so that ``state_dict()`` has the
reference's keys and shapes in the reference's order (229 tensors) and a reference checkpoint loads
unchanged.  ``forward`` never computes in torch: ``TSTNN.forward`` runs the whole denoiser in
libsddm_hip and ``Dual_Transformer.forward`` runs the block alone (sddm_dual_transformer).  The noise
level is accepted and ignored, as in the reference: no parameter depends on it.
"""
from torch import nn

from ._facade import DualTransformerFacade, LenientFacade
from .CAUNet import DenseBlock, SPConvTranspose2d
from .UNetModified2 import SignalToFrames
from .UNetTST import TransformerEncoderLayer

# the arguments the HIP kernels are built for (sddm_configure refuses anything else by name as well)
_FIXED = {"F": 512, "stride": 256, "n_channels": 64}


class Dual_Transformer(DualTransformerFacade):
    """Conv1x1 + PReLU() (one slope), num_layers x (row encoder, GroupNorm, residual, column encoder,
    GroupNorm, residual), PReLU() then Conv1x1 (tstnn.py:114-164).  The HIP kernels are built for
    input_size = output_size = 64; dim2 and dim1 are free."""

    network_type = "TSTNN"

    def __init__(self, input_size, output_size, dropout=0, num_layers=1):
        super().__init__()
        self._init_facade(dict(_FIXED, num_layers=num_layers), 512)
        self.input_size, self.output_size, self.num_layers = input_size, output_size, num_layers
        d = input_size // 2
        self.input = nn.Sequential(nn.Conv2d(input_size, d, kernel_size=1), nn.PReLU())
        self.row_trans = nn.ModuleList([])
        self.col_trans = nn.ModuleList([])
        self.row_norm = nn.ModuleList([])
        self.col_norm = nn.ModuleList([])
        for _ in range(num_layers):
            self.row_trans.append(TransformerEncoderLayer(d_model=d, nhead=4, dropout=dropout, bidirectional=True))
            self.col_trans.append(TransformerEncoderLayer(d_model=d, nhead=4, dropout=dropout, bidirectional=True))
            self.row_norm.append(nn.GroupNorm(1, d, eps=1e-8))
            self.col_norm.append(nn.GroupNorm(1, d, eps=1e-8))
        self.output = nn.Sequential(nn.PReLU(), nn.Conv2d(d, output_size, 1))

    def library_params(self):
        return {"dual_transformer." + k: v for k, v in self.state_dict().items()}

    def library_config(self):
        """A TSTNN context around this block (only its dual_transformer.* parameters get loaded)."""
        if self.input_size != 64 or self.output_size != 64:
            raise NotImplementedError(f"TSTNN Dual_Transformer on HIP: input_size / output_size 64, got "
                                      f"{self.input_size} / {self.output_size}")
        if self.num_layers < 1:
            raise NotImplementedError(f"TSTNN Dual_Transformer on HIP: num_layers {self.num_layers} (at least 1)")
        return super().library_config()


class TSTNN(LenientFacade):
    """forward(x, y_t, noise_level): x and y_t [B, 1, num_samples]; the noise level is not used."""

    def __init__(self, num_samples, F=512, stride=256, n_channels=64):
        super().__init__()
        given = {"F": F, "stride": stride, "n_channels": n_channels}
        for k, want in _FIXED.items():
            if given[k] != want:
                raise NotImplementedError(f"TSTNN on HIP: {k} {want}, got {given[k]}")
        self._init_facade(given, num_samples)
        self.segment = SignalToFrames(num_samples, F, stride)                          # asserts (num_samples - 512) % 256 == 0
        self.inp_conv = nn.Conv2d(2, n_channels, kernel_size=(1, 1))
        self.inp_norm = nn.LayerNorm(F)
        self.inp_prelu = nn.PReLU(n_channels)
        self.enc_dense1 = DenseBlock(F, 4, n_channels)
        self.enc_conv1 = nn.Conv2d(n_channels, n_channels, kernel_size=(1, 3), stride=(1, 2))
        self.enc_norm1 = nn.LayerNorm(F // 2)
        self.enc_prelu1 = nn.PReLU(n_channels)
        self.dual_transformer = Dual_Transformer(n_channels, n_channels, num_layers=4)
        self.output1 = nn.Sequential(nn.Conv2d(n_channels, n_channels, kernel_size=1), nn.Tanh())
        self.output2 = nn.Sequential(nn.Conv2d(n_channels, n_channels, kernel_size=1), nn.Sigmoid())
        self.maskconv = nn.Conv2d(n_channels, n_channels, kernel_size=1)
        self.dec_dense1 = DenseBlock(F // 2, 4, n_channels)
        self.dec_conv1 = SPConvTranspose2d(n_channels, n_channels, kernel_size=(1, 3), r=2)
        self.dec_norm1 = nn.LayerNorm(F)
        self.dec_prelu1 = nn.PReLU(n_channels)
        self.out_conv = nn.Conv2d(n_channels, 1, kernel_size=(1, 1))
