"""UNetTST facade (reference model/UNetTST.py:270-392): UNetModified2 whose ``mid`` is a
Dual_Transformer (UNetTST.py:184-233) and whose noise MLP has no final Swish.

As in UNetModified2.py, the module tree only *holds parameters*, laid out so that ``state_dict()``
has the reference's keys and shapes (454 tensors at config_unettst.json) and a reference checkpoint
loads unchanged; ``nn.MultiheadAttention``, ``nn.GRU``, ``nn.LayerNorm``, ``nn.GroupNorm`` and
``nn.PReLU`` serve as holders.  ``forward`` never computes in torch: ``UNetTST.forward`` runs the whole
denoiser in libsddm_hip and ``Dual_Transformer.forward`` runs the block alone (sddm_dual_transformer).
"""
from torch import nn

from ._facade import DualTransformerFacade, LenientFacade
from .UNetModified2 import (Block, Downsample, PositionalEncoding, ResnetBlock, SignalToFrames, Swish,  # noqa: F401
                            Upsample)


class TransformerEncoderLayer(nn.Module):
    """Self-attention, residual, LayerNorm, bidirectional GRU, ReLU, Linear, residual, LayerNorm
    (UNetTST.py:113-181)."""

    def __init__(self, d_model, nhead, bidirectional=True, dropout=0, activation="relu"):
        super().__init__()
        if not bidirectional or activation != "relu":
            raise NotImplementedError("TransformerEncoderLayer on HIP: bidirectional=True, activation='relu' "
                                      "(the only values Dual_Transformer passes, UNetTST.py:201-202)")
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout)
        self.gru = nn.GRU(d_model, d_model * 2, 1, bidirectional=True)
        self.dropout = nn.Dropout(dropout)
        self.linear2 = nn.Linear(d_model * 2 * 2, d_model)
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout1 = nn.Dropout(dropout)
        self.dropout2 = nn.Dropout(dropout)


class Dual_Transformer(DualTransformerFacade):
    """Conv1x1 + PReLU, num_layers x (row encoder, GroupNorm, residual, column encoder, GroupNorm,
    residual), Conv1x1 + PReLU (UNetTST.py:184-233).  The HIP kernel is built for input_size =
    output_size = 160 and at most 64 positions (dim2 * dim1)."""

    network_type = "UNetTST"

    def __init__(self, input_size, output_size, dropout=0, num_layers=1):
        super().__init__()
        self._init_facade({"res_blocks": 1, "n_TSTB": num_layers}, 2112)
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
        self.output = nn.Sequential(nn.Conv2d(d, output_size, 1), nn.PReLU())

    def library_config(self):
        """A UNetTST context around this block (only its mid.* parameters get loaded)."""
        if self.input_size != 160 or self.output_size != 160:
            raise NotImplementedError(f"Dual_Transformer on HIP: input_size / output_size 160, got "
                                      f"{self.input_size} / {self.output_size}")
        return super().library_config()


class UNetTST(LenientFacade):
    def __init__(self, num_samples, in_channel=2, out_channel=1, inner_channel=32, norm_groups=32,
                 channel_mults=(1, 2, 3, 4, 5), n_TSTB=6, res_blocks=3, dropout=0, segment_len=128, segment_stride=64):
        super().__init__()
        self._init_facade({"in_channel": in_channel, "out_channel": out_channel, "inner_channel": inner_channel,
                           "norm_groups": norm_groups, "channel_mults": list(channel_mults), "n_TSTB": n_TSTB,
                           "res_blocks": res_blocks, "dropout": dropout, "segment_len": segment_len,
                           "segment_stride": segment_stride}, num_samples)
        self.segment = SignalToFrames(num_samples, segment_len, segment_stride)
        E = inner_channel
        self.noise_level_mlp = nn.Sequential(PositionalEncoding(E), nn.Linear(E, E * 4), Swish(),
                                             nn.Linear(E * 4, E))                 # UNetTST.py:293-298
        rb = dict(noise_level_emb_dim=E, norm_groups=norm_groups, dropout=dropout)
        downs = [nn.Conv2d(in_channel, E, kernel_size=3, padding=1)]
        skip = [E]
        cin = E
        for mult in channel_mults:                                   # encoder (UNetTST.py:310-322)
            cout = E * mult
            for _ in range(res_blocks):
                downs.append(ResnetBlock(cin, cout, **rb))
                skip.append(cout)
                cin = cout
            downs.append(Downsample(cout))
            skip.append(cout)
        self.downs = nn.ModuleList(downs)
        self.mid = Dual_Transformer(cout, cout, 0, n_TSTB)            # UNetTST.py:324
        ups = []
        for ind in reversed(range(len(channel_mults))):               # decoder (UNetTST.py:330-354)
            cin = E * channel_mults[ind]
            ups.append(ResnetBlock(cin + skip.pop(), cin, **rb))
            ups.append(Upsample(cin))
            cout = E if ind == 0 else E * channel_mults[ind - 1]
            for _ in range(res_blocks):
                ups.append(ResnetBlock(cin + skip.pop(), cout, **rb))
                cin = cout
        self.ups = nn.ModuleList(ups)
        self.final_conv = Block(cout, out_channel, groups=norm_groups)
