"""UNetModified facade (reference model/UNetModified.py:192-323): the SR3-style U-Net UNetModified2 was
derived from, with spatial self-attention (UNetModified.py:140-169) behind the ResnetBlocks of the
levels in ``attn_layer`` and behind the first ``mid`` block.

As in UNetModified2.py the module tree only *holds parameters*, laid out so that ``state_dict()`` has the
reference's keys and shapes (242 tensors at config_unetmodified.json) and a reference checkpoint loads
unchanged.  ``forward`` never computes in torch: ``UNetModified.forward`` runs the whole denoiser in
libsddm_hip and ``SelfAttention.forward`` runs one attention block alone (sddm_self_attention).

Against UNetModified2: there is no Downsample after the last level, ``mid`` is (ResnetBlock + attention,
ResnetBlock), every decoder level has ``res_blocks + 1`` blocks over cat(x, skip) followed by its
Upsample (none at level 0), the noise MLP has no final Swish and the positional encoding is
``level * exp(-ln(1e4) * i / (dim / 2))``, sin then cos.
"""
import torch
from torch import nn

from ._facade import Facade, LenientFacade
from .UNetModified2 import Block, Downsample, FeatureWiseAffine, ResnetBlock, SignalToFrames, Swish, Upsample  # noqa: F401


class PositionalEncoding(nn.Module):
    """UNetModified.py:46-59: no parameters and no buffers."""

    def __init__(self, dim):
        super().__init__()
        self.dim = dim


class SelfAttention(Facade):
    """GroupNorm, 1x1 qkv conv without bias, softmax(Q K^T / sqrt(C)) V over all H * W positions with one
    head, 1x1 out conv, + input (UNetModified.py:140-169).  Run alone it owns a one-level UNetModified
    context (channel_mults [C / 32], attn_layer [0]) of which only ``mid.0.attn.*`` is loaded.  The HIP
    kernels take in_channel a multiple of 32 up to 256 and n_head 1 (the only value the network passes)."""

    network_type = "UNetModified"
    layer = "mid.0.attn"

    def __init__(self, in_channel, n_head=1, norm_groups=32):
        super().__init__()
        self.in_channel, self.n_head, self.norm_groups = in_channel, n_head, norm_groups
        self._init_facade({"inner_channel": 32, "norm_groups": norm_groups, "channel_mults": [in_channel // 32],
                           "attn_layer": [0], "res_blocks": 1}, 2112)
        self.norm = nn.GroupNorm(norm_groups, in_channel)
        self.qkv = nn.Conv2d(in_channel, in_channel * 3, 1, bias=False)
        self.out = nn.Conv2d(in_channel, in_channel, 1)

    def library_config(self):
        if self.n_head != 1:
            raise NotImplementedError(f"SelfAttention on HIP: n_head 1 (the only value UNetModified passes), got {self.n_head}")
        if self.in_channel % 32 or not 32 <= self.in_channel <= 256:
            raise NotImplementedError(f"SelfAttention on HIP: in_channel a multiple of 32 up to 256, got {self.in_channel}")
        return super().library_config()

    def library_params(self):
        return {self.layer + "." + k: v for k, v in self.state_dict().items()}

    @torch.no_grad()
    def forward(self, input):
        """input [B, C, H, W] -> [B, C, H, W]."""
        if not input.is_cuda:
            raise RuntimeError("SelfAttention runs on the HIP device; move the input to cuda")
        x = input.contiguous().float()
        if x.dim() != 4 or x.shape[1] != self.in_channel:
            raise AssertionError(f"SelfAttention expects [B, {self.in_channel}, H, W], got {tuple(x.shape)}")
        out = torch.empty_like(x)
        self._context(x.device).self_attention(self.layer, x, out)
        return out


class ResnetBlocWithAttn(nn.Module):
    def __init__(self, dim, dim_out, noise_level_emb_dim=None, norm_groups=32, dropout=0, with_attn=False):
        super().__init__()
        self.with_attn = with_attn
        self.res_block = ResnetBlock(dim, dim_out, noise_level_emb_dim, norm_groups=norm_groups, dropout=dropout)
        if with_attn:
            self.attn = SelfAttention(dim_out, norm_groups=norm_groups)


class UNetModified(LenientFacade):
    def __init__(self, num_samples, in_channel=2, out_channel=1, inner_channel=32, norm_groups=32,
                 channel_mults=(1, 2, 4, 8, 8), attn_layer=(4), res_blocks=3, dropout=0, segment_len=128,
                 segment_stride=64, with_noise_level_emb=True):
        super().__init__()
        if not with_noise_level_emb:
            # the reference builds nn.Linear(None, ...) in every FeatureWiseAffine and dies there (UNetModified.py:67)
            raise TypeError("UNetModified: with_noise_level_emb=False is refused as in the reference, whose "
                            "FeatureWiseAffine builds nn.Linear(None, ...)")
        if isinstance(attn_layer, int):
            # `ind in attn_layer` (UNetModified.py:238); the class default (4) is an int, not a tuple
            raise TypeError("argument of type 'int' is not iterable: attn_layer must be a list of levels")
        attn_layer = list(attn_layer)
        self._init_facade({"in_channel": in_channel, "out_channel": out_channel, "inner_channel": inner_channel,
                           "norm_groups": norm_groups, "channel_mults": list(channel_mults), "attn_layer": attn_layer,
                           "res_blocks": res_blocks, "dropout": dropout, "segment_len": segment_len,
                           "segment_stride": segment_stride}, num_samples)
        self.segment = SignalToFrames(num_samples, segment_len, segment_stride)
        E = inner_channel
        self.noise_level_mlp = nn.Sequential(PositionalEncoding(E), nn.Linear(E, E * 4), Swish(),
                                             nn.Linear(E * 4, E))                 # UNetModified.py:212-217
        rb = dict(noise_level_emb_dim=E, norm_groups=norm_groups, dropout=dropout)
        n = len(channel_mults)
        downs = [nn.Conv2d(in_channel, E, kernel_size=3, padding=1)]
        skip = [E]
        cin = E
        for ind in range(n):                                          # encoder (UNetModified.py:237-252)
            cout = E * channel_mults[ind]
            for _ in range(res_blocks):
                downs.append(ResnetBlocWithAttn(cin, cout, with_attn=ind in attn_layer, **rb))
                skip.append(cout)
                cin = cout
            if ind != n - 1:
                downs.append(Downsample(cin))
                skip.append(cin)
        self.downs = nn.ModuleList(downs)
        self.mid = nn.ModuleList([ResnetBlocWithAttn(cin, cin, with_attn=True, **rb),
                                  ResnetBlocWithAttn(cin, cin, with_attn=False, **rb)])
        ups = []
        for ind in reversed(range(n)):                                # decoder (UNetModified.py:262-274)
            cout = E * channel_mults[ind]
            for _ in range(res_blocks + 1):
                ups.append(ResnetBlocWithAttn(cin + skip.pop(), cout, with_attn=ind in attn_layer, **rb))
                cin = cout
            if ind >= 1:
                ups.append(Upsample(cin))
        self.ups = nn.ModuleList(ups)
        self.final_conv = Block(cin, out_channel, groups=norm_groups)
