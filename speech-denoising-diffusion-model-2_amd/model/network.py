"""Network registry resolved by ConfigParser.init_obj('network', module_network, ...)
(reference model/network.py).  The denoisers on the north-star path: UNetModified2, DiffWave,
WaveGrad and the waveform-conditioned DenoiseWaveGrad1 / DenoiseWaveGrad3 (the reference's
DenoiseWaveGrad2 has 4 / 8 / 16-channel levels the MFMA convolution cannot take: not built), and
the 1-D Wave-U-Nets Waveunet2 (FiLM-conditioned, 24 / 48 / 72 / 96 channels: its own MFMA convolution
for channel counts that are multiples of 8), Waveunet (the twelve-level original, 24 ... 288 channels:
the same convolution with the output channels split over the grid) and Waveunet3, at the arguments of
config_waveunet2.json, config_waveunet.json and config_waveunet3.json.  UNetTST (config_unettst.json) is
UNetModified2 with the dual-path transformer block Dual_Transformer (multi-head attention and a
bidirectional GRU along the rows, then along the columns of the bottom level) in place of ``mid``; the
block is also a module of its own.  CAUNet (config_caunet.json) is a causal dense-block U-Net over the
frames (dilated (2,3) convs with LayerNorm over the frame and PReLU, a strided downsample and a sub-pixel
upsample) around the same block at d_model 32 (``model.CAUNet.Dual_Transformer``: per-channel PReLUs, any
number of frames).  TSTNN (config_tstnn.json) frames at 512 / 256: a depth-4 dense block at the frame
width, a strided conv to half of it, the block again (``model.tstnn.Dual_Transformer``: single-slope
PReLUs, the output PReLU before its conv, four layers over 63 frames of 256 positions), a gated mask
(tanh x sigmoid -> conv -> ReLU) on the encoder's output, a second dense block and a sub-pixel conv back;
it ignores the noise level.  UNetModified (config_unetmodified.json) is the SR3-style U-Net UNetModified2
was derived from: spatial self-attention (``model.UNetModified.SelfAttention``: GroupNorm, 1x1 qkv conv,
one-head softmax attention over all positions of the level, 1x1 out conv, residual; also a module of its
own) behind the ResnetBlocks of the levels in ``attn_layer`` and behind the first ``mid`` block, no
Downsample after the last level and ``res_blocks + 1`` decoder blocks per level.  The reference's
SNR-estimator networks are not built."""
from .CAUNet import CAUNet  # noqa: F401
from .tstnn import TSTNN  # noqa: F401
from .UNetModified import SelfAttention, UNetModified  # noqa: F401
from .UNetModified2 import UNetModified2  # noqa: F401
from .UNetTST import Dual_Transformer, UNetTST  # noqa: F401
from .diffwave import DiffWave  # noqa: F401
from .wavegrad import DenoiseWaveGrad1, DenoiseWaveGrad3, WaveGrad  # noqa: F401
from .waveunet import Waveunet, Waveunet2  # noqa: F401
from .waveunet3 import Waveunet3  # noqa: F401
