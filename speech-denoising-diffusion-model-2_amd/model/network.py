"""Network registry resolved by ConfigParser.init_obj('network', module_network, ...)
(reference model/network.py).  The denoisers on the north-star path: UNetModified2, DiffWave,
WaveGrad and the waveform-conditioned DenoiseWaveGrad1 / DenoiseWaveGrad3 (the reference's
DenoiseWaveGrad2 has 4 / 8 / 16-channel levels the MFMA convolution cannot take: not built)."""
from .UNetModified2 import UNetModified2  # noqa: F401
from .diffwave import DiffWave  # noqa: F401
from .wavegrad import DenoiseWaveGrad1, DenoiseWaveGrad3, WaveGrad  # noqa: F401
