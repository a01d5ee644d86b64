"""Test infrastructure: the numpy DiffWave oracle with the 16-bit kernels' storage roundings.

``Emul(params, dtype)(spec, audio, steps)`` is ``oracle.diffwave.forward`` assembled from the
oracle's public pieces (upsample, conv1x1, dilated_conv, embedding), with every value that the HIP
path keeps in the 16-bit compute type rounded through ``torch.bfloat16`` / ``torch.float16`` where
the kernels store it (csrc/diffwave.hip):

  the upsampled spectrogram (dw_upsample2_kernel), the conditioner rows (dw_cond_kernel),
  x after the input projection and after every layer's epilogue, y = x + diffusion projection (the
  staged tap images), the gated activation z, and the 16-bit weights: dilated_conv,
  conditioner_projection, output_residual and the per-layer output_projection.

Accumulation, biases, the diffusion embedding / projection, the skip sum and the output head stay
fp32, as in the kernels.  ``dtype=None`` rounds nothing and returns exactly the oracle's forward.
The step-invariant conditioner (all layers) is cached per spectrogram, so a sampling loop pays it
once.  What the emulation does not restate is the order of the fp32 sums inside the MFMA GEMMs and
the kernels' exp2 / rcp gate activations: those are the GPU's own fp32 noise on top.
"""
import numpy as np
import torch

from oracle import diffwave as odw

f32 = np.float32
_TORCH = {"bfloat16": torch.bfloat16, "float16": torch.float16}
_ROUNDED_WEIGHTS = ("dilated_conv.weight", "conditioner_projection.weight", "output_residual.weight",
                    "output_projection.weight")


class Emul:
    def __init__(self, params, dtype=None, residual_layers=30, cycle=10):
        if dtype is not None and dtype not in _TORCH:
            raise ValueError(f"dtype {dtype!r}: None, 'bfloat16' or 'float16'")
        self.dtype, self.L, self.cycle = dtype, residual_layers, cycle
        self.P = dict(params)
        for i in range(residual_layers):
            for k in _ROUNDED_WEIGHTS:
                name = f"residual_layers.{i}.{k}"
                self.P[name] = self.q(self.P[name])
        self._spec = None
        self._cond = None

    def q(self, a):
        """Round to the storage type and back (identity for dtype None)."""
        if self.dtype is None:
            return a
        a = np.ascontiguousarray(a, dtype=np.float32)
        # one thread: an elementwise cast gains nothing from torch's pool, and waking the pool between
        # numpy's BLAS calls costs far more than the cast
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return torch.from_numpy(a).to(_TORCH[self.dtype]).to(torch.float32).numpy()
        finally:
            torch.set_num_threads(n)

    def conditioner(self, spec):
        """Every layer's conditioner_projection of the upsampled spectrogram, cached per spec."""
        if self._spec is None or self._spec.shape != spec.shape or not np.array_equal(self._spec, spec):
            P = self.P
            up = self.q(odw.upsample(P, spec.astype(np.float32)))
            self._cond = [self.q(odw.conv1x1(up, P[f"residual_layers.{i}.conditioner_projection.weight"],
                                             P[f"residual_layers.{i}.conditioner_projection.bias"]))
                          for i in range(self.L)]
            self._spec = spec.copy()
        return self._cond

    def __call__(self, spec, audio, steps):
        P, q = self.P, self.q
        x = q(np.maximum(odw.conv1x1(audio.astype(np.float32), P["input_projection.weight"], P["input_projection.bias"]), 0))
        emb = odw.embedding(P, steps)
        conds = self.conditioner(spec)
        skip = None
        for i in range(self.L):
            p = f"residual_layers.{i}."
            ds = (emb @ P[p + "diffusion_projection.weight"].T + P[p + "diffusion_projection.bias"]).astype(np.float32)
            y = q((x + ds[:, :, None]).astype(np.float32))
            y = odw.dilated_conv(y, P[p + "dilated_conv.weight"], P[p + "dilated_conv.bias"], 2 ** (i % self.cycle)) + conds[i]
            C = y.shape[1] // 2
            gate, filt = y[:, :C], y[:, C:]
            y = q(((f32(1.0) / (f32(1.0) + np.exp(-gate))) * np.tanh(filt)).astype(np.float32))
            res = odw.conv1x1(y, P[p + "output_residual.weight"], P[p + "output_residual.bias"])
            sk = odw.conv1x1(y, P[p + "output_projection.weight"], P[p + "output_projection.bias"])
            x = q(((x + res) / f32(np.sqrt(2.0))).astype(np.float32))
            skip = sk if skip is None else (skip + sk).astype(np.float32)
        x = (skip / f32(np.sqrt(self.L))).astype(np.float32)
        x = np.maximum(odw.conv1x1(x, P["skip_projection.weight"], P["skip_projection.bias"]), 0)
        return odw.conv1x1(x, P["output_projection.weight"], P["output_projection.bias"])
