"""What every network facade repeats: the library configuration, the cached libsddm_hip context and
the two forward prologues of the waveform-conditioned denoisers.

A facade's module tree only holds parameters; its forward hands them to the library.  The context
is rebuilt whenever the device, ``compute_dtype`` or any tensor of ``library_params()`` changes
(another storage, or an in-place write: ``_version``).
"""
import torch
from torch import nn

import sddm_hip


class Facade(nn.Module):
    network_type = None                  # the library's name of the network: the class name unless set
    arch = ("SDDM", {})                  # (type, args) of the sampler the context is configured with

    def _init_facade(self, config_args, num_samples=-1):
        self.config_args = config_args
        self.num_samples = num_samples
        self.compute_dtype = "float32"
        self._ctx = None
        self._ctx_key = None

    def library_params(self):
        """The tensors the library loads, under the library's keys."""
        return dict(self.state_dict())

    def library_config(self):
        arch_type, arch_args = self.arch
        return {"arch": {"type": arch_type, "args": arch_args},
                "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 1}},
                "network": {"type": self.network_type or type(self).__name__, "args": self.config_args},
                "num_samples": self.num_samples}

    def _context(self, device):
        sd = self.library_params()
        key = (device.index or 0, self.compute_dtype) + tuple((k, v.data_ptr(), v._version) for k, v in sd.items())
        if self._ctx is None or self._ctx_key != key:
            ctx = sddm_hip.Context(self.library_config(), device.index or 0, self.compute_dtype)
            ctx.load_state_dict(sd)
            self._ctx, self._ctx_key = ctx, key
        return self._ctx


class StrictFacade(Facade):
    """forward for the 1-D networks: the sizes must agree, one noise level per clip."""

    @torch.no_grad()
    def forward(self, x, y_t, noise_level):
        """x (condition) and y_t [B, 1, N], N a positive multiple of hop_samples; noise_level with B
        elements (any shape) -> [B, 1, N]."""
        if not y_t.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the HIP device; move the tensors to cuda")
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


class LenientFacade(Facade):
    """forward for the framed U-Nets: the tensors go to the library as they are, a single noise
    level serves the whole batch."""

    @torch.no_grad()
    def forward(self, x, y_t, noise_level):
        """x: condition [B,1,T], y_t: [B,1,T], noise_level: [B,1,1] -> eps [B,1,T]."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the HIP device; move inputs to cuda")
        x = x.contiguous().float()
        y_t = y_t.contiguous().float()
        nl = noise_level.reshape(-1).contiguous().float()
        if nl.numel() == 1 and x.shape[0] > 1:
            nl = nl.expand(x.shape[0]).contiguous()
        out = torch.empty_like(y_t)
        self._context(x.device).network_forward(x, y_t, nl, out)
        return out


class DualTransformerFacade(Facade):
    """forward and load of a Dual_Transformer run alone: a context of its network is configured around
    the block (the subclass's library_config) and only its ``mid.*`` parameters get loaded."""

    def library_params(self):
        return {"mid." + k: v for k, v in self.state_dict().items()}

    @torch.no_grad()
    def forward(self, input):
        """input [b, c, dim2, dim1] -> [b, c, dim2, dim1]."""
        if not input.is_cuda:
            raise RuntimeError("Dual_Transformer runs on the HIP device; move the input to cuda")
        x = input.contiguous().float()
        if x.dim() != 4 or x.shape[1] != self.input_size:
            raise AssertionError(f"Dual_Transformer expects [b, {self.input_size}, dim2, dim1], got {tuple(x.shape)}")
        out = torch.empty((x.shape[0], self.output_size) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
        self._context(x.device).dual_transformer(x, out)
        return out
