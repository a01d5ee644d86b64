"""ctypes binding of libsddm_hip.so (C ABI: include/sddm_hip.h).

This is the only way the Python facade reaches the hot path.  There is no CPU or torch
fallback: if the library is missing, or no HIP device is visible, calls raise.
"""
import ctypes
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SDDM_LIB") or os.path.join(HERE, "libsddm_hip.so")   # SDDM_LIB: profiling variants

OK, ERR_NOT_IMPLEMENTED, ERR_INVALID_ARG, ERR_SHAPE, ERR_HIP, ERR_STATE = range(6)
F32, BF16, F16 = 0, 1, 2
TR_ORIGINAL, TR_SR3, TR_SUPPORTIVE, TR_CONDITIONAL, TR_CONDITION_IN = range(5)
DTYPES = {"float32": F32, "fp32": F32, "f32": F32, "bfloat16": BF16, "bf16": BF16,
          "float16": F16, "fp16": F16, "f16": F16}
TRANSITIONS = {"original": TR_ORIGINAL, "condition_in": TR_CONDITION_IN, "sr3": TR_SR3,
               "supportive": TR_SUPPORTIVE, "conditional": TR_CONDITIONAL}
TABLE_NAMES = ("betas", "alphas", "alpha_bar", "sqrt_alpha_bar", "predicted_noise_coeff", "sigma",
               "supportive_gamma", "supportive_sigma_hat", "m", "sqrt_delta", "c_xt", "c_yt", "c_epst",
               "sqrt_delta_estimated")
EXPORTS = ("sddm_abi_version", "sddm_last_error", "sddm_create", "sddm_destroy", "sddm_configure",
           "sddm_load_param", "sddm_missing_params", "sddm_sample", "sddm_sample_noise", "sddm_sample_continuous",
           "sddm_network_forward", "sddm_dual_transformer", "sddm_self_attention",
           "sddm_transition", "sddm_q_sample", "sddm_log_spectrogram", "sddm_set_conv_tuning", "sddm_initial_state", "sddm_schedule", "sddm_unet_plan", "sddm_profile_enable",
           "sddm_profile_read", "sddm_profile_ops")

_lib = None


def lib():
    """Load libsddm_hip.so (fails loudly when it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} not built: run __graft_entry__.build() or "
                               "python speech-denoising-diffusion-model-2_amd/sddm_hip/build.py")
        L = ctypes.CDLL(LIB_PATH)
        vp, i64, u64, c_int = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64, ctypes.c_int
        L.sddm_abi_version.restype = c_int
        L.sddm_last_error.restype = ctypes.c_char_p
        L.sddm_create.argtypes = [c_int, c_int, ctypes.POINTER(vp)]
        L.sddm_destroy.argtypes = [vp]
        L.sddm_destroy.restype = None
        L.sddm_configure.argtypes = [vp, ctypes.c_char_p]
        L.sddm_load_param.argtypes = [vp, ctypes.c_char_p, vp, ctypes.POINTER(i64), c_int, c_int]
        L.sddm_missing_params.argtypes = [vp, ctypes.POINTER(i64)]
        L.sddm_sample.argtypes = [vp, vp, i64, i64, u64, i64, vp, vp]
        L.sddm_sample_noise.argtypes = [vp, vp, i64, i64, vp, vp, vp]
        L.sddm_sample_continuous.argtypes = [vp, vp, i64, i64, u64, i64, vp, vp, c_int, vp]
        L.sddm_network_forward.argtypes = [vp, vp, vp, vp, i64, i64, vp, vp]
        L.sddm_dual_transformer.argtypes = [vp, vp, i64, i64, i64, vp, vp]
        L.sddm_self_attention.argtypes = [vp, ctypes.c_char_p, vp, i64, i64, i64, vp, vp]
        L.sddm_transition.argtypes = [vp, c_int, vp, vp, vp, c_int, i64, i64, u64, i64, vp, vp]
        L.sddm_q_sample.argtypes = [vp, c_int, vp, vp, vp, vp, vp, i64, i64, vp, vp, vp, vp, vp]
        L.sddm_log_spectrogram.argtypes = [vp, i64, i64, c_int, c_int, vp, vp, c_int, vp, vp]
        L.sddm_set_conv_tuning.argtypes = [vp, ctypes.c_char_p]
        L.sddm_initial_state.argtypes = [vp, c_int, vp, i64, i64, u64, i64, vp, vp]
        L.sddm_schedule.argtypes = [ctypes.c_char_p, c_int, ctypes.c_double, ctypes.c_double, vp]
        L.sddm_unet_plan.argtypes = [ctypes.c_char_p, ctypes.c_char_p, c_int, ctypes.c_char_p, i64]
        L.sddm_profile_enable.argtypes = [vp, c_int]
        L.sddm_profile_read.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(i64), ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double)]
        L.sddm_profile_ops.argtypes = [vp, ctypes.c_char_p, i64]
        for name in EXPORTS:
            if name not in ("sddm_last_error", "sddm_destroy", "sddm_abi_version"):
                getattr(L, name).restype = c_int
        _lib = L
    return _lib


class SddmError(RuntimeError):
    pass


def check(status):
    """Map a status code to the exception type the reference raises for the same condition."""
    if status == OK:
        return
    msg = lib().sddm_last_error().decode(errors="replace")
    if status == ERR_NOT_IMPLEMENTED:
        raise NotImplementedError(msg)
    if status == ERR_SHAPE:
        raise AssertionError(msg)
    if status == ERR_INVALID_ARG:
        raise ValueError(msg)
    raise SddmError(f"sddm status {status}: {msg}")


def schedule(schedule="linear", n_timestep=1000, linear_start=1e-4, linear_end=2e-2):
    """The 14 GaussianDiffusion buffers (host computation in the library, no GPU needed)."""
    out = np.empty((14, int(n_timestep) + 1), dtype=np.float32)
    check(lib().sddm_schedule(str(schedule).encode(), int(n_timestep), float(linear_start),
                              float(linear_end), out.ctypes.data))
    return dict(zip(TABLE_NAMES, out))


def unet_plan(cfg, tuning_text=None, dtype="bfloat16"):
    """The plan of one UNetModified2 / UNetTST / UNetModified step (host computation in the library, no GPU needed):
    a list with one dict per step in launch order; conv steps carry the kernel family, the geometry
    and the kernel choice (sddm_unet_plan).  cfg: a config dict as Context takes it (its "network",
    "num_samples" and "lane_rows" are read); tuning_text: the text of a tuning file, or None."""
    buf = ctypes.create_string_buffer(1 << 20)
    check(lib().sddm_unet_plan(json.dumps(cfg).encode(), None if tuning_text is None else tuning_text.encode(),
                               DTYPES[str(dtype)], buf, len(buf)))
    return json.loads(buf.value.decode())


def planned_kernel(step):
    """A conv step of unet_plan in the tuning table's vocabulary: "strip" | "tile:<cfg>" |
    "deep:<mt>:<nw>:<nb>" | "chain"; "wide:<pixels>" is the K-chunked kernel of the layers none of those
    holds (no table can ask for it)."""
    k = step["kernel"]
    return {"tile": f"tile:{step['tile']}", "deep": f"deep:{step['mt']}:{step['nw']}:{step['nb']}",
            "wide": f"wide:{step['mt']}"}.get(k, k)


def _ptr(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def _stream(torch, device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class Context:
    """One configured sampler on one HIP device (owns weights, tables, workspace)."""

    def __init__(self, config, device=0, compute_dtype="float32"):
        self.device = int(device)
        self.dtype = DTYPES[str(compute_dtype)]
        h = ctypes.c_void_p()
        check(lib().sddm_create(self.device, self.dtype, ctypes.byref(h)))
        self._h = h
        check(lib().sddm_configure(self._h, json.dumps(config).encode()))
        # the library's own default when the schedule names no n_timestep (sddm_configure: 1000), so
        # sample_noise always checks the T + 1 draws it reads
        self.timesteps = int(config.get("diffusion", {}).get("args", {}).get("n_timestep", 1000))

    def close(self):
        if getattr(self, "_h", None):
            lib().sddm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_param(self, key, array):
        a = np.ascontiguousarray(np.asarray(array, dtype=np.float32))
        shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
        check(lib().sddm_load_param(self._h, key.encode(), a.ctypes.data, shape, a.ndim, F32))

    def load_state_dict(self, state):
        for k, v in state.items():
            if hasattr(v, "detach"):
                v = v.detach().float().cpu().numpy()
            self.load_param(k, v)

    def missing(self):
        n = ctypes.c_int64()
        check(lib().sddm_missing_params(self._h, ctypes.byref(n)))
        return n.value

    # the torch tensors below are device tensors (fp32, contiguous) on self.device
    def sample(self, cond, out, seed, row_offset=0):
        import torch
        B, N = out.shape[0], out.shape[-1]          # spectrogram archs: cond is [B, bins, frames]
        check(lib().sddm_sample(self._h, _ptr(cond), B, N, int(seed) & (2 ** 64 - 1), int(row_offset),
                                _ptr(out), _stream(torch, cond.device)))

    def sample_noise(self, cond, out, noise):
        """sddm_sample_noise: every Gaussian draw from `noise` ([T + 1][B][N] fp32 on the device).
        The library reads (T + 1) * B * N floats from that pointer, so the buffer is checked here:
        a contiguous fp32 device tensor of shape (T + 1, B, ...) holding exactly that many values."""
        import torch
        B, N = out.shape[0], out.shape[-1]
        T = self.timesteps
        if not isinstance(noise, torch.Tensor) or noise.dtype != torch.float32 or not noise.is_contiguous():
            raise ValueError("noise must be a contiguous float32 tensor")
        if noise.device != out.device:
            raise ValueError(f"noise must be on {out.device}, got {noise.device}")
        if noise.dim() < 2 or noise.shape[1] != B or noise.shape[0] != T + 1 or \
                noise.numel() != noise.shape[0] * B * N:
            raise ValueError(f"noise must be [T + 1, {B}, {N}] draws, got {tuple(noise.shape)}")
        check(lib().sddm_sample_noise(self._h, _ptr(cond), B, N, _ptr(noise), _ptr(out), _stream(torch, cond.device)))

    def sample_continuous(self, cond, out, record, sample_inter, seed, row_offset=0):
        import torch
        B, N = out.shape[0], out.shape[-1]
        check(lib().sddm_sample_continuous(self._h, _ptr(cond), B, N, int(seed) & (2 ** 64 - 1),
                                           int(row_offset), _ptr(out), _ptr(record), int(sample_inter),
                                           _stream(torch, cond.device)))

    def network_forward(self, cond, x_t, noise_level, eps_out):
        import torch
        B, N = x_t.shape[0], x_t.shape[-1]
        check(lib().sddm_network_forward(self._h, _ptr(cond), _ptr(x_t), _ptr(noise_level), B, N,
                                         _ptr(eps_out), _stream(torch, cond.device)))

    def dual_transformer(self, x, out):
        """sddm_dual_transformer: x, out [B, C, dim2, dim1] fp32 on the device (C = 160 in a UNetTST context, 64 in a CAUNet or TSTNN one)."""
        import torch
        B, _, dim2, dim1 = x.shape
        check(lib().sddm_dual_transformer(self._h, _ptr(x), B, dim2, dim1, _ptr(out), _stream(torch, x.device)))

    def self_attention(self, layer, x, out):
        """sddm_self_attention: x, out [B, C, H, W] fp32 on the device, layer e.g. "mid.0.attn" (a UNetModified context)."""
        import torch
        B, _, H, W = x.shape
        check(lib().sddm_self_attention(self._h, layer.encode(), _ptr(x), B, H, W, _ptr(out), _stream(torch, x.device)))

    def transition(self, mode, x_t, eps, cond, t, out, seed, row_offset=0):
        import torch
        B, N = x_t.shape[0], x_t.numel() // x_t.shape[0]
        check(lib().sddm_transition(self._h, int(mode), _ptr(x_t), _ptr(eps), _ptr(cond), int(t), B, N,
                                    int(seed) & (2 ** 64 - 1), int(row_offset), _ptr(out),
                                    _stream(torch, x_t.device)))

    def set_conv_tuning(self, table):
        """Per-layer conv tiles measured by tools/tune_deep.py (dict or JSON text)."""
        import json as _json
        text = table if isinstance(table, str) else _json.dumps(table)
        check(lib().sddm_set_conv_tuning(self._h, text.encode()))

    def q_sample(self, mode, x0, y, noise, t, r, x_t, combined, s_out, level_out):
        import torch
        B, N = x0.shape[0], x0.numel() // x0.shape[0]
        check(lib().sddm_q_sample(self._h, int(mode), _ptr(x0), _ptr(y), _ptr(noise), _ptr(t), _ptr(r), B, N,
                                  _ptr(x_t), _ptr(combined), _ptr(s_out), _ptr(level_out),
                                  _stream(torch, x0.device)))

    def initial_state(self, mode, cond, out, seed, row_offset=0):
        import torch
        B, N = out.shape[0], out.numel() // out.shape[0]
        check(lib().sddm_initial_state(self._h, int(mode), _ptr(cond), B, N, int(seed) & (2 ** 64 - 1),
                                       int(row_offset), _ptr(out), _stream(torch, out.device)))

    def profile(self, enable=True):
        check(lib().sddm_profile_enable(self._h, 1 if enable else 0))

    def profile_read(self, kernel_class):
        ms, b, f = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        check(lib().sddm_profile_read(self._h, kernel_class.encode(), ctypes.byref(ms), ctypes.byref(n),
                                      ctypes.byref(b), ctypes.byref(f)))
        return dict(avg_ms=ms.value, launches=n.value, bytes_per_launch=b.value, flops_per_launch=f.value)

    def profile_ops(self):
        buf = ctypes.create_string_buffer(1 << 20)
        check(lib().sddm_profile_ops(self._h, buf, len(buf)))
        return json.loads(buf.value.decode())


def log_spectrogram(audio, n_fft, hop, window, fb, n_out, out):
    """sddm_log_spectrogram on CUDA tensors (audio [B, N], window [n_fft], fb [n_fft/2+1, n_out] or
    None, out [B, n_out, 1 + N // hop])."""
    import torch
    B, N = audio.shape
    check(lib().sddm_log_spectrogram(_ptr(audio), B, N, int(n_fft), int(hop), _ptr(window), _ptr(fb), int(n_out),
                                     _ptr(out), _stream(torch, audio.device)))
