"""ORACLE (test infrastructure only) -- CAUNet and its Dual_Transformer restated with torch functionals
on the CPU in float64 (reference model/CAUNet.py:152-201, 307-374); results are rounded to float32.
Weights: dict of numpy arrays keyed like the reference state_dict without the ``noise_estimate_model.``
prefix.  Any batch size (the noise level is a vector of B entries).

``rounding=torch.bfloat16 / torch.float16`` is the CPU emulation of the 16-bit paths: it rounds what
the kernels round and nothing else (the arithmetic stays float64).  In the conv part: every MFMA
conv's weight, its input where it enters the product (after the affine for a DenseBlock's input) and
its stored output (after LayerNorm and PReLU), and first_conv's output (its weights, like
final_conv's, are fp32).  In the Dual_Transformer: the matrix weights (in_proj, out_proj, weight_ih,
weight_hh, linear2, the two 1x1 convs), the activations where they enter one of those products, q
(after the scaling), k, v and the softmax's probabilities where they enter the two attention
products, and the block's output tensor.  Everything else (the norms, softmax, the GRU's gates and
state, PReLU, the noise MLPs) is not rounded.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _dual_transformer_oracle as DT

ARGS = {"inner_channel": 64, "n_encode_layers": 4, "dense_depth": 3, "n_TSTB": 6, "segment_len": 128,
        "segment_stride": 64, "use_affine_level": False}


def _layer_names(args):
    n = args["n_encode_layers"]
    return [f"downs.{i}." for i in range(n)] + [f"ups.{i}." for i in range(n)]


def _widths(args):
    n, seg = args["n_encode_layers"], args["segment_len"]
    return [seg >> i for i in range(n)] + [(seg >> n) << i for i in range(n)]


def dual_transformer_shapes(C=64, n_tstb=6, prefix="mid."):
    return DT.shapes(C, n_tstb, prefix, per_channel=True)


def param_shapes(args=None):
    """State-dict shapes without the module prefix (450 tensors at ARGS)."""
    args = ARGS if args is None else args
    C, depth = args["inner_channel"], args["dense_depth"]
    out = C * (2 if args["use_affine_level"] else 1)
    s = {"first_conv.weight": (C, 2, 1, 1), "first_conv.bias": (C,)}
    for l, (p, W) in enumerate(zip(_layer_names(args), _widths(args))):
        for k in range(1, depth + 1):
            s[p + f"dense.conv{k}.weight"], s[p + f"dense.conv{k}.bias"] = (C, C * k, 2, 3), (C,)
            s[p + f"dense.norm{k}.weight"], s[p + f"dense.norm{k}.bias"] = (W,), (W,)
            s[p + f"dense.prelu{k}.weight"] = (C,)
        s[p + "noise_func.noise_func.0.weight"], s[p + "noise_func.noise_func.0.bias"] = (4 * C, C), (4 * C,)
        s[p + "noise_func.noise_func.1.weight"] = (4 * C,)
        s[p + "noise_func.noise_func.2.weight"], s[p + "noise_func.noise_func.2.bias"] = (out, 4 * C), (out,)
        if l < args["n_encode_layers"]:
            s[p + "downsample.0.weight"], s[p + "downsample.0.bias"] = (C, C, 1, 3), (C,)
            s[p + "downsample.1.weight"], s[p + "downsample.1.bias"] = (W // 2,), (W // 2,)
            s[p + "downsample.2.weight"] = (C,)
        else:
            s[p + "upsample.0.conv.weight"], s[p + "upsample.0.conv.bias"] = (2 * C, 2 * C, 1, 3), (2 * C,)
            s[p + "upsample.1.weight"], s[p + "upsample.1.bias"] = (2 * W,), (2 * W,)
            s[p + "upsample.2.weight"] = (C,)
    s.update(dual_transformer_shapes(C, args["n_TSTB"]))
    s["final_conv.weight"], s["final_conv.bias"] = (1, C, 1, 1), (1,)
    return s


_q, _w64 = DT.rounder, DT.w64


def _dual_transformer(W, x, q, n_tstb, prefix="mid."):
    return DT.block(W, x, q, n_tstb, prefix, round_attention=True, hoist_gru=True)


def dual_transformer(P, x, rounding=None, n_tstb=6, prefix="mid."):
    """The block alone: x [b, 64, dim2, dim1] -> [b, 64, dim2, dim1] float32."""
    y = _dual_transformer(_w64(P), torch.from_numpy(np.asarray(x, np.float64)), _q(rounding), n_tstb, prefix)
    return y.numpy().astype(np.float32)


def _noise_encoding(noise_level, dim):
    """PositionalEncoding: the fp32 argument of the reference, then float64 sin | cos."""
    half = dim // 2
    step = torch.arange(half, dtype=torch.float32) / half
    lv = torch.from_numpy(np.asarray(noise_level, np.float32).reshape(-1))
    arg = (lv.unsqueeze(1) * torch.exp(-math.log(1e4) * step.unsqueeze(0))).to(torch.float64)
    return torch.cat([torch.sin(arg), torch.cos(arg)], dim=-1)


def forward(P, cond, x_t, noise_level, rounding=None, args=None):
    """CAUNet.forward: cond, x_t [B, 1, N], noise level [B] -> [B, 1, N]."""
    args = ARGS if args is None else args
    q, W = _q(rounding), _w64(P)
    C, seg, st, depth = args["inner_channel"], args["segment_len"], args["segment_stride"], args["dense_depth"]
    n_enc, affine = args["n_encode_layers"], args["use_affine_level"]
    cond = torch.from_numpy(np.asarray(cond, np.float64).reshape(len(cond), 1, -1))
    x_t = torch.from_numpy(np.asarray(x_t, np.float64).reshape(len(x_t), 1, -1))
    B, _, N = cond.shape
    assert (N - seg) % st == 0
    nf = (N - seg) // st + 1
    idx = torch.arange(nf)[:, None] * st + torch.arange(seg)[None, :]
    enc = _noise_encoding(noise_level, C)
    assert enc.shape[0] == B
    x = q(F.conv2d(torch.cat([cond[:, :, idx], x_t[:, :, idx]], dim=1), W["first_conv.weight"], W["first_conv.bias"]))

    def norm_act(h, n_norm, n_prelu):
        h = F.layer_norm(h, (h.shape[-1],), W[n_norm + ".weight"], W[n_norm + ".bias"], 1e-5)
        return q(F.prelu(h, W[n_prelu + ".weight"]))

    def dense(p, h):
        m = F.linear(F.prelu(F.linear(enc, W[p + "noise_func.noise_func.0.weight"], W[p + "noise_func.noise_func.0.bias"]),
                             W[p + "noise_func.noise_func.1.weight"]),
                     W[p + "noise_func.noise_func.2.weight"], W[p + "noise_func.noise_func.2.bias"])[:, :, None, None]
        skip = q((1 + m[:, :C]) * h + m[:, C:] if affine else h + m)      # rounded where it enters the convs
        for k in range(1, depth + 1):
            dil = 2 ** (k - 1)
            out = F.conv2d(F.pad(skip, (1, 1, dil, 0)), q(W[p + f"dense.conv{k}.weight"]), W[p + f"dense.conv{k}.bias"], dilation=(dil, 1))
            out = norm_act(out, p + f"dense.norm{k}", p + f"dense.prelu{k}")
            skip = torch.cat([out, skip], dim=1)
        return out

    feats = []
    for i in range(n_enc):
        p = f"downs.{i}."
        x = dense(p, x)
        x = F.conv2d(x, q(W[p + "downsample.0.weight"]), W[p + "downsample.0.bias"], stride=(1, 2), padding=(0, 1))
        x = norm_act(x, p + "downsample.1", p + "downsample.2")
        feats.append(x)
    x = _dual_transformer(W, x, q, args["n_TSTB"])
    for i in range(n_enc):
        p = f"ups.{i}."
        x = torch.cat([dense(p, x), feats.pop()], dim=1)
        x = F.conv2d(x, q(W[p + "upsample.0.conv.weight"]), W[p + "upsample.0.conv.bias"], padding=(0, 1))
        b, c2, H, Wd = x.shape
        x = x.view(b, 2, c2 // 2, H, Wd).permute(0, 2, 3, 4, 1).reshape(b, c2 // 2, H, 2 * Wd)   # channel r * 64 + c -> [c, h, 2 w + r]
        x = norm_act(x, p + "upsample.1", p + "upsample.2")
    y = F.conv2d(x, W["final_conv.weight"], W["final_conv.bias"])
    out = torch.zeros(B, 1, N, dtype=torch.float64)
    for i in range(nf):
        out[:, :, i * st:i * st + seg] += y[:, :, i, :]
    return out.numpy().astype(np.float32)
