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

ARGS = {"inner_channel": 64, "n_encode_layers": 4, "dense_depth": 3, "n_TSTB": 6, "segment_len": 128,
        "segment_stride": 64, "use_affine_level": False}


def _layer_names(args):
    n = args["n_encode_layers"]
    return [f"downs.{i}." for i in range(n)] + [f"ups.{i}." for i in range(n)]


def _widths(args):
    n, seg = args["n_encode_layers"], args["segment_len"]
    return [seg >> i for i in range(n)] + [(seg >> n) << i for i in range(n)]


def dual_transformer_shapes(C=64, n_tstb=6, prefix="mid."):
    d, s = C // 2, {}
    s[prefix + "input.0.weight"], s[prefix + "input.0.bias"], s[prefix + "input.1.weight"] = (d, C, 1, 1), (d,), (d,)
    for i in range(n_tstb):
        for p in ("row", "col"):
            e = f"{prefix}{p}_trans.{i}."
            s[e + "self_attn.in_proj_weight"], s[e + "self_attn.in_proj_bias"] = (3 * d, d), (3 * d,)
            s[e + "self_attn.out_proj.weight"], s[e + "self_attn.out_proj.bias"] = (d, d), (d,)
            for sfx in ("", "_reverse"):
                s[e + "gru.weight_ih_l0" + sfx], s[e + "gru.weight_hh_l0" + sfx] = (6 * d, d), (6 * d, 2 * d)
                s[e + "gru.bias_ih_l0" + sfx], s[e + "gru.bias_hh_l0" + sfx] = (6 * d,), (6 * d,)
            s[e + "linear2.weight"], s[e + "linear2.bias"] = (d, 4 * d), (d,)
            for n in ("norm1", "norm2"):
                s[e + n + ".weight"], s[e + n + ".bias"] = (d,), (d,)
            s[f"{prefix}{p}_norm.{i}.weight"], s[f"{prefix}{p}_norm.{i}.bias"] = (d,), (d,)
    s[prefix + "output.0.weight"], s[prefix + "output.0.bias"], s[prefix + "output.1.weight"] = (C, d, 1, 1), (C,), (C,)
    return s


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


def _q(rounding):
    return (lambda t: t) if rounding is None else (lambda t: t.to(rounding).to(torch.float64))


def _w64(P):
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items()}


def _encoder(W, e, x, q):
    """One TransformerEncoderLayer: x [L, Nb, d] -> [L, Nb, d]; 4 heads, GRU hidden 2 d per direction."""
    L, Nb, d = x.shape
    H, hd = 4, d // 4
    qkv = q(x) @ q(W[e + "self_attn.in_proj_weight"]).T + W[e + "self_attn.in_proj_bias"]
    qh, kh, vh = (t.reshape(L, Nb * H, hd).transpose(0, 1) for t in qkv.chunk(3, dim=-1))
    a = q(torch.softmax(q(qh * hd ** -0.5) @ q(kh).transpose(1, 2), dim=-1)) @ q(vh)     # [Nb * H, L, hd]
    a = a.transpose(0, 1).reshape(L, Nb, d)
    a = q(a) @ q(W[e + "self_attn.out_proj.weight"]).T + W[e + "self_attn.out_proj.bias"]
    src = F.layer_norm(x + a, (d,), W[e + "norm1.weight"], W[e + "norm1.bias"], 1e-5)
    outs = []
    for sfx, order in (("", range(L)), ("_reverse", range(L - 1, -1, -1))):             # gates r, z, n; h0 = 0
        wih, whh = q(W[e + "gru.weight_ih_l0" + sfx]), q(W[e + "gru.weight_hh_l0" + sfx])
        bih, bhh = W[e + "gru.bias_ih_l0" + sfx], W[e + "gru.bias_hh_l0" + sfx]
        gi_all = q(src) @ wih.T + bih
        h = torch.zeros(Nb, 2 * d, dtype=torch.float64)
        o = [None] * L
        for t in order:
            gi, gh = gi_all[t].chunk(3, -1), (q(h) @ whh.T + bhh).chunk(3, -1)
            r, z = torch.sigmoid(gi[0] + gh[0]), torch.sigmoid(gi[1] + gh[1])
            n = torch.tanh(gi[2] + r * gh[2])
            h = (1 - z) * n + z * h
            o[t] = h
        outs.append(torch.stack(o))
    out = torch.cat(outs, dim=-1)
    s2 = q(F.relu(out)) @ q(W[e + "linear2.weight"]).T + W[e + "linear2.bias"]
    return F.layer_norm(src + s2, (d,), W[e + "norm2.weight"], W[e + "norm2.bias"], 1e-5)


def _dual_transformer(W, x, q, n_tstb, prefix="mid."):
    """The block on float64 [b, C, dim2, dim1]: per-channel PReLUs, GroupNorm(1, C / 2, eps 1e-8)."""
    b, C, dim2, dim1 = x.shape
    d = C // 2
    out = F.conv2d(q(x), q(W[prefix + "input.0.weight"]), W[prefix + "input.0.bias"])
    out = F.prelu(out, W[prefix + "input.1.weight"])
    for i in range(n_tstb):
        row = out.permute(3, 0, 2, 1).reshape(dim1, b * dim2, d)
        row = _encoder(W, f"{prefix}row_trans.{i}.", row, q).reshape(dim1, b, dim2, d).permute(1, 3, 2, 0)
        out = out + F.group_norm(row, 1, W[f"{prefix}row_norm.{i}.weight"], W[f"{prefix}row_norm.{i}.bias"], 1e-8)
        col = out.permute(2, 0, 3, 1).reshape(dim2, b * dim1, d)
        col = _encoder(W, f"{prefix}col_trans.{i}.", col, q).reshape(dim2, b, dim1, d).permute(1, 3, 0, 2)
        out = out + F.group_norm(col, 1, W[f"{prefix}col_norm.{i}.weight"], W[f"{prefix}col_norm.{i}.bias"], 1e-8)
    out = F.conv2d(q(out), q(W[prefix + "output.0.weight"]), W[prefix + "output.0.bias"])
    return q(F.prelu(out, W[prefix + "output.1.weight"]))


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
