"""ORACLE (test infrastructure only) -- TSTNN and its Dual_Transformer restated with torch functionals
on the CPU in float64 (reference model/tstnn.py:114-164, 216-299); results are rounded to float32.
Weights: dict of numpy arrays keyed like the reference state_dict without the ``noise_estimate_model.``
prefix.  Any batch size; the noise level is accepted and ignored, as in the reference.

``rounding=torch.bfloat16 / torch.float16`` is the CPU emulation of the 16-bit paths: it rounds what
the kernels round and nothing else (the arithmetic stays float64).  In the conv part: every MFMA
conv's weight and its stored output (after LayerNorm and PReLU), which is also the next product's
input, and the first kernel's output (inp_conv's weights, like out_conv's, are fp32).  In the gated
mask: the three 1x1 weights, the gate tanh(.) * sigmoid(.) where it enters maskconv, and the stored
x1 * mask.  In the Dual_Transformer: what _dual_transformer_oracle.py rounds for CAUNet's kernels (the
matrix weights, the activations where they enter a product, q, k, v and the probabilities), the
PReLU'd activations where they enter the output conv, and the block's output tensor.  Everything else
(the norms, softmax, the GRU's gates and state, PReLU, tanh, sigmoid, ReLU) is not rounded.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _dual_transformer_oracle as DT

ARGS = {"F": 512, "stride": 256, "n_channels": 64}
N_LAYERS = 4
_q, _w64 = DT.rounder, DT.w64


def dual_transformer_shapes(C=64, n_tstb=N_LAYERS, prefix="dual_transformer."):
    """tstnn.py:122-141: single-slope PReLUs, output = (PReLU, Conv2d)."""
    s = DT.shapes(C, n_tstb, prefix, per_channel=False)
    for k in ("output.0.weight", "output.0.bias", "output.1.weight"):
        del s[prefix + k]
    s[prefix + "output.0.weight"] = (1,)
    s[prefix + "output.1.weight"], s[prefix + "output.1.bias"] = (C, C // 2, 1, 1), (C,)
    return s


def _dense_shapes(s, p, W, C, depth=4):
    for k in range(1, depth + 1):
        s[p + f"conv{k}.weight"], s[p + f"conv{k}.bias"] = (C, C * k, 2, 3), (C,)
        s[p + f"norm{k}.weight"], s[p + f"norm{k}.bias"] = (W,), (W,)
        s[p + f"prelu{k}.weight"] = (C,)


def param_shapes(args=None):
    """State-dict shapes without the module prefix (229 tensors at ARGS)."""
    args = ARGS if args is None else args
    C, Fl = args["n_channels"], args["F"]
    s = {"inp_conv.weight": (C, 2, 1, 1), "inp_conv.bias": (C,), "inp_norm.weight": (Fl,), "inp_norm.bias": (Fl,),
         "inp_prelu.weight": (C,)}
    _dense_shapes(s, "enc_dense1.", Fl, C)
    s["enc_conv1.weight"], s["enc_conv1.bias"] = (C, C, 1, 3), (C,)
    s["enc_norm1.weight"], s["enc_norm1.bias"], s["enc_prelu1.weight"] = (Fl // 2,), (Fl // 2,), (C,)
    s.update(dual_transformer_shapes(C))
    for n in ("output1.0", "output2.0", "maskconv"):
        s[n + ".weight"], s[n + ".bias"] = (C, C, 1, 1), (C,)
    _dense_shapes(s, "dec_dense1.", Fl // 2, C)
    s["dec_conv1.conv.weight"], s["dec_conv1.conv.bias"] = (2 * C, C, 1, 3), (2 * C,)
    s["dec_norm1.weight"], s["dec_norm1.bias"], s["dec_prelu1.weight"] = (Fl,), (Fl,), (C,)
    s["out_conv.weight"], s["out_conv.bias"] = (1, C, 1, 1), (1,)
    return s


def _dual_transformer(W, x, q, n_tstb=N_LAYERS, prefix="dual_transformer.", prelu_after=False):
    """tstnn.py:143-164 on float64 [b, C, dim2, dim1].  prelu_after: the (wrong) CAUNet order of the
    output stage, conv then PReLU, for the wiring test."""
    b, C, dim2, dim1 = x.shape
    d = C // 2
    out = F.conv2d(q(x), q(W[prefix + "input.0.weight"]), W[prefix + "input.0.bias"])
    out = F.prelu(out, W[prefix + "input.1.weight"])
    for i in range(n_tstb):
        row = out.permute(3, 0, 2, 1).reshape(dim1, b * dim2, d)
        row = DT._encoder(W, f"{prefix}row_trans.{i}.", row, q, q, True).reshape(dim1, b, dim2, d).permute(1, 3, 2, 0)
        out = out + F.group_norm(row, 1, W[f"{prefix}row_norm.{i}.weight"], W[f"{prefix}row_norm.{i}.bias"], 1e-8)
        col = out.permute(2, 0, 3, 1).reshape(dim2, b * dim1, d)
        col = DT._encoder(W, f"{prefix}col_trans.{i}.", col, q, q, True).reshape(dim2, b, dim1, d).permute(1, 3, 0, 2)
        out = out + F.group_norm(col, 1, W[f"{prefix}col_norm.{i}.weight"], W[f"{prefix}col_norm.{i}.bias"], 1e-8)
    wo, bo, slope = q(W[prefix + "output.1.weight"]), W[prefix + "output.1.bias"], W[prefix + "output.0.weight"]
    if prelu_after:
        return q(F.prelu(F.conv2d(q(out), wo, bo), slope))
    return q(F.conv2d(q(F.prelu(out, slope)), wo, bo))


def dual_transformer(P, x, rounding=None, n_tstb=N_LAYERS, prefix="dual_transformer.", prelu_after=False):
    """The block alone: x [b, 64, dim2, dim1] -> [b, 64, dim2, dim1] float32."""
    y = _dual_transformer(_w64(P), torch.from_numpy(np.asarray(x, np.float64)), _q(rounding), n_tstb, prefix, prelu_after)
    return y.numpy().astype(np.float32)


def forward(P, cond, x_t, noise_level=None, rounding=None, args=None, taps=None, prelu_after=False):
    """TSTNN.forward: cond, x_t [B, 1, N] -> [B, 1, N].  taps: a dict that receives the mask."""
    args = ARGS if args is None else args
    q, W = _q(rounding), _w64(P)
    Fl, st = args["F"], args["stride"]
    cond = torch.from_numpy(np.asarray(cond, np.float64).reshape(len(cond), 1, -1))
    x_t = torch.from_numpy(np.asarray(x_t, np.float64).reshape(len(x_t), 1, -1))
    B, _, N = cond.shape
    assert (N - Fl) % st == 0
    nf = (N - Fl) // st + 1
    idx = torch.arange(nf)[:, None] * st + torch.arange(Fl)[None, :]

    def norm_act(h, n_norm, n_prelu):
        h = F.layer_norm(h, (h.shape[-1],), W[n_norm + ".weight"], W[n_norm + ".bias"], 1e-5)
        return q(F.prelu(h, W[n_prelu + ".weight"]))

    def dense(p, skip):
        for k in range(1, 5):
            dil = 2 ** (k - 1)
            out = F.conv2d(F.pad(skip, (1, 1, dil, 0)), q(W[p + f"conv{k}.weight"]), W[p + f"conv{k}.bias"], dilation=(dil, 1))
            out = norm_act(out, p + f"norm{k}", p + f"prelu{k}")
            skip = torch.cat([out, skip], dim=1)
        return out

    x = F.conv2d(torch.cat([cond[:, :, idx], x_t[:, :, idx]], dim=1), W["inp_conv.weight"], W["inp_conv.bias"])
    x = norm_act(x, "inp_norm", "inp_prelu")
    x = dense("enc_dense1.", x)
    x1 = F.conv2d(F.pad(x, (1, 1, 0, 0)), q(W["enc_conv1.weight"]), W["enc_conv1.bias"], stride=(1, 2))
    x1 = norm_act(x1, "enc_norm1", "enc_prelu1")
    y = _dual_transformer(W, x1, q, prelu_after=prelu_after)
    gate = torch.tanh(F.conv2d(y, q(W["output1.0.weight"]), W["output1.0.bias"])) * \
        torch.sigmoid(F.conv2d(y, q(W["output2.0.weight"]), W["output2.0.bias"]))
    mask = F.relu(F.conv2d(q(gate), q(W["maskconv.weight"]), W["maskconv.bias"]))
    if taps is not None:
        taps["mask"] = mask
    x = dense("dec_dense1.", q(x1 * mask))
    x = F.conv2d(F.pad(x, (1, 1, 0, 0)), q(W["dec_conv1.conv.weight"]), W["dec_conv1.conv.bias"])
    b, c2, H, Wd = x.shape
    x = x.view(b, 2, c2 // 2, H, Wd).permute(0, 2, 3, 4, 1).reshape(b, c2 // 2, H, 2 * Wd)   # channel r * 64 + c -> [c, h, 2 w + r]
    x = norm_act(x, "dec_norm1", "dec_prelu1")
    y = F.conv2d(x, W["out_conv.weight"], W["out_conv.bias"])
    out = torch.zeros(B, 1, N, dtype=torch.float64)
    for i in range(nf):
        out[:, :, i * st:i * st + Fl] += y[:, :, i, :]
    return out.numpy().astype(np.float32)
