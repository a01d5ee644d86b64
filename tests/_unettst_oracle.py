"""ORACLE (test infrastructure only) -- UNetTST and its Dual_Transformer restated with torch functionals
on the CPU in float64 (reference model/UNetTST.py:113-233, 270-392); results are rounded to float32.
Weights: dict of numpy arrays keyed like the reference state_dict without the ``noise_estimate_model.``
prefix.  Any batch size.

``rounding=torch.bfloat16 / torch.float16`` is the CPU emulation of the 16-bit paths: it rounds what
the kernels round and nothing else (the arithmetic stays float64).  In the UNet part: every 3x3 / 1x1
convolution's input (after GroupNorm + Swish), weight and stored output, and the first conv's output
(its weights, like the final conv's, are fp32).  In the Dual_Transformer: the matrix weights (in_proj,
out_proj, weight_ih, weight_hh, linear2, the two 1x1 convs), the activations where they enter one of
those products (they are fp32 everywhere else) and the block's output tensor.
"""
import numpy as np
import torch
import torch.nn.functional as F

import _dual_transformer_oracle as DT

ARGS = {"in_channel": 2, "out_channel": 1, "inner_channel": 32, "norm_groups": 32, "channel_mults": [1, 2, 3, 4, 5],
        "res_blocks": 1, "n_TSTB": 6, "dropout": 0, "segment_len": 128, "segment_stride": 64}


def _layers(args):
    """downs, ups as (kind, name, cin, cout) in forward order (UNetTST.py:301-357)."""
    E, mults, rb = args["inner_channel"], args["channel_mults"], args["res_blocks"]
    downs, feat, cin, idx = [("conv", "downs.0", args["in_channel"], E)], [E], E, 1
    for m in mults:
        cout = E * m
        for _ in range(rb):
            downs.append(("res", f"downs.{idx}", cin, cout)); idx += 1
            feat.append(cout)
            cin = cout
        downs.append(("down", f"downs.{idx}", cout, cout)); idx += 1
        feat.append(cout)
    bottom, ups, idx = cout, [], 0
    for ind in reversed(range(len(mults))):
        cin = E * mults[ind]
        ups.append(("res", f"ups.{idx}", cin + feat.pop(), cin)); idx += 1
        ups.append(("up", f"ups.{idx}", cin, cin)); idx += 1
        cout = E if ind == 0 else E * mults[ind - 1]
        for _ in range(rb):
            ups.append(("res", f"ups.{idx}", cin + feat.pop(), cout)); idx += 1
            cin = cout
    return downs, ups, bottom, cout


def dual_transformer_shapes(C=160, n_tstb=6, prefix="mid."):
    return DT.shapes(C, n_tstb, prefix, per_channel=False)


def param_shapes(args=None):
    """State-dict shapes without the module prefix (454 tensors at ARGS)."""
    args = ARGS if args is None else args
    E = args["inner_channel"]
    s = {"noise_level_mlp.1.weight": (4 * E, E), "noise_level_mlp.1.bias": (4 * E,),
         "noise_level_mlp.3.weight": (E, 4 * E), "noise_level_mlp.3.bias": (E,)}
    downs, ups, bottom, last = _layers(args)
    for kind, n, ci, co in downs + ups:
        if kind == "res":
            s[n + ".noise_func.noise_func.0.weight"], s[n + ".noise_func.noise_func.0.bias"] = (co, E), (co,)
            s[n + ".block1.block.0.weight"], s[n + ".block1.block.0.bias"] = (ci,), (ci,)
            s[n + ".block1.block.3.weight"], s[n + ".block1.block.3.bias"] = (co, ci, 3, 3), (co,)
            s[n + ".block2.block.0.weight"], s[n + ".block2.block.0.bias"] = (co,), (co,)
            s[n + ".block2.block.3.weight"], s[n + ".block2.block.3.bias"] = (co, co, 3, 3), (co,)
            if ci != co:
                s[n + ".res_conv.weight"], s[n + ".res_conv.bias"] = (co, ci, 1, 1), (co,)
        elif kind == "conv":
            s[n + ".weight"], s[n + ".bias"] = (co, ci, 3, 3), (co,)
        else:
            s[n + ".conv.weight"], s[n + ".conv.bias"] = (co, ci, 3, 3), (co,)
    s.update(dual_transformer_shapes(bottom, args["n_TSTB"]))
    s["final_conv.block.0.weight"], s["final_conv.block.0.bias"] = (last,), (last,)
    s["final_conv.block.3.weight"], s["final_conv.block.3.bias"] = (args["out_channel"], last, 3, 3), (args["out_channel"],)
    return s


_q, _w64 = DT.rounder, DT.w64


def _dual_transformer(W, x, q, n_tstb, prefix="mid."):
    return DT.block(W, x, q, n_tstb, prefix, round_attention=False, hoist_gru=False)


def dual_transformer(P, x, rounding=None, n_tstb=6, prefix="mid."):
    """The block alone: x [b, 160, dim2, dim1] -> [b, 160, dim2, dim1] float32."""
    y = _dual_transformer(_w64(P), torch.from_numpy(np.asarray(x, np.float64)), _q(rounding), n_tstb, prefix)
    return y.numpy().astype(np.float32)


def forward(P, cond, x_t, noise_level, rounding=None, args=None):
    """UNetTST.forward (UNetTST.py:359-392): cond, x_t [B, 1, N], noise level [B] -> [B, 1, N]."""
    args = ARGS if args is None else args
    q, W = _q(rounding), _w64(P)
    E, G, seg, st = args["inner_channel"], args["norm_groups"], args["segment_len"], args["segment_stride"]
    cond = torch.from_numpy(np.asarray(cond, np.float64).reshape(len(cond), 1, -1))
    x_t = torch.from_numpy(np.asarray(x_t, np.float64).reshape(len(x_t), 1, -1))
    B, _, N = cond.shape
    nf = (N - seg) // st + 1
    idx = torch.arange(nf)[:, None] * st + torch.arange(seg)[None, :]
    x = torch.cat([cond[:, :, idx], x_t[:, :, idx]], dim=1)
    # noise_level_mlp: the fp32 encoding vector and fp32 product of the reference, no final Swish
    half = E // 2
    ev = (np.float32(1e4) * np.power(np.float32(10.0), (-(np.arange(half).astype(np.float32)) * np.float32(4.0)) / np.float32(half))
          .astype(np.float32)).astype(np.float32)
    arg = (np.asarray(noise_level, np.float32).reshape(-1, 1) * ev[None, :]).astype(np.float32).astype(np.float64)
    t = torch.from_numpy(np.concatenate([np.sin(arg), np.cos(arg)], -1))
    t = F.linear(t, W["noise_level_mlp.1.weight"], W["noise_level_mlp.1.bias"])
    t = F.linear(t * torch.sigmoid(t), W["noise_level_mlp.3.weight"], W["noise_level_mlp.3.bias"])

    def block(n, h, extra=None):
        h = F.group_norm(h, G, W[n + ".block.0.weight"], W[n + ".block.0.bias"], 1e-5)
        h = F.conv2d(q(h * torch.sigmoid(h)), q(W[n + ".block.3.weight"]), W[n + ".block.3.bias"], padding=1)
        return h if extra is None else h + extra

    def res(n, h, ci, co):
        te = F.linear(t, W[n + ".noise_func.noise_func.0.weight"], W[n + ".noise_func.noise_func.0.bias"])
        a = q(block(n + ".block1", h, te[:, :, None, None]))
        r = h if ci == co else F.conv2d(h, q(W[n + ".res_conv.weight"]), W[n + ".res_conv.bias"])
        return q(block(n + ".block2", a, r))

    downs, ups, bottom, last = _layers(args)
    feats = []
    for kind, n, ci, co in downs:
        if kind == "res":
            x = res(n, x, ci, co)
        elif kind == "down":
            x = q(F.conv2d(x, q(W[n + ".conv.weight"]), W[n + ".conv.bias"], stride=2, padding=1))
        else:
            x = q(F.conv2d(x, W[n + ".weight"], W[n + ".bias"], padding=1))
        feats.append(x)
    x = _dual_transformer(W, x, q, args["n_TSTB"])
    for kind, n, ci, co in ups:
        if kind == "res":
            x = res(n, torch.cat([x, feats.pop()], dim=1), ci, co)
        else:
            x = q(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), q(W[n + ".conv.weight"]), W[n + ".conv.bias"], padding=1))
    h = F.group_norm(x, G, W["final_conv.block.0.weight"], W["final_conv.block.0.bias"], 1e-5)
    y = F.conv2d(h * torch.sigmoid(h), W["final_conv.block.3.weight"], W["final_conv.block.3.bias"], padding=1)
    out = torch.zeros(B, y.shape[1], N, dtype=torch.float64)
    for i in range(nf):
        out[:, :, i * st:i * st + seg] += y[:, :, i, :]
    return out.numpy().astype(np.float32)
