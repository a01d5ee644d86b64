"""ORACLE (test infrastructure only) -- UNetModified and its SelfAttention restated with torch functionals
on the CPU in float64 (reference model/UNetModified.py:140-169, 192-323); results are rounded to float32.
Weights: dict of numpy arrays keyed like the reference state_dict without the ``noise_estimate_model.``
prefix.  Any batch size.

``rounding=torch.bfloat16 / torch.float16`` is the CPU emulation of the 16-bit paths: it rounds what
the kernels round and nothing else (the arithmetic stays float64).  In the convolutions as in
_unettst_oracle.py: every 3x3 / 1x1 convolution's input (after GroupNorm + Swish), weight and stored
output, and the first conv's output.  In the SelfAttention: the normalized input, the qkv and out
weights, the stored q / k / v, the probabilities where they enter P V (unnormalized, relative to the
row maximum, as the kernel holds them; the normalizer sums the unrounded ones), O before the out conv
and the stored result.

Test weights: with the bounds of ``_weights.make_params`` alone the attention is nearly uniform (logit
std 0.35, mean row-max probability 0.018 at 128 positions), so a wrong scale, a missing maximum or a bad
rescale would pass.  ``sharpen`` multiplies the q and k rows of every ``attn.qkv.weight`` (the first 2C
rows) by QK_SCALE = 3: logit std 3.3-3.4, row-max probability 0.33-0.57.  The golden generator and every
test apply it after make_params.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

import _dual_transformer_oracle as DT

ARGS = {"in_channel": 2, "out_channel": 1, "inner_channel": 32, "norm_groups": 32, "channel_mults": [1, 2, 4, 8, 8],
        "attn_layer": [4], "res_blocks": 1, "dropout": 0, "segment_len": 128, "segment_stride": 64}
QK_SCALE = 3.0


def sharpen(P, scale=QK_SCALE):
    """The q and k rows of every attn.qkv.weight times `scale` (a new dict; P is left alone)."""
    out = dict(P)
    for k, v in P.items():
        if k.endswith("attn.qkv.weight"):
            w = np.array(v, copy=True)
            w[:2 * w.shape[1]] *= np.float32(scale)
            out[k] = w
    return out


def make_params(args=None, seed=0):
    from _weights import make_params as mp
    return sharpen(mp(param_shapes(args), seed))


def _layers(args):
    """downs, mid, ups as (kind, name, cin, cout, attn) in forward order (UNetModified.py:228-277)."""
    E, mults, rb, al = args["inner_channel"], args["channel_mults"], args["res_blocks"], args["attn_layer"]
    n = len(mults)
    downs, feat, cin, idx = [("conv", "downs.0", args["in_channel"], E, False)], [E], E, 1
    for ind in range(n):
        cout = E * mults[ind]
        for _ in range(rb):
            downs.append(("res", f"downs.{idx}", cin, cout, ind in al)); idx += 1
            feat.append(cout)
            cin = cout
        if ind != n - 1:
            downs.append(("down", f"downs.{idx}", cin, cin, False)); idx += 1
            feat.append(cin)
    mid = [("res", "mid.0", cin, cin, True), ("res", "mid.1", cin, cin, False)]
    ups, idx = [], 0
    for ind in reversed(range(n)):
        cout = E * mults[ind]
        for _ in range(rb + 1):
            ups.append(("res", f"ups.{idx}", cin + feat.pop(), cout, ind in al)); idx += 1
            cin = cout
        if ind >= 1:
            ups.append(("up", f"ups.{idx}", cin, cin, False)); idx += 1
    return downs, mid, ups, cin


def attention_shapes(C, prefix):
    return {prefix + "norm.weight": (C,), prefix + "norm.bias": (C,), prefix + "qkv.weight": (3 * C, C, 1, 1),
            prefix + "out.weight": (C, C, 1, 1), prefix + "out.bias": (C,)}


def param_shapes(args=None):
    """State-dict shapes without the module prefix (242 tensors at ARGS)."""
    args = ARGS if args is None else args
    E = args["inner_channel"]
    s = {"noise_level_mlp.1.weight": (4 * E, E), "noise_level_mlp.1.bias": (4 * E,),
         "noise_level_mlp.3.weight": (E, 4 * E), "noise_level_mlp.3.bias": (E,)}
    downs, mid, ups, last = _layers(args)
    for kind, n, ci, co, attn in downs + mid + ups:
        if kind == "res":
            r = n + ".res_block"
            s[r + ".noise_func.noise_func.0.weight"], s[r + ".noise_func.noise_func.0.bias"] = (co, E), (co,)
            s[r + ".block1.block.0.weight"], s[r + ".block1.block.0.bias"] = (ci,), (ci,)
            s[r + ".block1.block.3.weight"], s[r + ".block1.block.3.bias"] = (co, ci, 3, 3), (co,)
            s[r + ".block2.block.0.weight"], s[r + ".block2.block.0.bias"] = (co,), (co,)
            s[r + ".block2.block.3.weight"], s[r + ".block2.block.3.bias"] = (co, co, 3, 3), (co,)
            if ci != co:
                s[r + ".res_conv.weight"], s[r + ".res_conv.bias"] = (co, ci, 1, 1), (co,)
            if attn:
                s.update(attention_shapes(co, n + ".attn."))
        elif kind == "conv":
            s[n + ".weight"], s[n + ".bias"] = (co, ci, 3, 3), (co,)
        else:
            s[n + ".conv.weight"], s[n + ".conv.bias"] = (co, ci, 3, 3), (co,)
    s["final_conv.block.0.weight"], s["final_conv.block.0.bias"] = (last,), (last,)
    s["final_conv.block.3.weight"], s["final_conv.block.3.bias"] = (args["out_channel"], last, 3, 3), (args["out_channel"],)
    return s


_q, _w64 = DT.rounder, DT.w64


def _logits(W, prefix, x, q, G):
    """(q k^T / sqrt(C) [B, P, P], v [B, C, P]) of the block `prefix` ("mid.0.attn.") on x [B, C, H, W]."""
    B, C, H, Wd = x.shape
    h = q(F.group_norm(x, G, W[prefix + "norm.weight"], W[prefix + "norm.bias"], 1e-5))
    qkv = q(F.conv2d(h, q(W[prefix + "qkv.weight"]))).reshape(B, 3 * C, H * Wd)
    qq, kk, vv = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    return torch.einsum("bcp,bck->bpk", qq, kk) / math.sqrt(C), vv


def _attention(W, prefix, x, q, G):
    B, C, H, Wd = x.shape
    s, vv = _logits(W, prefix, x, q, G)
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)        # in (0, 1], as the kernel holds it
    o = torch.einsum("bpk,bck->bcp", q(p), vv) / p.sum(dim=-1)[:, None, :]
    o = q(o).reshape(B, C, H, Wd)
    return q(F.conv2d(o, q(W[prefix + "out.weight"]), W[prefix + "out.bias"]) + x)


def self_attention(P, prefix, x, rounding=None, groups=32):
    """One SelfAttention alone: x [B, C, H, W] -> [B, C, H, W] float32; prefix e.g. "mid.0.attn."."""
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items() if k.startswith(prefix)}
    q = _q(rounding)
    return _attention(W, prefix, q(torch.from_numpy(np.asarray(x, np.float64))), q, groups).numpy().astype(np.float32)


def logit_stats(P, prefix, x, groups=32):
    """(std of the logits, mean row-max probability, max |logit|) of the block on x."""
    W = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items() if k.startswith(prefix)}
    s, _ = _logits(W, prefix, torch.from_numpy(np.asarray(x, np.float64)), _q(None), groups)
    return float(s.std()), float(torch.softmax(s, -1).max(dim=-1).values.mean()), float(s.abs().max())


def forward(P, cond, x_t, noise_level, rounding=None, args=None):
    """UNetModified.forward (UNetModified.py:279-323): cond, x_t [B, 1, N], noise level [B] -> [B, 1, N]."""
    args = ARGS if args is None else args
    q, W = _q(rounding), _w64(P)
    E, G, seg, st = args["inner_channel"], args["norm_groups"], args["segment_len"], args["segment_stride"]
    cond = torch.from_numpy(np.asarray(cond, np.float64).reshape(len(cond), 1, -1))
    x_t = torch.from_numpy(np.asarray(x_t, np.float64).reshape(len(x_t), 1, -1))
    B, _, N = cond.shape
    nf = (N - seg) // st + 1
    idx = torch.arange(nf)[:, None] * st + torch.arange(seg)[None, :]
    x = torch.cat([cond[:, :, idx], x_t[:, :, idx]], dim=1)
    # noise_level_mlp (UNetModified.py:46-59, 212-217): fp32 step, exponent and product as the reference's
    # float32 tensors, sin then cos, no final Swish
    half = E // 2
    step = (np.arange(half, dtype=np.float32) / np.float32(half)).astype(np.float32)
    ev = np.exp((np.float32(-math.log(1e4)) * step).astype(np.float32)).astype(np.float32)
    arg = (np.asarray(noise_level, np.float32).reshape(-1, 1) * ev[None, :]).astype(np.float32).astype(np.float64)
    t = torch.from_numpy(np.concatenate([np.sin(arg), np.cos(arg)], -1))
    t = F.linear(t, W["noise_level_mlp.1.weight"], W["noise_level_mlp.1.bias"])
    t = F.linear(t * torch.sigmoid(t), W["noise_level_mlp.3.weight"], W["noise_level_mlp.3.bias"])

    def block(n, h, extra=None):
        h = F.group_norm(h, G, W[n + ".block.0.weight"], W[n + ".block.0.bias"], 1e-5)
        h = F.conv2d(q(h * torch.sigmoid(h)), q(W[n + ".block.3.weight"]), W[n + ".block.3.bias"], padding=1)
        return h if extra is None else h + extra

    def res(n, h, ci, co, attn):
        r = n + ".res_block"
        te = F.linear(t, W[r + ".noise_func.noise_func.0.weight"], W[r + ".noise_func.noise_func.0.bias"])
        a = q(block(r + ".block1", h, te[:, :, None, None]))
        sc = h if ci == co else F.conv2d(h, q(W[r + ".res_conv.weight"]), W[r + ".res_conv.bias"])
        y = q(block(r + ".block2", a, sc))
        return _attention(W, n + ".attn.", y, q, G) if attn else y

    downs, mid, ups, last = _layers(args)
    feats = []
    for kind, n, ci, co, attn in downs:
        if kind == "res":
            x = res(n, x, ci, co, attn)
        elif kind == "down":
            x = q(F.conv2d(x, q(W[n + ".conv.weight"]), W[n + ".conv.bias"], stride=2, padding=1))
        else:
            x = q(F.conv2d(x, W[n + ".weight"], W[n + ".bias"], padding=1))
        feats.append(x)
    for kind, n, ci, co, attn in mid:
        x = res(n, x, ci, co, attn)
    for kind, n, ci, co, attn in ups:
        if kind == "res":
            x = res(n, torch.cat([x, feats.pop()], dim=1), ci, co, attn)
        else:
            x = q(F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), q(W[n + ".conv.weight"]), W[n + ".conv.bias"], padding=1))
    h = F.group_norm(x, G, W["final_conv.block.0.weight"], W["final_conv.block.0.bias"], 1e-5)
    y = F.conv2d(h * torch.sigmoid(h), W["final_conv.block.3.weight"], W["final_conv.block.3.bias"], padding=1)
    out = torch.zeros(B, y.shape[1], N, dtype=torch.float64)
    for i in range(nf):
        out[:, :, i * st:i * st + seg] += y[:, :, i, :]
    return out.numpy().astype(np.float32)
