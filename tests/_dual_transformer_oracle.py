"""ORACLE (test infrastructure only) -- the Dual_Transformer of UNetTST (reference model/UNetTST.py:113-233)
and CAUNet (model/CAUNet.py:152-201) restated with torch functionals on the CPU in float64.

The two blocks differ in the channel count, in their PReLU slopes (one for UNetTST, one per channel
for CAUNet: `per_channel`) and in what the 16-bit kernels round (`round_attention`): CAUNet's kernels
round q (after the scaling), k, v and the softmax's probabilities where they enter the two attention
products; UNetTST's fused kernel keeps them in registers.  Both round the matrix weights (in_proj,
out_proj, weight_ih, weight_hh, linear2, the two 1x1 convs), the activations where they enter one of
those products and the block's output tensor; the arithmetic stays float64.
`hoist_gru` keeps each oracle's own form of the GRU's input projection (CAUNet's: once for all steps;
UNetTST's: per step): in float64 the two differ in the last bits at dim2 = 1 (dt/1x4, dt/1x8), and the
16-bit bars are computed from these outputs.
_unettst_oracle.py and _caunet_oracle.py bind the three and export the block under their own names.
"""
import numpy as np
import torch
import torch.nn.functional as F


def shapes(C, n_tstb, prefix, per_channel):
    d, s = C // 2, {}
    s[prefix + "input.0.weight"], s[prefix + "input.0.bias"] = (d, C, 1, 1), (d,)
    s[prefix + "input.1.weight"] = (d,) if per_channel else (1,)
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
    s[prefix + "output.0.weight"], s[prefix + "output.0.bias"] = (C, d, 1, 1), (C,)
    s[prefix + "output.1.weight"] = (C,) if per_channel else (1,)
    return s


def rounder(rounding):
    return (lambda t: t) if rounding is None else (lambda t: t.to(rounding).to(torch.float64))


def w64(P):
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in P.items()}


def _encoder(W, e, x, q, qa, hoist_gru):
    """One TransformerEncoderLayer: x [L, Nb, d] -> [L, Nb, d]; 4 heads, GRU hidden 2 d per direction."""
    L, Nb, d = x.shape
    H, hd = 4, d // 4
    qkv = q(x) @ q(W[e + "self_attn.in_proj_weight"]).T + W[e + "self_attn.in_proj_bias"]
    qh, kh, vh = (t.reshape(L, Nb * H, hd).transpose(0, 1) for t in qkv.chunk(3, dim=-1))
    a = qa(torch.softmax(qa(qh * hd ** -0.5) @ qa(kh).transpose(1, 2), dim=-1)) @ qa(vh)   # [Nb * H, L, hd]
    a = a.transpose(0, 1).reshape(L, Nb, d)
    a = q(a) @ q(W[e + "self_attn.out_proj.weight"]).T + W[e + "self_attn.out_proj.bias"]
    src = F.layer_norm(x + a, (d,), W[e + "norm1.weight"], W[e + "norm1.bias"], 1e-5)
    outs = []
    for sfx, order in (("", range(L)), ("_reverse", range(L - 1, -1, -1))):             # gates r, z, n; h0 = 0
        wih, whh = q(W[e + "gru.weight_ih_l0" + sfx]), q(W[e + "gru.weight_hh_l0" + sfx])
        bih, bhh = W[e + "gru.bias_ih_l0" + sfx], W[e + "gru.bias_hh_l0" + sfx]
        gi_all = q(src) @ wih.T + bih if hoist_gru else None
        h = torch.zeros(Nb, 2 * d, dtype=torch.float64)
        o = [None] * L
        for t in order:
            gi = (gi_all[t] if hoist_gru else q(src[t]) @ wih.T + bih).chunk(3, -1)
            gh = (q(h) @ whh.T + bhh).chunk(3, -1)
            r, z = torch.sigmoid(gi[0] + gh[0]), torch.sigmoid(gi[1] + gh[1])
            n = torch.tanh(gi[2] + r * gh[2])
            h = (1 - z) * n + z * h
            o[t] = h
        outs.append(torch.stack(o))
    out = torch.cat(outs, dim=-1)
    s2 = q(F.relu(out)) @ q(W[e + "linear2.weight"]).T + W[e + "linear2.bias"]
    return F.layer_norm(src + s2, (d,), W[e + "norm2.weight"], W[e + "norm2.bias"], 1e-5)


def block(W, x, q, n_tstb, prefix, round_attention, hoist_gru):
    """Dual_Transformer.forward on float64 [b, C, dim2, dim1]; GroupNorm(1, C / 2, eps 1e-8)."""
    b, C, dim2, dim1 = x.shape
    d = C // 2
    qa = q if round_attention else (lambda t: t)
    out = F.conv2d(q(x), q(W[prefix + "input.0.weight"]), W[prefix + "input.0.bias"])
    out = F.prelu(out, W[prefix + "input.1.weight"])
    for i in range(n_tstb):
        row = out.permute(3, 0, 2, 1).reshape(dim1, b * dim2, d)
        row = _encoder(W, f"{prefix}row_trans.{i}.", row, q, qa, hoist_gru).reshape(dim1, b, dim2, d).permute(1, 3, 2, 0)
        out = out + F.group_norm(row, 1, W[f"{prefix}row_norm.{i}.weight"], W[f"{prefix}row_norm.{i}.bias"], 1e-8)
        col = out.permute(2, 0, 3, 1).reshape(dim2, b * dim1, d)
        col = _encoder(W, f"{prefix}col_trans.{i}.", col, q, qa, hoist_gru).reshape(dim2, b, dim1, d).permute(1, 3, 0, 2)
        out = out + F.group_norm(col, 1, W[f"{prefix}col_norm.{i}.weight"], W[f"{prefix}col_norm.{i}.bias"], 1e-8)
    out = F.conv2d(q(out), q(W[prefix + "output.0.weight"]), W[prefix + "output.0.bias"])
    return q(F.prelu(out, W[prefix + "output.1.weight"]))
