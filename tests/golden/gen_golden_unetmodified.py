"""Generate the UNetModified goldens by running the REFERENCE Python on CPU (build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_unetmodified.py [--reference /root/reference]

As gen_golden_unettst.py: the reference is imported read-only, its UNetModified (built with ARGS of
tests/_unetmodified_oracle.py: channel_mults (1, 2, 4, 8, 8), attn_layer [4], res_blocks 1) carries the
deterministic weights of ``tests/_weights.py`` (seed 0) with the q and k rows of every attn.qkv.weight
times QK_SCALE (the oracle's ``sharpen``: without it the attention is nearly uniform), and torch.randn_like
/ torch.randn are replaced by the Philox stream of ``oracle.philox`` (draw 0 = x_T, draw t = transition
noise at step t, seed 7).  Written: ``unetmodified.npz`` (inputs and outputs only, no weights),
``unetmodified_keys.json`` (state-dict keys and shapes) and ``reference_config_unetmodified.json`` (the
settings used: the reference ships no config for this network).

  fw/{cond,x_t,noise_level,eps}            one forward at B = 2, N = 2112 (the bottom level is 2 x 8 = 16 positions)
  at/<C>x<H>x<W>/{x,y}                     the reference SelfAttention alone: the network's mid.0.attn at C = 256,
                                           a SelfAttention(160) with the seed-0 weights of the same names at C = 160
  at12/256x16x8/y                          mid.0.attn with the q / k rows times 12 instead of QK_SCALE on at/256x16x8/x
  inf/cond, inf/<noise_condition>/<mode>/steps   the unmodified SDDM.infer (model.py:50-124) at N = 2112,
                                           schedule linear, 3, 1e-4, 0.05: every x_t (the last is the output)
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCHED = ("linear", 3, 1e-4, 0.05)
AT_SHAPES = ((256, 1, 1, 2), (256, 2, 8, 2), (160, 3, 8, 2), (256, 5, 13, 1), (256, 16, 8, 1))   # C, H, W, B
COUNTS = ((1, [4], 242, 16715937), (2, [3, 4], 387, 25787009), (3, [4], 482, 32228961))   # res_blocks, attn_layer, keys, parameters
B, N = 2, 2112


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    for p in (HERE, os.path.join(REPO, "tests"), REPO):
        sys.path.insert(0, p)
    from gen_golden import INFER_CASES, record_infer
    from oracle import philox
    from _weights import make_params
    import _unetmodified_oracle as O
    sys.path.insert(0, args.reference)
    import torch
    torch.set_num_threads(8)
    from model.UNetModified import SelfAttention, UNetModified
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    for rb, al, n_keys, n_par in COUNTS:      # the reference's own counts at the default widths
        sd = UNetModified(num_samples=N, **dict(O.ARGS, res_blocks=rb, attn_layer=al)).state_dict()
        got = (len(sd), sum(v.numel() for v in sd.values()))
        assert got == (n_keys, n_par), (rb, al, got)
        assert {k: tuple(v.shape) for k, v in sd.items()} == O.param_shapes(dict(O.ARGS, res_blocks=rb, attn_layer=al)), (rb, al)
    net = UNetModified(num_samples=N, **O.ARGS)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    P = O.sharpen(make_params(shapes, 0))
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
    net.eval()
    out = {}
    cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
    x_t = philox.normal(6, 0, (B, 1, N))
    nl = np.array([0.7, 0.3], dtype=np.float32)
    with torch.no_grad():
        eps = net(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl).reshape(B, 1, 1)).numpy().copy()
    assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
    out["fw/cond"], out["fw/x_t"], out["fw/noise_level"], out["fw/eps"] = cond, x_t, nl, eps
    print(f"UNetModified: {len(shapes)} keys, eps rms {np.sqrt(np.mean(eps ** 2)):.3f}", flush=True)
    for i, (C, H, W, Bn) in enumerate(AT_SHAPES):
        if C == 256:
            blk, Pa = net.mid[0].attn, P
        else:
            blk = SelfAttention(C).eval()
            Pa = O.sharpen(make_params(O.attention_shapes(C, "mid.0.attn."), 0))
            blk.load_state_dict({k[len("mid.0.attn."):]: torch.from_numpy(v) for k, v in Pa.items()})
        x = philox.normal(21 + i, 0, (Bn, C, H, W))
        with torch.no_grad():
            y = blk(torch.from_numpy(x)).numpy().copy()
        assert y.shape == x.shape and np.isfinite(y).all()
        out[f"at/{C}x{H}x{W}/x"], out[f"at/{C}x{H}x{W}/y"] = x, y
        std, pmax, amax = O.logit_stats(Pa, "mid.0.attn.", x)
        print(f"SelfAttention {C}x{H}x{W}: output rms {np.sqrt(np.mean(y ** 2)):.3f}, attention branch rms "
              f"{np.sqrt(np.mean((y - x) ** 2)):.3f}, logit std {std:.2f}, mean row-max probability {pmax:.3f}", flush=True)
    # the same block with the q / k rows times 12 instead of QK_SCALE (max |logit| about 260) on the last input:
    # the reference's own float32 result, the yardstick of the GPU test's large-logit bar
    big = SelfAttention(256).eval()
    Pb = O.sharpen({k: v for k, v in make_params(shapes, 0).items() if k.startswith("mid.0.attn.")}, 12.0)
    big.load_state_dict({k[len("mid.0.attn."):]: torch.from_numpy(v) for k, v in Pb.items()})
    with torch.no_grad():
        y = big(torch.from_numpy(out["at/256x16x8/x"])).numpy().copy()
    assert np.isfinite(y).all()
    out["at12/256x16x8/y"] = y
    print("SelfAttention 256x16x8, q / k rows x 12: logit std %.1f, row-max probability %.3f, max |logit| %.0f"
          % O.logit_stats(Pb, "mid.0.attn.", out["at/256x16x8/x"]), flush=True)
    out["inf/cond"] = cond
    for nc, mode in INFER_CASES:
        out[f"inf/{nc}/{mode}/steps"] = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode)
    np.savez_compressed(os.path.join(args.out, "unetmodified.npz"), **out)
    with open(os.path.join(args.out, "unetmodified_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in shapes.items()], f, indent=0)
    cfg = {"num_samples": N, "sample_rate": 16000,
           "arch": {"type": "SDDM", "args": {"p_transition": "original", "q_transition": "original"}},
           "diffusion": {"type": "GaussianDiffusion", "args": dict(zip(("schedule", "n_timestep", "linear_start", "linear_end"), SCHED))},
           "network": {"type": "UNetModified", "args": O.ARGS}, "qk_scale": O.QK_SCALE}
    with open(os.path.join(args.out, "reference_config_unetmodified.json"), "w") as f:
        json.dump(cfg, f, indent=4)
        f.write("\n")
    print("wrote", os.path.join(args.out, "unetmodified.npz"), os.path.getsize(os.path.join(args.out, "unetmodified.npz")), "bytes")


if __name__ == "__main__":
    main()
