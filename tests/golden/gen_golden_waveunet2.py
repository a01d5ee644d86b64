"""Generate the Waveunet2 goldens by running the REFERENCE Python on CPU (build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_waveunet2.py [--reference /root/reference]

As gen_golden_denoise_wavegrad.py: the reference is imported read-only, its module (built with the
network args of config_waveunet2.json) carries the deterministic weights of ``tests/_weights.py``
(seed 0) and torch.randn_like / torch.randn are replaced by the Philox stream of ``oracle.philox``
(draw 0 = x_T, draw t = transition noise at step t, seed 7).  Written: ``waveunet2.npz`` (inputs and
outputs only, no weights), ``waveunet2_keys.json`` (state-dict keys and shapes) and
``reference_config_waveunet2.json`` (the settings of config_waveunet2.json).

B = 2, N = 296 (level lengths 296 / 148 / 74 / 37):
  fw/{cond,x_t,noise_level,eps}          one forward
  inf/<noise_condition>/<mode>/{out,steps}  the unmodified SDDM.infer (model.py:50-124) at schedule
                                         linear, 3, 1e-4, 0.05 with every intermediate x_t
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
SCHED = ("linear", 3, 1e-4, 0.05)
B, N = 2, 296


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    for p in (HERE, os.path.join(REPO, "tests"), REPO):
        sys.path.insert(0, p)
    from gen_golden import CLAMP_CAPS, INFER_CASES, clamped_share, load_seed0, record_infer
    from oracle import philox
    from _weights import make_params
    sys.path.insert(0, args.reference)
    import torch
    torch.set_num_threads(8)
    from model.waveunet2 import Waveunet2
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    with open(os.path.join(args.reference, "config_waveunet2.json")) as f:
        cfg = json.load(f)
    net, shapes = load_seed0(torch, make_params, Waveunet2(**cfg["network"]["args"]))
    out = {}
    cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
    x_t = philox.normal(6, 0, (B, 1, N))
    nl = np.array([0.7, 0.3], dtype=np.float32)
    with torch.no_grad():
        eps = net(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl).reshape(B, 1, 1)).numpy().copy()
    assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
    assert len(shapes) == 90 and sum(int(np.prod(s)) for s in shapes.values()) == 449473
    # the network clamps its own output: a mostly clamped golden would hide errors
    assert clamped_share(eps) <= 0.25, f"forward: clamped share {clamped_share(eps)}"
    out["fw/cond"], out["fw/x_t"], out["fw/noise_level"], out["fw/eps"] = cond, x_t, nl, eps
    print(f"Waveunet2: {sum(int(np.prod(s)) for s in shapes.values())} parameters, {len(shapes)} keys, "
          f"eps rms {np.sqrt(np.mean(eps ** 2)):.3f}, clamped share {clamped_share(eps):.3f}", flush=True)
    out["inf/cond"] = cond
    for nc, mode in INFER_CASES:
        steps = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode, caps=CLAMP_CAPS)
        out[f"inf/{nc}/{mode}/out"] = steps[-1]
        out[f"inf/{nc}/{mode}/steps"] = steps
    np.savez_compressed(os.path.join(args.out, "waveunet2.npz"), **out)
    with open(os.path.join(args.out, "waveunet2_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in shapes.items()], f, indent=0)
    with open(os.path.join(args.out, "reference_config_waveunet2.json"), "w") as f:
        json.dump(cfg, f, indent=4)
        f.write("\n")
    print("wrote", os.path.join(args.out, "waveunet2.npz"))


if __name__ == "__main__":
    main()
