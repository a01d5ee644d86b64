"""Generate the DenoiseWaveGrad1 / DenoiseWaveGrad3 goldens by running the REFERENCE Python on CPU
(build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_denoise_wavegrad.py [--reference /root/reference]

As gen_golden.py: the reference is imported read-only, its modules carry the deterministic weights
of ``tests/_weights.py`` (seed 0) and torch.randn_like / torch.randn are replaced by the Philox
stream of ``oracle.philox`` (draw 0 = x_T, draw t = transition noise at step t, seed 7).  Written:
``denoise_wavegrad.npz`` (inputs and outputs only, no weights) and ``denoise_wavegrad_keys.json``
(state-dict key and shape lists of both networks).

Per network (B = 2, N = 3 hop; the reference cannot run B = 1, wavegrad.py:37-47):
  <net>/fw/{cond,x_t,noise_level,eps}          one forward
  <net>/inf/<noise_condition>/<mode>/{out,steps}  the unmodified SDDM.infer (model.py:50-124) at schedule
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
NETS = {"DenoiseWaveGrad1": 400, "DenoiseWaveGrad3": 300}
B = 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    for p in (HERE, os.path.join(REPO, "tests"), REPO):
        sys.path.insert(0, p)
    from gen_golden import CLAMP_CAPS, INFER_CASES, load_seed0, record_infer
    from oracle import philox
    from _weights import make_params
    sys.path.insert(0, args.reference)
    import torch
    torch.set_num_threads(8)
    import model.wavegrad as ref_wavegrad
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    out, keys = {}, {}
    for name, hop in NETS.items():
        net, shapes = load_seed0(torch, make_params, getattr(ref_wavegrad, name)())
        keys[name] = [[k, list(s)] for k, s in shapes.items()]
        N = 3 * hop
        cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
        x_t = philox.normal(6, 0, (B, 1, N))
        nl = np.array([0.7, 0.3], dtype=np.float32)
        with torch.no_grad():
            eps = net(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl)).numpy().copy()
        assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
        out[f"{name}/fw/cond"], out[f"{name}/fw/x_t"], out[f"{name}/fw/noise_level"] = cond, x_t, nl
        out[f"{name}/fw/eps"] = eps
        print(f"{name}: {sum(int(np.prod(s)) for s in shapes.values())} parameters, {len(shapes)} keys, "
              f"eps rms {np.sqrt(np.mean(eps ** 2)):.3f}", flush=True)
        out[f"{name}/inf/cond"] = cond
        for nc, mode in INFER_CASES:
            steps = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode, caps=CLAMP_CAPS,
                                 tag=name + " ")
            out[f"{name}/inf/{nc}/{mode}/out"] = steps[-1]
            out[f"{name}/inf/{nc}/{mode}/steps"] = steps
    np.savez_compressed(os.path.join(args.out, "denoise_wavegrad.npz"), **out)
    with open(os.path.join(args.out, "denoise_wavegrad_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", os.path.join(args.out, "denoise_wavegrad.npz"))


if __name__ == "__main__":
    main()
