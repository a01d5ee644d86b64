"""Generate the CAUNet goldens by running the REFERENCE Python on CPU (build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_caunet.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

As gen_golden_unettst.py: the reference is imported read-only, its CAUNet (built with the network
args of config_caunet.json) carries the deterministic weights of ``tests/_weights.py`` (seed 0) and
torch.randn_like / torch.randn are replaced by the Philox stream of ``oracle.philox`` (draw 0 = x_T,
draw t = transition noise at step t, seed 7).  Written: ``caunet.npz`` (inputs and outputs only, no
weights), ``caunet_keys.json`` (state-dict keys and shapes) and ``reference_config_caunet.json``
(the settings of config_caunet.json).

  fw/{cond,x_t,noise_level,eps}            one forward at B = 2, N = 704 (10 frames; mid sees [2, 64, 10, 8])
  fwa/eps                                  the same inputs with use_affine_level = true (its own seed-0 weights)
  dt/<dim2>x8/{x,y}                        the network's ``mid`` (Dual_Transformer(64, 64, 0, 6)) alone at
                                           B = 2 for dim2 = 1, 2, 3, 10, 17, 70
  inf/cond, inf/<noise_condition>/<mode>/steps   the unmodified SDDM.infer (model.py:50-124) at N = 704,
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
DT_DIM2 = (1, 2, 3, 10, 17, 70)
B, N = 2, 704


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project (read only)")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    for p in (HERE, os.path.join(REPO, "tests"), REPO):
        sys.path.insert(0, p)
    from gen_golden import INFER_CASES, load_seed0, record_infer
    from oracle import philox
    from _weights import make_params
    sys.path.insert(0, args.reference)
    import torch
    torch.set_num_threads(8)
    from model.CAUNet import CAUNet
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    with open(os.path.join(args.reference, "config_caunet.json")) as f:
        cfg = json.load(f)

    def build(**change):
        return load_seed0(torch, make_params, CAUNet(num_samples=N, **dict(cfg["network"]["args"], **change)))

    net, shapes = build()
    n_par = sum(int(np.prod(s)) for s in shapes.values())
    assert len(shapes) == 450 and n_par == 2258049, (len(shapes), n_par)
    assert sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("mid.")) == 558400
    out = {}
    cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
    x_t = philox.normal(6, 0, (B, 1, N))
    nl = np.array([0.7, 0.3], dtype=np.float32)
    for tag, n in (("fw", net), ("fwa", build(use_affine_level=True)[0])):
        with torch.no_grad():
            eps = n(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl).reshape(B, 1, 1)).numpy().copy()
        assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
        out[tag + "/eps"] = eps
        print(f"CAUNet {tag}: eps rms {np.sqrt(np.mean(eps ** 2)):.3f}", flush=True)
    out["fw/cond"], out["fw/x_t"], out["fw/noise_level"] = cond, x_t, nl
    for i, d2 in enumerate(DT_DIM2):
        x = philox.normal(11 + i, 0, (B, 64, d2, 8))
        with torch.no_grad():
            y = net.mid(torch.from_numpy(x)).numpy().copy()
        assert y.shape == x.shape and np.isfinite(y).all()
        out[f"dt/{d2}x8/x"], out[f"dt/{d2}x8/y"] = x, y
        print(f"Dual_Transformer {d2}x8: output rms {np.sqrt(np.mean(y ** 2)):.3f}", flush=True)
    out["inf/cond"] = cond
    for nc, mode in INFER_CASES:
        out[f"inf/{nc}/{mode}/steps"] = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode)
    np.savez_compressed(os.path.join(args.out, "caunet.npz"), **out)
    with open(os.path.join(args.out, "caunet_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in shapes.items()], f, indent=0)
    with open(os.path.join(args.out, "reference_config_caunet.json"), "w") as f:
        json.dump(cfg, f, indent=4)
        f.write("\n")
    size = os.path.getsize(os.path.join(args.out, "caunet.npz"))
    assert size < 1000000, size
    print("wrote", os.path.join(args.out, "caunet.npz"), size, "bytes")


if __name__ == "__main__":
    main()
