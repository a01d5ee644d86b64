"""Generate the UNetTST goldens by running the REFERENCE Python on CPU (build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_unettst.py [--reference /root/reference]

As gen_golden_waveunet.py: the reference is imported read-only, its UNetTST (built with the network
args of config_unettst.json) carries the deterministic weights of ``tests/_weights.py`` (seed 0) and
torch.randn_like / torch.randn are replaced by the Philox stream of ``oracle.philox`` (draw 0 = x_T,
draw t = transition noise at step t, seed 7).  Written: ``unettst.npz`` (inputs and outputs only, no
weights), ``unettst_keys.json`` (state-dict keys and shapes) and ``reference_config_unettst.json``
(the settings of config_unettst.json).

  fw/{cond,x_t,noise_level,eps}            one forward at B = 2, N = 4160 (mid sees [2, 160, 2, 4])
  dt/<dim2>x<dim1>/{x,y}                   the network's ``mid`` (Dual_Transformer(160, 160, 0, 6)) alone at
                                           B = 2 for (dim2, dim1) = (1,4), (2,4), (3,4), (8,4), (2,8)
  inf/cond, inf/<noise_condition>/<mode>/steps   the unmodified SDDM.infer (model.py:50-124) at N = 4160,
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
DT_SHAPES = ((1, 4), (2, 4), (3, 4), (8, 4), (2, 8))
B, N = 2, 4160


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
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
    from model.UNetTST import UNetTST
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    with open(os.path.join(args.reference, "config_unettst.json")) as f:
        cfg = json.load(f)
    net, shapes = load_seed0(torch, make_params, UNetTST(num_samples=N, **cfg["network"]["args"]))
    n_par = sum(int(np.prod(s)) for s in shapes.values())
    assert len(shapes) == 454 and n_par == 8201395, (len(shapes), n_par)
    assert sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("mid.")) == 3438642
    out = {}
    cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
    x_t = philox.normal(6, 0, (B, 1, N))
    nl = np.array([0.7, 0.3], dtype=np.float32)
    with torch.no_grad():
        eps = net(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl).reshape(B, 1, 1)).numpy().copy()
    assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
    out["fw/cond"], out["fw/x_t"], out["fw/noise_level"], out["fw/eps"] = cond, x_t, nl, eps
    print(f"UNetTST: {n_par} parameters, {len(shapes)} keys, eps rms {np.sqrt(np.mean(eps ** 2)):.3f}", flush=True)
    for i, (d2, d1) in enumerate(DT_SHAPES):
        x = philox.normal(11 + i, 0, (B, 160, d2, d1))
        with torch.no_grad():
            y = net.mid(torch.from_numpy(x)).numpy().copy()
        assert y.shape == x.shape and np.isfinite(y).all()
        out[f"dt/{d2}x{d1}/x"], out[f"dt/{d2}x{d1}/y"] = x, y
        print(f"Dual_Transformer {d2}x{d1}: output rms {np.sqrt(np.mean(y ** 2)):.3f}", flush=True)
    out["inf/cond"] = cond
    for nc, mode in INFER_CASES:
        out[f"inf/{nc}/{mode}/steps"] = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode)
    np.savez_compressed(os.path.join(args.out, "unettst.npz"), **out)
    with open(os.path.join(args.out, "unettst_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in shapes.items()], f, indent=0)
    with open(os.path.join(args.out, "reference_config_unettst.json"), "w") as f:
        json.dump(cfg, f, indent=4)
        f.write("\n")
    print("wrote", os.path.join(args.out, "unettst.npz"), os.path.getsize(os.path.join(args.out, "unettst.npz")), "bytes")


if __name__ == "__main__":
    main()
