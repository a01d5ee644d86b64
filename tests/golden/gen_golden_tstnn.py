"""Generate the TSTNN goldens by running the REFERENCE Python on CPU (build container only).

Usage (from the repo root, with the reference mounted read-only):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_tstnn.py --reference PATH_TO_THE_REFERENCE_CHECKOUT

As gen_golden_caunet.py: the reference is imported read-only, its TSTNN (built with the network args
of config_tstnn.json) carries the deterministic weights of ``tests/_weights.py`` (seed 0) and
torch.randn_like / torch.randn are replaced by the Philox stream of ``oracle.philox`` (draw 0 = x_T,
draw t = transition noise at step t, seed 7).  Written: ``tstnn.npz`` (the network: fw/ and inf/) and
``tstnn_dt.npz`` (the block alone: dt/) -- inputs and outputs only, no weights; together they are
1.06 MB, more than a committed file may hold, so they are two files -- ``tstnn_keys.json`` (state-dict
keys and shapes, in order) and ``reference_config_tstnn.json`` (the settings of config_tstnn.json).

  fw/{cond,x_t,noise_level,eps}            one forward at B = 2, N = 2816 (10 frames, so the dilation-8 tap
                                           reads real rows; dual_transformer sees [2, 64, 10, 256])
  dt/<dim2>x<dim1>/{x,y}                   the network's ``dual_transformer`` (Dual_Transformer(64, 64, num_layers=4))
                                           alone: B = 2 at (1,16), (2,33), (5,40); B = 1 at (3,256)
  inf/cond, inf/<noise_condition>/<mode>/steps   the unmodified SDDM.infer (model.py:50-124) at N = 2816,
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
DT_SHAPES = ((2, 1, 16), (2, 2, 33), (2, 5, 40), (1, 3, 256))   # (B, dim2, dim1)
B, N = 2, 2816


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
    from model.tstnn import TSTNN
    from model.diffusion import GaussianDiffusion
    from model.model import SDDM

    with open(os.path.join(args.reference, "config_tstnn.json")) as f:
        cfg = json.load(f)
    net, shapes = load_seed0(torch, make_params, TSTNN(num_samples=N, **cfg["network"]["args"]))
    n_par = sum(int(np.prod(s)) for s in shapes.values())
    assert len(shapes) == 229 and n_par == 924835, (len(shapes), n_par)
    assert sum(int(np.prod(s)) for k, s in shapes.items() if k.startswith("dual_transformer.")) == 373602
    out, blk = {}, {}
    cond = np.clip(0.3 * philox.normal(5, 0, (B, 1, N)), -1, 1).astype(np.float32)
    x_t = philox.normal(6, 0, (B, 1, N))
    nl = np.array([0.7, 0.3], dtype=np.float32)
    with torch.no_grad():
        eps = net(torch.from_numpy(cond), torch.from_numpy(x_t), torch.from_numpy(nl).reshape(B, 1, 1)).numpy().copy()
    assert eps.shape == (B, 1, N) and np.isfinite(eps).all()
    print(f"TSTNN fw: eps rms {np.sqrt(np.mean(eps ** 2)):.3f}", flush=True)
    out["fw/cond"], out["fw/x_t"], out["fw/noise_level"], out["fw/eps"] = cond, x_t, nl, eps
    for i, (b, d2, d1) in enumerate(DT_SHAPES):
        x = philox.normal(11 + i, 0, (b, 64, d2, d1))
        with torch.no_grad():
            y = net.dual_transformer(torch.from_numpy(x)).numpy().copy()
        assert y.shape == x.shape and np.isfinite(y).all()
        blk[f"dt/{d2}x{d1}/x"], blk[f"dt/{d2}x{d1}/y"] = x, y
        print(f"Dual_Transformer {d2}x{d1}: output rms {np.sqrt(np.mean(y ** 2)):.3f}", flush=True)
    out["inf/cond"] = cond
    for nc, mode in INFER_CASES:
        out[f"inf/{nc}/{mode}/steps"] = record_infer(torch, philox, GaussianDiffusion, SDDM, net, cond, SCHED, nc, mode)
    np.savez_compressed(os.path.join(args.out, "tstnn.npz"), **out)
    np.savez_compressed(os.path.join(args.out, "tstnn_dt.npz"), **blk)
    with open(os.path.join(args.out, "tstnn_keys.json"), "w") as f:
        json.dump([[k, list(s)] for k, s in shapes.items()], f, indent=0)
    with open(os.path.join(args.out, "reference_config_tstnn.json"), "w") as f:
        json.dump(cfg, f, indent=4)
        f.write("\n")
    for name in ("tstnn.npz", "tstnn_dt.npz"):
        size = os.path.getsize(os.path.join(args.out, name))
        assert size < 1000000, size
        print("wrote", os.path.join(args.out, name), size, "bytes")


if __name__ == "__main__":
    main()
