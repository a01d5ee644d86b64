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
MODES = ("original", "condition_in", "sr3", "supportive", "conditional")
NETS = {"DenoiseWaveGrad1": 400, "DenoiseWaveGrad3": 300}
B = 2


def clamped_share(x):
    return float(np.mean(np.abs(x) >= 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    for p in (HERE, os.path.join(REPO, "tests"), REPO):
        sys.path.insert(0, p)
    from gen_golden import NoiseInjector
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
        net = getattr(ref_wavegrad, name)()
        shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
        keys[name] = [[k, list(s)] for k, s in shapes.items()]
        P = make_params(shapes, 0)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in P.items()})
        net.eval()
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
        for nc, modes in (("sqrt_alpha_bar", MODES), ("time_step", ("original",))):
            for mode in modes:
                d = GaussianDiffusion(*SCHED, device="cpu")
                m = SDDM(d, net, noise_condition=nc, p_transition=mode).eval()
                steps = []

                def rec(fn):
                    def w(*a, **kw):
                        y = fn(*a, **kw)
                        steps.append(y.numpy().copy())
                        return y
                    return w
                for fn in ("p_transition", "p_transition_sr3", "p_transition_supportive", "p_transition_conditional"):
                    setattr(d, fn, rec(getattr(d, fn)))
                inj = NoiseInjector(torch, philox, 7)
                inj.draws = ([] if mode == "supportive" else [0]) + list(range(SCHED[1], 1, -1))
                with inj, torch.no_grad():
                    y = m.infer(torch.from_numpy(cond)).numpy().copy()
                steps = np.stack(steps)
                assert steps.shape == (SCHED[1], B, 1, N) and np.array_equal(steps[-1], y)
                assert np.isfinite(steps).all()
                shares = [clamped_share(s) for s in steps]
                # a golden that is mostly clamp values would hide errors: at most 25 % of a final
                # output sits at +-1.  The intermediate x_t are looser by construction: a run that
                # starts from x_T ~ N(0, 1) has P(|z| > 1) = 31.7 % of its samples beyond the clamp
                # before the first step ('original' / 'sr3': 0.31 after it), so they are held to the
                # x_T share plus a margin, 35 %
                assert shares[-1] <= 0.25, f"{name} {nc} {mode}: clamped share of the output {shares}"
                assert max(shares) <= 0.35, f"{name} {nc} {mode}: clamped share {shares}"
                print(f"{name} {nc} {mode}: clamped share per step {['%.3f' % s for s in shares]}", flush=True)
                out[f"{name}/inf/{nc}/{mode}/out"] = y
                out[f"{name}/inf/{nc}/{mode}/steps"] = steps
    np.savez_compressed(os.path.join(args.out, "denoise_wavegrad.npz"), **out)
    with open(os.path.join(args.out, "denoise_wavegrad_keys.json"), "w") as f:
        json.dump(keys, f, indent=0)
    print("wrote", os.path.join(args.out, "denoise_wavegrad.npz"))


if __name__ == "__main__":
    main()
