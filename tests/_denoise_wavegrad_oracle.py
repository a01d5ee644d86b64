"""ORACLE (test infrastructure only) -- DenoiseWaveGrad1 / DenoiseWaveGrad3 forward in numpy.

Restates the two waveform-conditioned networks of the reference's model/wavegrad.py (184-242 and
307-353) from the primitives of ``oracle.wavegrad`` (conv1d / leaky / up / down / encoding, film,
ublock): same float64 accumulation, float32 rounding per layer.  Weights: dict of numpy arrays keyed
like the reference state_dict without the ``noise_estimate_model.`` prefix.
"""
import numpy as np

from oracle import wavegrad as wg

FILM = wg.FILM
NETS = {
    "DenoiseWaveGrad1": dict(
        hop=400, stem_ci=1,
        down=[(1, 32, None), (32, 128, 2), (128, 128, 2), (128, 256, 4), (256, 512, 5)],
        up=[(512, 512, 5, (1, 2, 1, 2)), (512, 512, 5, (1, 2, 1, 2)), (512, 256, 4, (1, 2, 4, 8)),
            (256, 128, 2, (1, 2, 4, 8)), (128, 128, 2, (1, 2, 4, 8))]),
    "DenoiseWaveGrad3": dict(
        hop=300, stem_ci=2,
        down=[(2, 32, None), (32, 128, 2), (128, 128, 2), (128, 256, 3), (256, 512, 5)],
        up=[(512, 512, 5, (1, 2, 1, 2)), (512, 512, 5, (1, 2, 1, 2)), (512, 256, 3, (1, 2, 4, 8)),
            (256, 128, 2, (1, 2, 4, 8)), (128, 128, 2, (1, 2, 4, 8))]),
}
BOTTOM = (512, 512, 5)          # downsample_x.5 (wavegrad.py:207) / bottleneck (wavegrad.py:323)


def dblock(P, p, x, f):
    """DBlock with key prefix p (wavegrad.py:126-137)."""
    res = wg.down(wg.conv1d(x, P[p + "residual_dense.weight"], P[p + "residual_dense.bias"]), f)
    x = wg.down(x, f)
    for j, d in enumerate((1, 2, 4)):
        x = wg.conv1d(wg.leaky(x), P[p + f"conv.{j}.weight"], P[p + f"conv.{j}.bias"], d)
    return (x + res).astype(np.float32)


def _ladder(P, prefix, net, x, noise_level=None):
    """Stem + 4 DBlocks under `prefix`; with a noise level also the FiLM of every level."""
    films = []
    for i, (_, _, f) in enumerate(net["down"]):
        if f is None:
            x = wg.conv1d(x, P[f"{prefix}.0.weight"], P[f"{prefix}.0.bias"])
        else:
            x = dblock(P, f"{prefix}.{i}.", x, f)
        if noise_level is not None:
            films.append(wg.film(P, i, x, noise_level))
    return x, films


def _decode(P, net, x, films):
    for i, (_, _, f, dil) in enumerate(net["up"]):
        shift, scale = films[len(films) - 1 - i]
        x = wg.ublock(P, i, x, shift, scale, f, dil)
    return wg.conv1d(x, P["last_conv.weight"], P["last_conv.bias"])


def forward(name, P, x, y_t, noise_level):
    """forward(x, y_t, noise_level) of the named network: x, y_t [B, 1, N], noise level [B] -> [B, 1, N]."""
    net = NETS[name]
    x = np.asarray(x, np.float32).reshape(len(x), 1, -1)
    y_t = np.asarray(y_t, np.float32).reshape(len(y_t), 1, -1)
    nl = np.asarray(noise_level, np.float32).reshape(-1)
    assert x.shape == y_t.shape and x.shape[2] % net["hop"] == 0 and x.shape[2] >= net["hop"]
    if name == "DenoiseWaveGrad1":                                   # wavegrad.py:226-242
        _, films = _ladder(P, "downsample", net, y_t, nl)
        h, _ = _ladder(P, "downsample_x", net, x)
        h = dblock(P, "downsample_x.5.", h, BOTTOM[2])
    else:                                                            # wavegrad.py:341-353
        h, films = _ladder(P, "downsample", net, np.concatenate([y_t, x], axis=1), nl)
        h = dblock(P, "bottleneck.", h, BOTTOM[2])
    return _decode(P, net, h, films)


def param_shapes(name):
    """State-dict shapes of the named network without the module prefix."""
    net = NETS[name]
    s = {}

    def conv(p, co, ci, k):
        s[p + ".weight"], s[p + ".bias"] = (co, ci, k), (co,)

    def db(p, ci, co):
        conv(p + "residual_dense", co, ci, 1)
        for j, c in enumerate((ci, co, co)):
            conv(p + f"conv.{j}", co, c, 3)

    conv("downsample.0", 32, net["stem_ci"], 5)
    for i, (ci, co, _) in enumerate(net["down"][1:], 1):
        db(f"downsample.{i}.", ci, co)
    if name == "DenoiseWaveGrad1":
        conv("downsample_x.0", 32, 1, 5)
        for i, (ci, co, _) in enumerate(net["down"][1:], 1):
            db(f"downsample_x.{i}.", ci, co)
        db("downsample_x.5.", BOTTOM[0], BOTTOM[1])
    else:
        db("bottleneck.", BOTTOM[0], BOTTOM[1])
    for i, (ci, co) in enumerate(FILM):
        conv(f"film.{i}.input_conv", ci, ci, 3)
        conv(f"film.{i}.output_conv", 2 * co, ci, 3)
    for i, (ci, h, _, _) in enumerate(net["up"]):
        p = f"upsample.{i}."
        conv(p + "block1", h, ci, 1)
        conv(p + "block2.0", h, ci, 3)
        for k in ("block2.1", "block3.0", "block3.1"):
            conv(p + k, h, h, 3)
    conv("last_conv", 1, 128, 3)
    return s
