"""The UNet kernels' output bits, pinned across changes of how activations are stored.

How a kernel writes its output tile (plain or write-through stores, 8 or 16 bytes per lane, which
lane holds which channel) moves whole elements and touches no arithmetic, so every output must
stay bit-identical.  tests/golden/unet_store_digests.json holds SHA-256 digests of the outputs
below, recorded on the GPU with the library of the commit before the store flavours were
introduced (tools/record_store_digests.py); every case asserts digest equality (each runs in
well under a second on an MI355X):
  fw2112/<dtype>/heuristic      forward, B=2 x N=2112, the plan the heuristic picks
  fw2112/<dtype>/<table>        the same forward on the forced per-layer tables of test_gpu_unet.py
                                 (every tile configuration, 16- and 64-channel deep blocks): generic
                                 kernels, odd-fragment blocks, image-edge tiles.  The launchers
                                 refuse the chain table and fp32 64-channel deep blocks at this size
                                 ("invalid argument", before and after this change), so those three
                                 combinations run at the bench shape only
  fw16448/<dtype>/<table>       B=16 x N=16448 on the forced tables and on the repository's measured
                                 table: every compile-time-shape kernel
  sample2112/bfloat16/graph4    4 graph-replayed sampling steps, B=2 x N=2112
"""
import hashlib
import json
import os

import numpy as np
import pytest

import test_gpu_unet as tu
from _helpers import GOLDEN, golden

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(GOLDEN, "unet_store_digests.json")
_TABLES = {"table": tu._TUNING, "table16": tu._TUNING16, "table16gn": tu._TUNING16_GN, "table64": tu._TUNING64,
           "chain": tu._CHAIN}

CASES = (
    [f"fw2112/{d}/heuristic" for d in ("float32", "bfloat16", "float16")]
    + [f"fw2112/{d}/{t}" for d in ("float32", "bfloat16", "float16") for t in ("table", "table16", "table64")
       if (d, t) != ("float32", "table64")]
    + [f"fw16448/{d}/{t}" for d, t in (("bfloat16", "table"), ("bfloat16", "table16"), ("float32", "table16"),
                                      ("bfloat16", "table16gn"), ("bfloat16", "table64"), ("float16", "table64"),
                                      ("bfloat16", "chain"), ("float16", "chain"), ("bfloat16", "repo"),
                                      ("float16", "repo"))]
    + ["sample2112/bfloat16/graph4"]
)

_INPUTS = {}


def _inputs16448():
    """16 distinct rows of the bench shape at 16 noise levels (the inputs of test_gpu_unet.bench_rows,
    without its numpy-oracle forward)."""
    if "big" not in _INPUTS:
        from oracle import schedule as osched
        from sddm_hip.synth import noisy_speech
        N, B = 16448, 16
        tab = osched.make_tables("linear", 1000, 1e-6, 1e-3)
        nl = tab["sqrt_alpha_bar"][np.linspace(1000, 1, B).round().astype(int)].astype(np.float32)
        cond = noisy_speech(B, N, seed=21)
        z = np.random.default_rng(22).standard_normal((B, 1, N)).astype(np.float32)
        x_t = (nl[:, None, None] * cond + np.sqrt(1 - nl[:, None, None] ** 2) * z).astype(np.float32)
        _INPUTS["big"] = (cond, x_t, nl)
    return _INPUTS["big"]


def digest(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_case(torch, case):
    """The output array of one case (fp32 on the host)."""
    shape, dtype, what = case.split("/")
    dev = torch.device("cuda", 0)
    if shape == "sample2112":
        from sddm_hip.synth import noisy_speech
        ctx = tu.make_ctx(2112, dtype, ("linear", 4, 1e-6, 1e-3))
        return tu._sample(torch, ctx, noisy_speech(2, 2112, seed=99))
    N = int(shape[2:])
    ctx = tu.make_ctx(N, dtype)
    if what == "repo":
        text, tab = tu.repo_tuning_table(N, 16)
        assert tab is not None, "no measured table for the bench geometry"
        ctx.set_conv_tuning(text)
    elif what != "heuristic":
        ctx.set_conv_tuning({"lane_batch": 16, "dtype": dtype, "num_samples": N, "kernel": _TABLES[what]})
    if N == 2112:
        return tu._forward(torch, ctx, golden("unet_forward.npz"), N)
    cond, x_t, nl = _inputs16448()
    eps = torch.full((cond.shape[0], 1, N), float("nan"), device=dev)
    ctx.network_forward(torch.from_numpy(cond).to(dev), torch.from_numpy(x_t).to(dev), torch.from_numpy(nl).to(dev), eps)
    torch.cuda.synchronize()
    return eps.cpu().numpy()


@pytest.mark.parametrize("case", CASES)
def test_output_digest_is_pinned(torch_cuda, case):
    pinned = json.load(open(FIXTURE))["digests"]
    out = run_case(torch_cuda, case)
    assert np.isfinite(out).all()
    got = digest(out)
    print(f"{case}: {got[:16]} (pinned {pinned[case][:16]})")
    assert got == pinned[case]
