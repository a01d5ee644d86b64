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

The cases below were appended (and recorded with the parent's library; that recording reproduced the
22 above) before the UNet runtime moved out of sddm_runtime.cpp into unet_runtime.h: the branches of
the lane path and the UNetTST plan that the first 22 do not reach.  N = 2112 (every level down to
1 x 4), T = 4 where sampling:
  sample2112/bfloat16/record    sample_continuous, sample_inter 2, B=2: out, then the two recorded
                                 states (the per-launch loop, no graph)
  sample2112/float32/noise      sample_noise with seeded draws [5][2][1][2112] (per-launch as well)
  sample2112/bfloat16/lanes     B=5 under "lane_rows": 2: three lanes, the last one partial, on three
                                 streams, graph replay (SDDM_LANE_ROWS unset)
  tst2112/<dtype>/fw            UNetTST (_unettst_oracle.ARGS), forward at B=2
  tst2112/bfloat16/graph4       UNetTST, 4 graph-replayed sampling steps, B=2
  tst2112/float32/res2          UNetTST forward with res_blocks 2: the concatenation step of the plan
  tst/<dtype>/dt                Context.dual_transformer on [2, 160, 2, 4] where only mid.* is loaded
                                 (every other parameter packs as zeros)
"""
import hashlib
import json
import os

import numpy as np
import pytest

import _unettst_oracle as TO
import test_gpu_unet as tu
from _helpers import GOLDEN, golden, unet_config
from _weights import make_params

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
    # appended behind the first 22, whose names and order stay
    + ["sample2112/bfloat16/record", "sample2112/float32/noise", "sample2112/bfloat16/lanes"]
    + [f"tst2112/{d}/fw" for d in ("float32", "bfloat16", "float16")]
    + ["tst2112/bfloat16/graph4", "tst2112/float32/res2"]
    + [f"tst/{d}/dt" for d in ("float32", "bfloat16")]
)
SCHED4 = ("linear", 4, 1e-6, 1e-3)

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


def _tst_ctx(dtype, sched=("linear", 100, 1e-6, 1e-3), only=None, lane_rows=None, **change):
    """A UNetTST context at N = 2112; `only`: load just the parameters with that prefix."""
    import sddm_hip
    args = dict(TO.ARGS, **change)
    cfg = unet_config(2112, sched)
    cfg["network"] = {"type": "UNetTST", "args": args}
    ctx = sddm_hip.Context(cfg, 0, dtype)
    P = make_params(TO.param_shapes(args), 0)
    ctx.load_state_dict({k: v for k, v in P.items() if only is None or k.startswith(only)})
    assert (ctx.missing() == 0) == (only is None)
    return ctx


def _sample_case(torch, ctx, what):
    """sampling at N = 2112, T = 4: graph4 and lanes replay graphs, record and noise launch per step."""
    from sddm_hip.synth import noisy_speech
    dev = torch.device("cuda", 0)
    rows = 5 if what == "lanes" else 2
    cond_np = noisy_speech(rows, 2112, seed=99)
    if what in ("graph4", "lanes"):
        return tu._sample(torch, ctx, cond_np)
    cond = torch.from_numpy(cond_np).to(dev)
    out = torch.full_like(cond, float("nan"))
    if what == "record":
        record = torch.full((2,) + tuple(cond.shape), float("nan"), device=dev)
        ctx.sample_continuous(cond, out, record, 2, 7, 0)
        out = torch.cat([out[None], record])
    else:
        draws = np.random.default_rng(11).standard_normal((5, 2, 1, 2112)).astype(np.float32)
        ctx.sample_noise(cond, out, torch.from_numpy(draws).to(dev))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_case(torch, case):
    """The output array of one case (fp32 on the host)."""
    shape, dtype, what = case.split("/")
    dev = torch.device("cuda", 0)
    if shape == "sample2112":
        if what != "lanes":
            return _sample_case(torch, tu.make_ctx(2112, dtype, SCHED4), what)
        import sddm_hip
        assert "SDDM_LANE_ROWS" not in os.environ, "SDDM_LANE_ROWS overrides the config's lane_rows"
        ctx = sddm_hip.Context(dict(unet_config(2112, SCHED4), lane_rows=2), 0, dtype)
        ctx.load_state_dict(tu.unet_params(2112))
        return _sample_case(torch, ctx, what)
    if shape == "tst":
        x = np.random.default_rng(17).standard_normal((2, 160, 2, 4)).astype(np.float32)
        y = torch.full(x.shape, float("nan"), device=dev)
        _tst_ctx(dtype, only="mid.").dual_transformer(torch.from_numpy(x).to(dev), y)
        torch.cuda.synchronize()
        return y.cpu().numpy()
    if shape == "tst2112":
        if what == "graph4":
            return _sample_case(torch, _tst_ctx(dtype, SCHED4), what)
        ctx = _tst_ctx(dtype, res_blocks=2) if what == "res2" else _tst_ctx(dtype)
        return tu._forward(torch, ctx, golden("unet_forward.npz"), 2112)
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
