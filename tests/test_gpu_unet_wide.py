"""GPU: UNetModified2 with wide levels (channel_mults [1, 2, 4, 8], res_blocks 1) in float32, the
facades' default dtype.  Its 256-channel convs with a res_conv, and the 512-channel concatenations of the
decoder, do not fit the whole-K kernel (conv_deep) in float32: before the K-chunked kernel (conv_wide.hip)
the plan failed with `no tile for downs.7`.  Checked against the numpy oracle (oracle/unet.py) at N = 2112
and N = 3136 (bottom levels of 2 x 8 and 3 x 8, level 3 of 4 x 16 and 6 x 16), B = 2, bar 1e-4 x gate; the
profiled op list names the kernel on the layers that used to fail; rows are bit-identical in two parts.

Measured on MI355X: rms against the oracle 1.02e-6 (N = 2112, output rms 0.552) and 1.06e-6 (N = 3136, 0.584).
"""
import functools

import numpy as np
import pytest
import torch

from _helpers import rms
from _weights import make_params, unet_shapes
from oracle import unet

pytestmark = pytest.mark.gpu

ARGS = dict(in_channel=2, out_channel=1, inner_channel=32, norm_groups=32, channel_mults=[1, 2, 4, 8], res_blocks=1,
            dropout=0, segment_len=128, segment_stride=64)
WIDE_LAYERS = ("downs.7.block2", "ups.0.block2", "ups.2.block1", "ups.2.block2")   # the float32 plan's, at both lengths
_NETS = {}


def _arch(N):
    return unet.architecture(N, inner_channel=32, channel_mults=(1, 2, 4, 8), res_blocks=1)


@functools.lru_cache(maxsize=None)
def _params(N):
    return make_params(unet_shapes(_arch(N)), 0)


def _net(N):
    if N not in _NETS:
        import model.network as NW
        n = NW.UNetModified2(num_samples=N, **ARGS)
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _params(N).items()})
        _NETS[N] = n.cuda()
    return _NETS[N]


def _inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    cond = np.clip(0.3 * rng.standard_normal((B, 1, N)), -1, 1).astype(np.float32)
    return cond, rng.standard_normal((B, 1, N)).astype(np.float32), rng.uniform(0.05, 0.99, B).astype(np.float32)


@pytest.mark.parametrize("N", [2112, 3136])
def test_wide_float32_forward_matches_oracle(torch_cuda, N):
    cond, x_t, nl = _inputs(2, N, seed=31)
    ref = unet.forward(_params(N), _arch(N), cond, x_t, nl)
    net = _net(N)
    assert net.compute_dtype == "float32"
    eps = net(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), torch.from_numpy(nl).cuda()).cpu().numpy()
    err = rms(eps, ref)
    print(f"UNetModified2 [1, 2, 4, 8] float32 B=2 N={N}: rms vs oracle {err:.3e} (ref rms {rms(ref, 0):.3f})")
    assert eps.shape == (2, 1, N) and np.isfinite(eps).all() and err <= 1e-4 * max(1.0, rms(ref, 0))


def test_profiled_ops_name_the_wide_kernel(torch_cuda):
    net = _net(2112)
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(2, 2112, seed=31))
    ctx = net._context(cond.device)
    ctx.profile(True)
    out = torch.empty_like(x_t)
    ctx.network_forward(cond, x_t, nl, out)
    torch.cuda.synchronize()
    ops = ctx.profile_ops()
    ctx.profile(False)
    wide = {o["name"]: o for o in ops if "[wide" in o["name"]}
    assert sorted(n.split("[")[0] for n in wide) == sorted(WIDE_LAYERS)
    for o in wide.values():
        assert o["kernel"].startswith("conv_wide_kernel<f32,") and o["launches"] == 1 and o["avg_ms"] > 0
    assert torch.equal(out, net(cond, x_t, nl))          # profiling changes no result


def test_wide_rows_in_two_parts(torch_cuda):
    """A B = 5 float32 forward equals its rows 0-1 and 2-4 run on their own, bit for bit."""
    n = _net(3136)
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in _inputs(5, 3136, seed=2))
    full = n(cond, x_t, nl)
    parts = [n(cond[s].contiguous(), x_t[s].contiguous(), nl[s].contiguous()) for s in (slice(0, 2), slice(2, 5))]
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat(parts))
