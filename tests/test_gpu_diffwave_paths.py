"""GPU: the 16-bit DiffWave layer kernels (dw_layer_pp_kernel, dw_layer_chain_kernel,
dw_skip_head_kernel; csrc/diffwave.hip) pinned bit for bit and per 128-sample tile.

A. Launch paths against each other.  The GEMM group of the ping-pong and dilation-chain kernels
   (dw_tile_gate / dw_tile_out) has the K order, MFMA sequence, gate expression and epilogue of the
   one-phase dw_layer_kernel<T, true> (SDDM_DW_NOPP=1), so the shipped path must equal the one-phase
   path bit for bit: a staging index, ring slot or barrier error has no tolerance to hide in.  The
   knobs are read once per process, so every knob set is a fresh child interpreter
   (_dw_paths_child.py), spawned once per module.  fw_many batches make a block of the chain kernel
   take a second segment (B x segments per clip > CU count; asserted, so the coverage cannot lapse
   on a part with more CUs).
B. Per-tile bound of the 16-bit arithmetic: per 128-sample tile, rms(tile error) / rms(ref row)
   against the numpy oracle, gated at 2 x the worst tile of the oracle with the kernels' storage
   roundings (_dw_emul.Emul) -- the yardstick is computed on every run.  The GPU adds its fp32
   accumulation order and exp2 / rcp gate activations on top of that rounding; noise of a 30-layer
   sum over 128 samples is stable to tens of percent, a misplaced tap image changes a tile by the
   order of its signal.
C. Sampling values: T = 50 reverse steps in 16 bits against the HIP fp32 path, gated at 2 x the same
   distance between the emulation and the oracle (Philox noise is common to all four runs).

Measured on MI355X (DESIGN.md section 4 has the commit): worst GPU tile / E of B 0.999 (bfloat16)
and 0.958 (float16); drift / D of C 1.006 and 0.986; every pair of A bit-equal; unfused against fused
head 2.98e-8 at most.
"""
import functools
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import _dw_paths_child as child
from _dw_emul import Emul
from _helpers import diffwave_params, rms

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KNOB_NAMES = ("SDDM_DW_NOPP", "SDDM_DW_NOCHAIN", "SDDM_DW_CHSEG", "SDDM_DW_NOFUSE", "SDDM_DW_NOPRE")

DEFAULT = ()
NOPP = (("SDDM_DW_NOPP", "1"),)
NOCHAIN = (("SDDM_DW_NOCHAIN", "1"),)
CHSEG8 = (("SDDM_DW_CHSEG", "8"),)
CHSEG16 = (("SDDM_DW_CHSEG", "16"),)
NOFUSE = (("SDDM_DW_NOFUSE", "1"),)
# what each child runs beyond the fw and sample cases, and its time limit: interpreter start-up and
# library load dominate (tens of seconds); a fw_many batch adds a 72 x 63-frame forward and its copies
EXTRAS = {DEFAULT: "many32,f32", NOPP: "many32,many8", NOCHAIN: "", CHSEG8: "many8", CHSEG16: "many32", NOFUSE: ""}
TIMEOUT = {DEFAULT: 300, NOPP: 300, NOCHAIN: 180, CHSEG8: 240, CHSEG16: 240, NOFUSE: 180}
_FAILED = []          # reason of the first child that faulted, aborted or hung: nothing of the module runs after it
_CHILD_ERRORS = {}    # knob set -> reason of an ordinary child failure (an exception): that child is not started again
# a GPU fault that reached the child as a Python exception (exit status 1) counts as a fault
_FAULT_WORDS = ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR", "hipErrorLaunchFailure",
                "hipErrorIllegalAddress", "unspecified launch failure")


@pytest.fixture(autouse=True)
def _nothing_runs_after_a_faulted_child():
    """Once a child died by a signal, exited 134 / 139, reported a GPU fault or hit its time limit, every
    later test of the module -- the in-process ones, which launch the same kernels, included -- fails
    with that child's reason before it touches the GPU."""
    _check_not_faulted()


def _check_not_faulted():
    if _FAILED:
        pytest.fail("not run: " + _FAILED[0])


@functools.lru_cache(maxsize=None)
def _spawn(knobs):
    env = {k: v for k, v in os.environ.items() if k not in KNOB_NAMES}
    env.update(dict(knobs))
    tmp = tempfile.mkdtemp(prefix="dw_paths_")
    out = os.path.join(tmp, "out.npz")
    name = " ".join(f"{k}={v}" for k, v in knobs) or "default"
    try:
        try:
            r = subprocess.run([sys.executable, os.path.join(HERE, "_dw_paths_child.py"), out, EXTRAS[knobs]],
                               env=env, timeout=TIMEOUT[knobs], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        except subprocess.TimeoutExpired:
            _FAILED.append(f"child [{name}] was killed at its {TIMEOUT[knobs]} s limit")
            pytest.fail(_FAILED[0])
        if r.returncode != 0:
            how = f"signal {-r.returncode}" if r.returncode < 0 else f"exit status {r.returncode}"
            reason = f"child [{name}] ended with {how}:\n{r.stdout[-2000:]}"
            if r.returncode < 0 or r.returncode in (134, 139) or any(w in r.stdout for w in _FAULT_WORDS):
                _FAILED.append(reason)
            else:
                _CHILD_ERRORS[knobs] = reason
            pytest.fail(reason)
        with np.load(out, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _run(knobs):
    """The arrays of one knob set.  After a faulted child every call fails with that child's reason; a
    child that failed in an ordinary way fails each test that needs it, and is not started again."""
    _check_not_faulted()
    if knobs in _CHILD_ERRORS:
        pytest.fail(_CHILD_ERRORS[knobs])
    return _spawn(knobs)


def segments_per_clip(F, d, seg):
    """dw_layer_chain_kernel's segment count: chain rho of the R = d / 128 chains of a clip has
    ceil((tpc - rho) / R) tiles, walked in segments of seg tiles."""
    tpc, R = -(-256 * F // 128), d // 128
    return sum(-(-(-(-(tpc - rho) // R)) // seg) for rho in range(min(R, tpc)))


def _assert_second_segment(kind, seg, ncu):
    B = child.many_batch(kind, ncu)
    for d in (128, 256, 512):
        nseg = B * segments_per_clip(child.F_MANY, d, seg)
        assert nseg > ncu, f"d={d}: {nseg} segments on {ncu} CUs: no block takes a second segment"
    return B


def _assert_bit_equal(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        if not np.array_equal(a[k], b[k]):
            diff = a[k] != b[k]
            rows = np.unique(np.nonzero(diff)[0])
            tiles = np.unique(np.nonzero(diff)[-1] // 128)
            pytest.fail(f"{what}: {k} differs in {diff.sum()} of {diff.size} values, max |diff| "
                        f"{np.abs(a[k] - b[k]).max():.3e}; rows {rows[:8].tolist()}, 128-sample tiles {tiles[:16].tolist()}")


def _common_keys(*extra):
    keys = [f"fw/{dt}/{B}x{F}" for dt in child.DTYPES for B, F in child.FW_CASES]
    return keys + [f"sample/{dt}" for dt in child.DTYPES] + list(extra)


# ---------------- A. launch paths ----------------
def test_shipped_path_equals_one_phase_kernel(torch_cuda):
    """Default launch plan (ping-pong for d <= 64, chains of 32-tile segments for d >= 128) == one-phase
    kernel on every forward, the 72-clip batch (second segment per block) and T = 200 sampling."""
    a, b = _run(DEFAULT), _run(NOPP)
    B = _assert_second_segment("many32", 32, int(a["ncu"]))
    assert a["many/many32"].shape == (B, 1, 256 * child.F_MANY)
    _assert_bit_equal(a, b, _common_keys("many/many32"), "default vs SDDM_DW_NOPP")


def test_ping_pong_at_large_dilations_equals_one_phase_kernel(torch_cuda):
    """SDDM_DW_NOCHAIN: the ping-pong kernel with three disjoint tap images at d >= 128."""
    _assert_bit_equal(_run(NOCHAIN), _run(NOPP), _common_keys(), "SDDM_DW_NOCHAIN vs SDDM_DW_NOPP")


@pytest.mark.parametrize("knobs,seg,kind", [(CHSEG8, 8, "many8"), (CHSEG16, 16, "many32")], ids=["8", "16"])
def test_chain_segment_lengths_equal_one_phase_kernel(torch_cuda, knobs, seg, kind):
    """The 8- and 16-tile instantiations of dw_layer_chain_kernel, each on a batch at which a block
    takes a second segment."""
    a, b = _run(knobs), _run(NOPP)
    _assert_second_segment(kind, seg, int(a["ncu"]))
    _assert_bit_equal(a, b, _common_keys(f"many/{kind}"), f"SDDM_DW_CHSEG={seg} vs SDDM_DW_NOPP")


def test_unfused_head_matches_fused_head(torch_cuda):
    """SDDM_DW_NOFUSE (dw_skip_kernel, fp32 skip rows through HBM, dw_output_kernel) against the fused
    dw_skip_head_kernel.  Both read the same 16-bit z; the skip GEMM has the same K order, and
    skip_projection sums its 64 terms (and output_projection its 64) in another fp32 order: per
    element within the project's fp32 bar, 1e-4 max(1, rms(row)), in max norm.  The bar is asserted on
    every forward.  The 200-step sampling figure is informational (printed, finiteness and shape
    asserted): the two-sums argument bounds one forward, not its propagation through 200 clipped
    steps, and a bound taken from the measured figure would be no bound."""
    a, b = _run(NOFUSE), _run(DEFAULT)
    worst = 0.0
    for k in _common_keys():
        assert a[k].shape == b[k].shape and np.isfinite(a[k]).all(), k
        diff = np.abs(a[k].astype(np.float64) - b[k]).reshape(a[k].shape[0], -1).max(axis=1)
        if k.startswith("sample/"):
            print(f"{k}: unfused vs fused head after 200 steps, max |diff| {diff.max():.3e}")
            continue
        bar = np.array([1e-4 * max(1.0, rms(row, 0)) for row in b[k]])
        worst = max(worst, float(diff.max()))
        print(f"{k}: max |diff| {diff.max():.3e} (bar {bar.min():.1e})")
        assert (diff <= bar).all(), k
    print(f"unfused vs fused head, one forward: max |diff| {worst:.3e}")


def test_many_clip_batch_matches_oracle(torch_cuda):
    """Rows of the 72-clip batch (blocks with a second chain segment) against the numpy oracle."""
    from oracle import diffwave as odw
    a = _run(DEFAULT)
    B = child.many_batch("many32", int(a["ncu"]))
    spec, audio, steps = child.dw_rows(B, child.F_MANY, child.many_seed("many32"))
    rows = [0, B // 2, B - 9, B - 1]
    ref = odw.forward(diffwave_params(), spec[rows], audio[rows], steps[rows])
    eps = a["many/many32"]
    for i, b in enumerate(rows):
        err = rms(eps[b], ref[i])
        print(f"bf16 B={B} row {b}: rms {err:.3e}, worst tile {_tile_ratio(eps[b:b + 1], ref[i:i + 1]).max():.3e} of the row rms")
        assert err <= 3e-2 * max(1.0, rms(ref[i], 0))


def test_sampling_63_frames_is_finite(torch_cuda):
    """T = 200 at config #3's clip length: gated by bit equality with the one-phase path (above) and
    finiteness; no CPU yardstick is affordable here.  The drift from the fp32 HIP path is printed."""
    a = _run(DEFAULT)
    for dt in child.DTYPES:
        x = a[f"sample/{dt}"]
        assert x.shape == (child.SAMPLE_SHAPE[0], 1, 256 * child.SAMPLE_SHAPE[1]) and np.isfinite(x).all()
        print(f"T=200, 63 frames: rms({dt} - fp32 HIP) {rms(x, a['sample/float32']):.3e} (rms of the fp32 output "
              f"{rms(a['sample/float32'], 0):.3f})")


# ---------------- B / C: in-process, default path ----------------
def _net(dtype):
    import model.network as NW
    _check_not_faulted()
    assert not any(k in os.environ for k in KNOB_NAMES), "the in-process tests measure the default launch plan"
    n = NW.DiffWave(num_samples=-1, num_timesteps=3, freq_bins=513, residual_channels=64, residual_layers=30,
                    dilation_cycle_length=10)
    n.load_state_dict({k: torch.from_numpy(v) for k, v in diffwave_params().items()})
    n.compute_dtype = dtype
    return n.cuda()


def _tile_ratio(x, ref):
    """[B, tiles]: rms of the error over each 128-sample tile / rms of the reference row."""
    B = ref.shape[0]
    e = (x.astype(np.float64) - ref).reshape(B, -1, 128)
    row = np.sqrt(np.mean(ref.astype(np.float64).reshape(B, -1) ** 2, axis=1))
    return np.sqrt(np.mean(e ** 2, axis=-1)) / row[:, None]


TILE_B, TILE_F = 1, 40      # 80 tiles: a d = 128 chain has segments of 32, 32 and 16 tiles


@functools.lru_cache(maxsize=None)
def _tile_case():
    from oracle import diffwave as odw
    rows = child.dw_rows(TILE_B, TILE_F, 51)
    return rows, odw.forward(diffwave_params(), *rows)


@pytest.mark.parametrize("dtype", child.DTYPES)
def test_per_tile_error_within_twice_the_storage_rounding(torch_cuda, dtype):
    (spec, audio, steps), ref = _tile_case()
    e = _tile_ratio(Emul(diffwave_params(), dtype)(spec, audio, steps), ref)
    g = _tile_ratio(_net(dtype)(torch.from_numpy(spec).cuda(), torch.from_numpy(audio).cuda(),
                                torch.from_numpy(steps).reshape(-1, 1, 1).cuda()).cpu().numpy(), ref)
    E = float(e.max())
    print(f"{dtype}: emulation tiles max {E:.3e} median {np.median(e):.3e}; GPU tiles max {g.max():.3e} median "
          f"{np.median(g):.3e}; worst GPU tile / E = {g.max() / E:.3f} at tile {int(g.argmax())} of {g.size}")
    assert E > 0 and np.isfinite(g).all()
    bad = np.nonzero(g[0] > 2 * E)[0]
    assert bad.size == 0, f"tiles {bad.tolist()} above 2 E: {(g[0][bad] / E).round(2).tolist()}"


SAMPLE_SCHED = ("linear", 50, 1e-4, 0.02)


@functools.lru_cache(maxsize=None)
def _sample_case():
    from oracle import sampler, schedule
    spec = child.dw_rows(2, 2, 52)[0]
    tab = schedule.make_tables(*SAMPLE_SCHED)
    emul = lambda dtype: sampler.infer_spectrogram(Emul(diffwave_params(), dtype), tab, spec, 256,
                                                   noise_condition="time_step", seed=7)
    return spec, emul, emul(None), _gpu_sample(spec, "float32")


def _gpu_sample(spec, dtype):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SAMPLE_SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, _net(dtype), hop_samples=256, noise_condition="time_step", compute_dtype=dtype).cuda()
    return m.infer(torch.from_numpy(spec).cuda(), seed=7).cpu().numpy()


@pytest.mark.parametrize("dtype", child.DTYPES)
def test_sampling_drift_within_twice_the_storage_rounding(torch_cuda, dtype):
    """50 reverse steps at (2, 513, 2): rms(16-bit HIP - fp32 HIP) <= 2 rms(emulation - oracle), the
    layer kernels taking the diffusion projection from the device-side step (t_dev).  (The three CPU
    sampling runs of the module take about 6 s each, so T stays at 50.)"""
    spec, emul, e32, g32 = _sample_case()
    D = rms(emul(dtype), e32)
    g16 = _gpu_sample(spec, dtype)
    drift = rms(g16, g32)
    print(f"{dtype}: rms(gpu16 - gpu32) {drift:.3e}, D = rms(emul16 - emul32) {D:.3e}, ratio {drift / D:.3f}; "
          f"rms(gpu32 - oracle) {rms(g32, e32):.3e}")
    assert np.isfinite(g16).all() and D > 0
    assert drift <= 2 * D
