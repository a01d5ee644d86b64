"""Shared parity harness of the waveform-conditioned denoisers' GPU tests (test infrastructure).

A test_gpu_<net>.py describes its network in one NetCase, lists its parametrizations and keeps one
one-line wrapper per shared test; the bodies are the check_* functions below.  Wherever the networks'
tests assert different things the difference is a field of the case, never a branch on its name.
Per process there is at most one facade network per (case, length, dtype, variant), and every oracle
case is computed once.
"""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest
import torch

from _helpers import golden, rms, write_pcm16
from _weights import make_params

SCHED = ("linear", 3, 1e-4, 0.05)
MODES = ("original", "condition_in", "sr3", "supportive", "conditional")
SAMPLING_CASES = [("sqrt_alpha_bar", m) for m in MODES] + [("time_step", "original")]
_NETS = {}


@dataclasses.dataclass(frozen=True, eq=False)
class NetCase:
    name: str                         # the facade class in model.network, the config's network type, the printed label
    oracle: object                    # param_shapes and forward (and ARGS, unless by_name)
    golden: str                       # file under tests/golden
    golden_len: int                   # N of the golden's forward and sampling cases
    short_len: int = 0                # N of the row-sharding, row-independence and SDDM.forward tests (0: golden_len)
    key: str = ""                     # prefix of the golden's keys
    by_name: bool = False             # the oracle serves several networks: param_shapes(name), forward(name, P, ...)
    dual_transformer: bool = False    # segmented network around a Dual_Transformer: the facade is built per length
    #                                   (num_samples=N) and variant, the oracle takes args=, mid has its own compute_dtype
    rounding: bool = False            # the oracle's forward has the 16-bit emulation (rounding=); it is printed
    emulated_bar16: bool = False      # 16-bit forward bar: bar16(dtype, emulation); else the test's own tol (3e-2 / 5e-3)
    state_dict_count: int = 0         # Context.missing() before any tensor is loaded
    loads_state_dict: bool = True     # ... and the test loads the parameters and expects 0
    refusal_match: bool = False       # the NotImplementedError's message must name the refused argument
    bad_lengths: tuple = ()           # lengths the facade and SDDM.infer must refuse
    rejects_empty_batch: bool = False
    spec_hop: int = 0                 # hop_samples of the SDDM_spectrogram test
    spec_input: tuple = (1, 1, 8)     # and the shape of its input
    gated_sampling_bar: bool = False  # sampling: every x_t within 1e-4 * gate(x_t); else the output and every x_t within 1e-3
    continuous_shape: bool = True     # continuous sampling also asserts the recorded shape
    sharding_nonzero: bool = True     # row sharding also asserts a non-zero output
    sharded_infer: bool = False       # ... and that sharded_infer without a process group is model.infer
    cli_config: str = ""              # file under configs/
    cli_chunk: int = 0                # the chunk length N the test sets
    cli_lengths: tuple = ()           # the two utterances
    cli_num_samples: tuple = ()       # precondition on the config's num_samples: ("%", 8) or ("==", 16448)
    cli_exact_shape: bool = True      # output is exactly ceil(n / N) chunks; else a multiple of N that is >= n


def args(case, **variant):
    return dict(case.oracle.ARGS, **variant)


def _variant_key(case, variant):
    return tuple(sorted((k, v) for k, v in variant.items() if case.oracle.ARGS[k] != v))


@functools.lru_cache(maxsize=None)
def _params(case, vkey):
    if case.by_name:
        return make_params(case.oracle.param_shapes(case.name), 0)
    if case.dual_transformer:
        return make_params(case.oracle.param_shapes(args(case, **dict(vkey))), 0)
    return make_params(case.oracle.param_shapes(), 0)


def params(case, **variant):
    return _params(case, _variant_key(case, variant))


def net(case, N=None, dtype="float32", **variant):
    """One facade network per (case, length, dtype, variant), shared by the tests (its weights never change)."""
    vkey = _variant_key(case, variant)
    key = (case.name, N if case.dual_transformer else None, dtype, vkey)
    if key not in _NETS:
        import model.network as NW
        cls = getattr(NW, case.name)
        if case.by_name:
            n = cls()
        elif case.dual_transformer:
            n = cls(num_samples=N, **args(case, **dict(vkey)))
        else:
            n = cls(**case.oracle.ARGS)
        n.load_state_dict({k: torch.from_numpy(v) for k, v in _params(case, vkey).items()})
        n.compute_dtype = dtype
        if case.dual_transformer:
            n.mid.compute_dtype = dtype
        _NETS[key] = n.cuda()
    return _NETS[key]


def model(case, N=None, mode="original", noise_condition="sqrt_alpha_bar", dtype="float32"):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    return M.SDDM(d, net(case, N, dtype), noise_condition=noise_condition, p_transition=mode, compute_dtype=dtype).cuda()


def config(case, num_samples=None, **change):
    cfg = {"arch": {"type": "SDDM", "args": {}},
           "diffusion": {"type": "GaussianDiffusion", "args": {"schedule": "linear", "n_timestep": 3}},
           "network": {"type": case.name, "args": args(case, **change)}}
    if num_samples is not None:
        cfg["num_samples"] = num_samples
    return cfg


def inputs(B, N, seed):
    rng = np.random.default_rng(seed)
    cond = np.clip(0.3 * rng.standard_normal((B, 1, N)), -1, 1).astype(np.float32)
    x_t = rng.standard_normal((B, 1, N)).astype(np.float32)
    nl = rng.uniform(0.05, 0.99, B).astype(np.float32)
    return cond, x_t, nl


def gate(ref):
    return max(1.0, rms(ref, 0))


def bar16(dtype, emu):
    """The 16-bit bar: the project's where the CPU emulation's error is at most half of it, else twice
    the emulation's."""
    project = {"bfloat16": 3e-2, "float16": 5e-3}[dtype]
    return project if emu <= 0.5 * project else 2.0 * emu


def clamped(x):
    return float(np.mean(np.abs(x) >= 1.0))


def run(net, cond, x_t, nl):
    return net(torch.from_numpy(cond).cuda(), torch.from_numpy(x_t).cuda(), torch.from_numpy(nl).cuda()).cpu().numpy()


def oracle_forward(case, cond, x_t, nl, rounding=None, **variant):
    P = params(case, **variant)
    if case.by_name:
        return case.oracle.forward(case.name, P, cond, x_t, nl)
    kw = {} if rounding is None else {"rounding": getattr(torch, rounding)}
    if case.dual_transformer:
        kw["args"] = args(case, **variant)
    return case.oracle.forward(P, cond, x_t, nl, **kw)


@functools.lru_cache(maxsize=None)
def _oracle_case(case, B, N, vkey):
    cond, x_t, nl = inputs(B, N, seed=31)
    return cond, x_t, nl, oracle_forward(case, cond, x_t, nl, **dict(vkey))


def oracle_case(case, B, N, **variant):
    """Inputs and the oracle's output of one shape, computed once."""
    return _oracle_case(case, B, N, _variant_key(case, variant))


@functools.lru_cache(maxsize=None)
def big_case(case):
    """The config's own chunk length, B = 2: inputs and the oracle's output, computed once."""
    cond, x_t, nl = inputs(2, 16384, seed=41)
    return cond, x_t, nl, oracle_forward(case, cond, x_t, nl)


def _short(case):
    return case.short_len or case.golden_len


# ---- the shared test bodies
def check_forward_matches_reference(case, dtype, tol=1e-4):
    z = golden(case.golden)
    cond, x_t, nl = (z[f"{case.key}fw/{k}"] for k in ("cond", "x_t", "noise_level"))
    ref = z[f"{case.key}fw/eps"]
    eps = run(net(case, dtype=dtype), cond, x_t, nl)
    assert eps.shape == ref.shape
    err = rms(eps, ref)
    print(f"{case.name} {dtype}: rms vs reference {err:.3e}, relative {err / rms(ref, 0):.3e}")
    if dtype == "float32":
        assert err <= tol * gate(ref)
        return
    note = f"{case.name} {dtype}: CPU emulation (conv inputs, weights, outputs rounded) relative"
    if case.emulated_bar16:
        emu = rms(oracle_forward(case, cond, x_t, nl, rounding=dtype), ref) / rms(ref, 0)
        tol = bar16(dtype, emu)
        print(f"{note} {emu:.3e}, bar {tol:.3e}")
    elif case.rounding:
        print(f"{note} {rms(oracle_forward(case, cond, x_t, nl, rounding=dtype), ref) / rms(ref, 0):.3e}")
    assert err / rms(ref, 0) <= tol


def check_forward_16bit_at_the_config_length(case, dtype, tol=None):
    cond, x_t, nl, ref = big_case(case)
    assert clamped(ref) <= 0.25
    rel = rms(run(net(case, dtype=dtype), cond, x_t, nl), ref) / rms(ref, 0)
    head = f"{case.name} {dtype} B=2 N=16384: relative rms vs oracle {rel:.3e}"
    if case.rounding:
        emu = rms(oracle_forward(case, cond, x_t, nl, rounding=dtype), ref) / rms(ref, 0)
    if case.emulated_bar16:
        tol = bar16(dtype, emu)
        print(f"{head} (CPU emulation {emu:.3e}, bar {tol:.3e})")
    else:
        print(f"{head} (CPU emulation {emu:.3e})" if case.rounding else head)
    assert rel <= tol


def check_sampling_matches_reference(case, nc, mode):
    """The reference's unmodified SDDM.infer: the output and every intermediate x_t; a second run is
    bit-equal.  (Where a golden stores the output as .../out too, it is steps[-1] bit for bit.)"""
    z = golden(case.golden)
    steps = z[f"{case.key}inf/{nc}/{mode}/steps"]
    cond = torch.from_numpy(z[f"{case.key}inf/cond"]).cuda()
    m = model(case, case.golden_len, mode, nc)
    out = m.infer(cond, seed=7).cpu().numpy()
    assert out.shape == steps[-1].shape
    T = SCHED[1]
    record = torch.empty((T,) + tuple(cond.shape), dtype=torch.float32, device="cuda")
    out2 = torch.empty_like(cond)
    m._context(cond.device).sample_continuous(cond, out2, record, 1, 7, 0)
    errs = [rms(record[i].cpu().numpy(), steps[i]) for i in range(T)]
    if case.gated_sampling_bar:
        print(f"{case.name} {nc} {mode}: rms of x_t per step {['%.2e' % e for e in errs]}")
        for e, s in zip(errs, steps):
            assert e <= 1e-4 * gate(s)
    else:
        err = rms(out, steps[-1])
        print(f"{case.name} {nc} {mode}: rms of the output {err:.3e}, of x_t per step {['%.2e' % e for e in errs]}")
        assert err <= 1e-3
        assert max(errs) <= 1e-3
    assert torch.equal(out2.cpu(), torch.from_numpy(out))


def check_continuous_sampling_single_clip(case):
    z = golden(case.golden)
    cond = torch.from_numpy(z[f"{case.key}inf/cond"][:1]).cuda()
    rec = model(case, case.golden_len, "sr3").infer(cond, continuous=True, seed=7)
    assert len(rec) == 1 + SCHED[1]
    assert torch.equal(rec[0], cond)
    got = np.stack([r.cpu().numpy() for r in rec[1:]])
    if case.continuous_shape:
        assert got.shape[1:] == (1, 1, case.golden_len)
    assert rms(got, z[f"{case.key}inf/sqrt_alpha_bar/sr3/steps"][:, :1]) <= 1e-3


def check_row_sharding(case):
    """Rows sampled in two shards (row_offset) equal the rows of one batch."""
    m = model(case, _short(case), "conditional", dtype="bfloat16")
    cond = torch.from_numpy(inputs(4, _short(case), seed=1)[0]).cuda()
    full = m.infer(cond, seed=11)
    a = m.infer(cond[:2].contiguous(), seed=11, row_offset=0)
    b = m.infer(cond[2:].contiguous(), seed=11, row_offset=2)
    assert torch.isfinite(full).all()
    if case.sharding_nonzero:
        assert float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat([a, b]))
    if case.sharded_infer:
        import model.model as M
        assert torch.equal(M.sharded_infer(m, cond, seed=11), full)


def check_rows_in_two_parts(case):
    """A B = 5 forward equals its rows 0-1 and 2-4 run on their own, bit for bit (bfloat16)."""
    n = net(case, dtype="bfloat16")
    cond, x_t, nl = (torch.from_numpy(a).cuda() for a in inputs(5, _short(case), seed=2))
    full = n(cond, x_t, nl)
    parts = [n(cond[s].contiguous(), x_t[s].contiguous(), nl[s].contiguous()) for s in (slice(0, 2), slice(2, 5))]
    assert torch.isfinite(full).all() and float(full.abs().max()) > 0
    assert torch.equal(full, torch.cat(parts))


def check_rejects_bad_geometry(case):
    n, m = net(case), model(case)
    for N in case.bad_lengths:
        z = torch.zeros(1, 1, N, device="cuda")
        with pytest.raises(AssertionError):
            n(z, z, torch.ones(1, device="cuda"))
        with pytest.raises(AssertionError):
            m.infer(z, seed=1)
    if case.rejects_empty_batch:
        z = torch.zeros(0, 1, case.golden_len, device="cuda")              # B = 0
        with pytest.raises((AssertionError, ValueError, RuntimeError)):
            n(z, z, torch.ones(0, device="cuda"))


def check_spectrogram_arch_is_not_implemented(case):
    import model.diffusion as D
    import model.model as M
    d = D.GaussianDiffusion(*SCHED, device="cuda")
    m = M.SDDM_spectrogram(d, net(case, case.golden_len), hop_samples=case.spec_hop).cuda()
    with pytest.raises(NotImplementedError):
        m.infer(torch.zeros(*case.spec_input, device="cuda"), seed=1)


def check_refused_at_configure(case, cfg, name):
    import sddm_hip
    with pytest.raises(NotImplementedError, match=name if case.refusal_match else None):
        sddm_hip.Context(cfg, 0)


def check_missing_params(case):
    import sddm_hip
    ctx = sddm_hip.Context(config(case, case.golden_len if case.dual_transformer else None), 0)
    assert ctx.missing() == case.state_dict_count
    if case.loads_state_dict:
        ctx.load_state_dict({"noise_estimate_model." + k: v for k, v in params(case).items()})
        assert ctx.missing() == 0
    ctx.close()


def check_sddm_forward_matches_oracle(case):
    """SDDM.forward (evaluation only): q-sample at fixed t, then the network."""
    B, N = 2, _short(case)
    rng = np.random.default_rng(23)
    target = torch.from_numpy(rng.uniform(-0.5, 0.5, (B, 1, N)).astype(np.float32)).cuda()
    cond = (target + torch.from_numpy(rng.uniform(-0.1, 0.1, (B, 1, N)).astype(np.float32)).cuda())
    noise = torch.from_numpy(rng.standard_normal((B, 1, N)).astype(np.float32)).cuda()
    t = torch.tensor([3, 1])
    r = torch.tensor([0.25, 0.75])
    m = model(case, N)
    with torch.no_grad():
        predicted, got_noise = m(target, cond, noise=noise, t=t, random_step=r)
    assert torch.equal(got_noise, noise) and tuple(predicted.shape) == (B, 1, N)
    x_t, level, _ = m.diffusion.q_stochastic(target, noise, t=t, random_step=r)   # (x_t, noise level, step)
    ref = oracle_forward(case, cond.cpu().numpy(), x_t.cpu().numpy(), level.cpu().numpy())
    err = rms(predicted.cpu().numpy(), ref)
    print(f"{case.name} SDDM.forward: rms vs oracle {err:.3e}")
    assert err <= 1e-4 * gate(ref)


def check_infer_cli_end_to_end(case, tmp_path):
    """infer.py with the network's config at chunks of cli_chunk samples and T = 3: WAV in, chunk,
    denoise, stitch, WAV out."""
    import infer
    import model.diffusion as D
    import model.model as M
    from data_loader import wav_io
    from parse_config import ConfigParser, read_json
    N = case.cli_chunk
    rng = np.random.default_rng(4)
    for d in ("clean", "noisy"):
        os.makedirs(tmp_path / "data" / d)
    lengths = list(case.cli_lengths)
    for i, n in enumerate(lengths):
        c = 0.3 * np.sin(np.arange(n) * 0.05)
        write_pcm16(tmp_path / "data" / "clean" / f"u{i}.wav", c)
        write_pcm16(tmp_path / "data" / "noisy" / f"u{i}.wav", c + rng.uniform(-0.05, 0.05, n))
    cfg = read_json(os.path.join(os.path.dirname(infer.__file__), "configs", case.cli_config))
    assert cfg["network"]["type"] == case.name
    op, value = case.cli_num_samples
    assert cfg["num_samples"] % value == 0 if op == "%" else cfg["num_samples"] == value
    cfg["num_samples"] = N
    cfg["diffusion"]["args"].update({"n_timestep": 3, "linear_end": 0.05})
    cfg["infer_dataset"]["args"]["data_root"] = str(tmp_path / "data")
    cfg["infer_data_loader"]["args"].update({"batch_size": 1, "num_workers": 0})
    cfg["trainer"]["save_dir"] = str(tmp_path / "runs")
    ref_model = M.SDDM(D.GaussianDiffusion("linear", 3, 1e-4, 0.05, device="cpu"), net(case, N))
    ck = tmp_path / "model_best.pth"
    torch.save({"arch": "SDDM", "epoch": 1,
                "state_dict": {"module." + k: v.cpu() for k, v in ref_model.state_dict().items()},
                "config": json.loads(json.dumps(cfg))}, ck)
    config = ConfigParser(cfg, resume=ck, run_id="e2e")
    log = infer.main(config, seed=100)
    assert np.isfinite(log["loss"])
    for i, n in enumerate(lengths):
        out, sr = wav_io.load(os.path.join(str(config.save_dir), "samples", "output", f"u{i}.wav"))
        assert sr == 16000 and out.shape[1] % N == 0
        assert out.shape == (1, -(-n // N) * N) if case.cli_exact_shape else out.shape[1] >= n
        assert torch.isfinite(out).all() and float(out.abs().max()) > 0
