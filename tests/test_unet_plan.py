"""CPU: the UNet planner (csrc/unet_plan.h) through its device-free entry point sddm_hip.unet_plan.

Which kernel and tiling every conv of a UNetModified2 / UNetTST step gets is a function of the
config, the dtype, the lane capacity and the tuning table; here it is pinned without a GPU: the
measured tables of configs/conv_tuning.json land on every layer they name (the CPU twin of the GPU
tests that parse profile_ops), and tests/golden/unet_plans.json holds the whole plan of CASES.
test_gpu_unet.py::test_plan_call_agrees_with_the_run ties the call to what a context runs."""
import copy
import json
import os

import pytest

import sddm_hip
from _helpers import GOLDEN, unet_config

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TUNING = os.path.join(REPO, "speech-denoising-diffusion-model-2_amd", "configs", "conv_tuning.json")
PLANS = os.path.join(GOLDEN, "unet_plans.json")


def config(N, lane_rows=None, type="UNetModified2", **args):
    cfg = unet_config(N)
    cfg["network"]["type"] = type
    cfg["network"]["args"].update(args)
    if lane_rows:
        cfg["lane_rows"] = lane_rows
    return cfg


# the bottom level (downs.10, mid.0, ups.0) as one launch (conv_chain.hip), on the headline geometry
CHAIN = {"lane_batch": 16, "dtype": "bfloat16", "num_samples": 16448,
         "kernel": {k: "chain" for k in ("downs.10", "mid.0.block1", "mid.0.block2", "ups.0.block1", "ups.0.block2")}}

# name -> (config, tuning: "repo" (the repository's file), a table or None, dtype, rows of the forward
# in the GPU op-list comparison).  headline: the bench geometry (N=16448, lanes of 16); small: the
# suite's geometry; frames96: 96 frames, whose 6 x 8 and 3 x 4 levels no full conv_deep tile divides
# (choose_deep's second pass); res_blocks2: GroupNorm groups straddle cat(x, skip), so concat steps appear
CASES = {
    "headline_bf16": (config(16448), "repo", "bfloat16", 16),
    "headline_f16": (config(16448), "repo", "float16", 16),
    "headline_f32": (config(16448), "repo", "float32", 16),
    "small_bf16": (config(2112), None, "bfloat16", 4),
    "small_f32": (config(2112), None, "float32", 4),
    "unettst_bf16": (config(16448, type="UNetTST", n_TSTB=6), "repo", "bfloat16", 4),
    "res_blocks2_bf16": (config(2112, res_blocks=2), None, "bfloat16", 4),
    "frames96_f32": (config(128 + 95 * 64), None, "float32", 4),
}


def tuning_text(tuned):
    return open(TUNING).read() if tuned == "repo" else json.dumps(tuned) if tuned else None


def plan_of(case):
    cfg, tuned, dtype, _ = CASES[case]
    return sddm_hip.unet_plan(copy.deepcopy(cfg), tuning_text(tuned), dtype)


def kernels(plan):
    return {s["name"]: sddm_hip.planned_kernel(s) for s in plan if s["type"] == "conv"}


def tables():
    return json.load(open(TUNING))["tables"]


@pytest.mark.parametrize("N,lane,dtype", [(16448, 16, "bfloat16"), (16448, 8, "bfloat16"), (16448, 4, "bfloat16"),
                                          (32832, 64, "float16")])
def test_measured_table_lands_on_every_layer(N, lane, dtype):
    tab, = [t for t in tables() if t["num_samples"] == N and t["lane_batch"] == lane]
    assert tab["dtype"] == dtype
    got = kernels(sddm_hip.unet_plan(config(N, lane), open(TUNING).read(), dtype))
    assert len(tab["kernel"]) == 42
    for layer, k in tab["kernel"].items():
        assert got.get(layer) == k, f"{layer}: table names {k}, plan has {got.get(layer)}"


def test_bf16_table_serves_f16_and_not_the_reverse():
    text = open(TUNING).read()
    bf16, = [t for t in tables() if (t["num_samples"], t["lane_batch"]) == (16448, 16)]
    assert bf16["dtype"] == "bfloat16"
    assert kernels(sddm_hip.unet_plan(config(16448, 16), text, "float16")) == bf16["kernel"]
    f16, = [t for t in tables() if (t["num_samples"], t["lane_batch"]) == (32832, 64)]
    assert f16["dtype"] == "float16"
    assert kernels(sddm_hip.unet_plan(config(32832, 64), text, "float16")) == f16["kernel"]
    # a bf16 plan of the f16 table's geometry: the heuristic's plan, as with no table at all
    assert sddm_hip.unet_plan(config(32832, 64), text, "bfloat16") == sddm_hip.unet_plan(config(32832, 64), None, "bfloat16")
    assert kernels(sddm_hip.unet_plan(config(32832, 64), text, "bfloat16")) != f16["kernel"]


@pytest.mark.parametrize("case", ["headline_f32", "small_f32"])
def test_fp32_takes_no_tile_kernel(case):
    convs = [s for s in plan_of(case) if s["type"] == "conv"]
    assert len(convs) == 42
    assert all(s["kernel"] in ("strip", "deep") and s["tile"] == -1 for s in convs)


def test_step_lists():
    """Launch order and step kinds: conv_in, the convs, final; one concat per straddling block at
    res_blocks 2; the Dual_Transformer in place of mid.0; chain marks on the bottom level (bf16)."""
    p = plan_of("headline_bf16")
    assert [p[0]["type"], p[-1]["type"]] == ["conv_in", "final"] and len(p) == 44
    c = sddm_hip.unet_plan(config(16448), json.dumps(CHAIN), "bfloat16")
    assert [s["name"] for s in c if s.get("kernel") == "chain"] == list(CHAIN["kernel"])
    unmarked = lambda plan: [s for s in plan if s["name"] not in CHAIN["kernel"]]   # noqa: E731
    assert unmarked(c) == unmarked(sddm_hip.unet_plan(config(16448), None, "bfloat16"))
    assert "chain" not in kernels(sddm_hip.unet_plan(config(16448), json.dumps(dict(CHAIN, dtype="float32")), "float32")).values()
    t = plan_of("unettst_bf16")
    assert [s["name"] for s in t if s["type"] == "dual_transformer"] == ["mid"] and len(t) == 43
    assert "chain" not in kernels(t).values()
    assert [s["type"] for s in plan_of("res_blocks2_bf16")].count("concat") > 0
    # 96 frames: no full conv_deep tile divides the 6 x 8 level, so fp32 runs partly filled ones (3 x 8
    # of 32 pixels, choose_deep's second pass); the 16-bit plan takes a tile kernel over the whole image
    f = {s["name"]: s for s in plan_of("frames96_f32") if s["type"] == "conv"}["downs.8"]
    assert (f["Ho"], f["Wo"], f["kernel"], f["TR"], f["TW"], f["mt"]) == (6, 8, "deep", 3, 8, 32)
    h = {s["name"]: s for s in sddm_hip.unet_plan(config(128 + 95 * 64), None, "bfloat16") if s["type"] == "conv"}["downs.8"]
    assert (h["kernel"], h["TR"], h["TW"]) == ("tile", 6, 8)


def pack(plans):
    """{case: plan} in the pin file's form.  Many steps recur between the cases and every step of a
    kind has the same keys, so the file holds each key tuple and each distinct step once: "keys"
    [[key, ...]], "steps" [[index into keys, value, ...]] ("out" as its five values) and per case
    the indices of its steps in launch order."""
    keys, steps, cases = [], [], {}
    for case, plan in plans.items():
        cases[case] = []
        for s in plan:
            ks = list(s)
            if ks not in keys:
                keys.append(ks)
            row = [keys.index(ks)] + [list(v.values()) if k == "out" else v for k, v in s.items()]
            if row not in steps:
                steps.append(row)
            cases[case].append(steps.index(row))
    return {"keys": keys, "steps": steps, "cases": cases}


OUT_KEYS = ("C", "H", "W", "tiles", "n_tile")


def unpack(pins, case):
    rows = [pins["steps"][i] for i in pins["cases"][case]]
    return [{k: dict(zip(OUT_KEYS, v)) if k == "out" else v for k, v in zip(pins["keys"][r[0]], r[1:])} for r in rows]


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_is_the_pinned_one(case):
    """The whole plan, every field of every step.  The pins were recorded after the op lists of a
    forward of every case had been compared, string for string, with those of the runtime before
    the planner was split out (profiles/unet_plan_ops_new.txt; the earlier runtime's list was the
    same file, byte for byte)."""
    assert plan_of(case) == unpack(json.load(open(PLANS)), case)


def test_refusals_keep_their_messages():
    with pytest.raises(NotImplementedError, match=r"conv_in needs inner_channel 32 and segment_len dividing 512 \(got 64, 128\)"):
        sddm_hip.unet_plan(config(2112, inner_channel=64))
    # 48 frames halve to an odd size above the bottom level
    with pytest.raises(AssertionError, match=r"n_frames 48 and segment_len 128 must be multiples of 32"):
        sddm_hip.unet_plan(config(128 + 47 * 64))
    with pytest.raises(NotImplementedError, match=r"the bottom level has 32 x 4 = 128 tokens, the Dual_Transformer kernel holds 64"):
        sddm_hip.unet_plan(config(128 + 1023 * 64, type="UNetTST"))
    with pytest.raises(NotImplementedError, match="network type 'DiffWave'"):
        sddm_hip.unet_plan(config(2112, type="DiffWave"))
