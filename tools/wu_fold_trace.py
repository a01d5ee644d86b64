"""Kernel time of Waveunet's short levels by row length, from a rocprofv3 --kernel-trace CSV of
tools/bench_waveunet.py: wu_fold_trace.py <kernel_trace.csv> [--samples 16384] [--per-row]

The launch sequence of a reverse step is fixed (csrc/wu1_runtime.h), so the n-th launch of a step
is a known layer with a known output length.  The script walks the trace in start order, cuts it
into steps at the stem kernel, checks each step against the sequence of the path (--per-row: the
trace was taken on the per-row path, the default or SDDM_WU_NO_FOLD=1; else with SDDM_WU_FOLD_ALL=1)
and sums, per output length below 128, the time of the
convs and of the finalize launches that belong to them.  One JSON line: microseconds per step.
"""
import argparse
import csv
import json


def sequence(N, per_row, levels=12):
    """(kind, output length) of every launch of a step; kind: stem, conv, film, fin, head, trans."""
    L = [N >> i for i in range(levels)]
    seq = []

    def layer(n, film):
        folded = not per_row and n < 128
        seq.append(("conv", n))
        if not folded:
            seq.append(("fin", n))
        if film:
            seq.extend([("film", n), ("film", n)])
    seq += [("stem", L[0]), ("fin", L[0]), ("film", L[0]), ("film", L[0])]
    for i in range(levels - 1):
        if i > 0:
            layer(L[i], True)
        layer(L[i], False)
        layer(L[i + 1], False)
    layer(L[-1], False)
    for i in range(levels - 1, 0, -1):
        for _ in range(3):
            layer(L[i - 1], False)
    seq += [("head", L[0]), ("trans", L[0])]
    return seq


def kind_of(name):
    if "wu_stem_kernel" in name:
        return "stem"
    if "wu_gn_finalize" in name:
        return "fin"
    if "wu_fold_kernel" in name or "wu_conv_kernel" in name:
        return "conv"
    if "wu2_head_kernel" in name:
        return "head"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--samples", type=int, default=16384)
    ap.add_argument("--per-row", action="store_true")
    args = ap.parse_args()
    with open(args.csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    seq = sequence(args.samples, args.per_row)
    stems = [i for i, r in enumerate(rows) if kind_of(r["Kernel_Name"]) == "stem"]
    total, steps, per_len = 0.0, 0, {}
    for s in stems:
        step = rows[s:s + len(seq) - 1]                     # the transition is not matched by name
        if len(step) < len(seq) - 1:
            continue
        ok = all(kind_of(r["Kernel_Name"]) == (k if k != "film" else "conv") for r, (k, _) in zip(step, seq))
        if not ok:
            continue
        steps += 1
        for r, (k, n) in zip(step, seq):
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            total += us
            if n < 128:
                d = per_len.setdefault(n, {"conv_us": 0.0, "film_us": 0.0, "fin_us": 0.0, "launches": 0})
                d[{"conv": "conv_us", "film": "film_us", "fin": "fin_us"}[k]] += us
                d["launches"] += 1
    assert steps, "no step of the trace matches the launch sequence"
    out = {"path": "per_row" if args.per_row else "fold_all", "steps": steps, "launches_per_step": len(seq),
           "kernel_us_per_step": round(total / steps, 2),
           "by_length": {str(n): {k: round(v / steps, 2) for k, v in d.items()} for n, d in sorted(per_len.items(), reverse=True)}}
    for d in out["by_length"].values():
        d["sum_us"] = round(d["conv_us"] + d["film_us"] + d["fin_us"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
