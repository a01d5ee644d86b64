"""Kernel time and boundary gaps of the UNet reverse steps in a rocprofv3 --kernel-trace CSV.

    python tools/trace_gaps.py PROFILE_DIR/run_kernel_trace.csv [--label before]

A reverse step is the run of sddm kernels from conv_in to final_kernel.  Per step: the sum of kernel
durations, the wall time from conv_in's start to final_kernel's end, and their difference (the
boundary gaps).  Per producer family (conv_in, strip, tile, deep): the mean kernel duration and the
mean gap between that kernel's end and the next kernel's start.
"""
import argparse
import csv
import re
import statistics as st


def family(name):
    for key, fam in (("conv_in_kernel", "conv_in"), ("conv_strip_kernel", "strip"), ("conv_tile_kernel", "tile"),
                     ("conv_deep_kernel", "deep"), ("conv_chain_kernel", "chain"), ("final_kernel", "final")):
        if key in name:
            return fam
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    rows = []
    with open(a.trace) as f:
        for r in csv.DictReader(f):
            fam = family(r["Kernel_Name"])
            if fam:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), fam, r["Kernel_Name"]))
    rows.sort()
    steps, cur = [], None
    for r in rows:
        if r[2] == "conv_in":
            cur = [r]
        elif cur is not None:
            cur.append(r)
            if r[2] == "final":
                steps.append(cur)
                cur = None
    n = len(steps[0])
    steps = [s for s in steps if len(s) == n]
    steps = steps[len(steps) // 10:]                      # leave the first tenth out (warm-up)
    ksum = [sum(e - b for b, e, _, _ in s) * 1e-3 for s in steps]
    wall = [(s[-1][1] - s[0][0]) * 1e-3 for s in steps]
    gap = [w - k for w, k in zip(wall, ksum)]
    print(f"[{a.label}] {len(steps)} reverse steps of {n} launches: kernels {st.median(ksum):.1f} us, "
          f"conv_in start -> final end {st.median(wall):.1f} us, gaps {st.median(gap):.1f} us "
          f"({st.median(gap) / (n - 1):.2f} us per boundary)  (medians)")
    per = {}
    for s in steps:
        for i in range(n - 1):
            d = per.setdefault(s[i][2], [[], [], 0])
            d[0].append((s[i][1] - s[i][0]) * 1e-3)
            d[1].append((s[i + 1][0] - s[i][1]) * 1e-3)
    for fam, (dur, g, _) in per.items():
        k = len(dur) // len(steps)
        print(f"  {fam:8s} {k:2d} launches/step: duration {st.mean(dur):6.2f} us, gap to the next kernel {st.mean(g):5.2f} us "
              f"(per step {st.mean(dur) * k:6.1f} + {st.mean(g) * k:5.1f} us)")
    # per launch position (the same layer in every step)
    print("  pos family   duration   gap-after   kernel")
    for i in range(n - 1):
        dur = st.mean((s[i][1] - s[i][0]) * 1e-3 for s in steps)
        g = st.mean((s[i + 1][0] - s[i][1]) * 1e-3 for s in steps)
        short = re.sub(r"^_ZN4sddm\d+|NS_\d+ConvArgsE.*$", "", steps[0][i][3])[:60]
        print(f"  {i:3d} {steps[0][i][2]:8s} {dur:8.2f} {g:8.2f}   {short}")


if __name__ == "__main__":
    main()
