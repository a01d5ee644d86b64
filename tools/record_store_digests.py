"""Record the digest fixture of a test module (its FIXTURE): SHA-256 of the outputs of every one of
its CASES, computed on the GPU with the library that SDDM_LIB names (build the commit to pin as a
variant: SDDM_BUILD_VARIANT=parent python .../sddm_hip/build.py).

    SDDM_LIB=tools/_parent/libsddm_hip.so python tools/record_store_digests.py [--module NAME] [--out FILE] [--check]

--module: test_gpu_store_flavour (tests/golden/unet_store_digests.json, the default) or
test_gpu_seq_digests (tests/golden/seq_path_digests.json).
--check compares against the committed fixture instead of writing (any library).
"""
import argparse
import importlib
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "speech-denoising-diffusion-model-2_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--module", default="test_gpu_store_flavour")
    ap.add_argument("--out", default=None)
    ap.add_argument("--check", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch
    import sddm_hip
    sf = importlib.import_module(a.module)
    pinned = json.load(open(sf.FIXTURE))["digests"] if a.check else {}
    digests, bad = {}, []
    for case in sf.CASES:
        t0 = time.time()
        try:
            out = sf.run_case(torch, case)
        except (AssertionError, ValueError, NotImplementedError, sddm_hip.SddmError) as e:
            if isinstance(e, sddm_hip.SddmError) and "invalid argument" not in str(e):
                raise                                             # a device error: stop here
            print(f"{case}: REFUSED {e}", flush=True)             # the plan or a launcher refused the table
            bad.append(case)
            continue
        assert np.isfinite(out).all() and np.abs(out).max() > 0, case
        digests[case] = sf.digest(out)
        note = ""
        if a.check and digests[case] != pinned.get(case):
            bad.append(case)
            note = "  MISMATCH"
        print(f"{case}: {digests[case][:16]}  {time.time() - t0:.1f} s{note}", flush=True)
    if a.check:
        print("DIGESTS_DIFFER " + " ".join(bad) if bad else "DIGESTS_EQUAL")
        return 1 if bad else 0
    doc = {"recorded_with": os.path.relpath(sddm_hip.LIB_PATH, REPO), "hash": "sha256 of the fp32 output bytes",
           "digests": digests}
    with open(a.out or sf.FIXTURE, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("RECORDED", len(digests), "REFUSED", " ".join(bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
