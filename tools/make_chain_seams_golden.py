#!/usr/bin/env python
"""Records what tests/test_gpu_chain_seams.py compares against: run it on the build whose results are to be kept (TACO_LIB names a library
other than the tree's), on a whole MI355X.  Every case runs twice, and nothing is written when the two runs of that build differ.
Writes chain_seams.json (sha256 of the complete arrays) and chain_seams.npz (first and last frames of two rows of every array) into the
directory given (default tests/golden).
    python tools/make_chain_seams_golden.py [DIR]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import test_gpu_chain_seams as S


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN
    os.makedirs(out, exist_ok=True)
    doc, arrays = {}, {}
    for name in sorted(S.CASES):
        first, second = S.run_case(name), S.run_case(name)
        for array, a, b in zip(S.ARRAYS, first, second):
            k = S.key(name, array)
            if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
                raise SystemExit("nothing written: two runs of this build differ in " + k)
            doc[k + "_shape"] = list(a.shape)
            doc[k + "_sha256"] = S.digest(a)
            arrays[k] = S.sample(a)
            print(k, doc[k + "_shape"], doc[k + "_sha256"], flush=True)
    np.savez(os.path.join(out, "chain_seams.npz"), **arrays)
    with open(os.path.join(out, "chain_seams.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
