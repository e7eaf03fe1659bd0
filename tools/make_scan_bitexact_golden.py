#!/usr/bin/env python
"""Records what tests/test_gpu_scan_bitexact.py compares against: run it on the build whose results are to be kept (TACO_LIB names a
library other than the tree's), on a whole MI355X.  Writes scan_bitexact.json (sha256 of the complete arrays, the losses of the training
step as bit patterns) and scan_bitexact.npz (first and last frames of two rows of every scan array) into the directory given
(default tests/golden).
    python tools/make_scan_bitexact_golden.py [DIR]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np
import test_gpu_scan_bitexact as S


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else S.GOLDEN
    os.makedirs(out, exist_ok=True)
    doc, arrays = {}, {}

    def keep(name, a):
        doc[name + "_shape"] = list(a.shape)
        doc[name + "_sha256"] = S.digest(a)
        arrays[name] = S.sample(a)
        print(name, doc[name + "_shape"], doc[name + "_sha256"], flush=True)

    for name in sorted(S.CASES):
        keep(name + "/out", S.run_infer(name))
        o, g = S.run_tape(name)
        keep(name + "/tape_out", o)
        keep(name + "/tape_gates", g)
    (l1, g1), (l2, g2) = S.run_train()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), "the build is not reproducible"
    doc["train/losses"] = [float(v) for v in l1]
    doc["train/losses_bits"] = [int(v) for v in l1.view(np.uint32)]
    doc["train/grads_shape"] = list(g1.shape)
    doc["train/grads_sha256"] = S.digest(g1)
    print("train", doc["train/losses"], doc["train/grads_sha256"], flush=True)
    np.savez(os.path.join(out, "scan_bitexact.npz"), **arrays)
    json.dump(doc, open(os.path.join(out, "scan_bitexact.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
