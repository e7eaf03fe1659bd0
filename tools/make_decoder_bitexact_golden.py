#!/usr/bin/env python
"""Records what tests/test_gpu_decoder_bitexact.py compares against: run it on the build whose results are to be kept (TACO_LIB names a
library other than the tree's), on a whole MI355X.  Writes decoder_bitexact.json (sha256 of the complete arrays) and one
decoder_bitexact_<case>.npz (a fixed sample of steps) per case into the directory given (default tests/golden).
    python tools/make_decoder_bitexact_golden.py [DIR]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import test_gpu_decoder_bitexact as T


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    os.makedirs(out, exist_ok=True)
    doc = {}
    for name in sorted(T.CASES):
        mel, al, stop = T.run_case(name)
        steps, mel_s, al_s = T.sample(name, mel, al)
        np.savez(os.path.join(out, "decoder_bitexact_%s.npz" % name), steps=steps, mel=mel_s, alignments=al_s)
        doc[name] = {"mel_shape": list(mel.shape), "alignments_shape": list(al.shape), "stop_step": stop,
                     "mel_sha256": T.digest(mel), "alignments_sha256": T.digest(al)}
        print(name, doc[name], flush=True)
    json.dump(doc, open(os.path.join(out, "decoder_bitexact.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
