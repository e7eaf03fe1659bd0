#!/usr/bin/env python
"""Records what tests/test_pack_host.py compares against: arena length and the three digests of taco_debug_pack_host for every case of
the test.  Run it on the build whose packs are to be kept (TACO_LIB names a library other than the tree's) -- the packing code as it
stood before a change to it, with tools/pack_hook_only.patch applied when that build has no hook yet.  No GPU is needed.
    python tools/make_pack_digests.py [FILE]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import test_pack_host as P


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else P.GOLDEN
    doc = {}
    for name in sorted(P.CASES):
        rc, got, dt = P.pack(name)
        assert rc == 0, (name, rc)
        assert got["mask"] == P.CASES[name][3], "%s: mask %#x, expected %#x" % (name, got["mask"], P.CASES[name][3])
        doc[name] = {k: got[k] for k in ("arena_floats", "arena", "vars", "bf3")}
        print("%s: %.2f s  %s" % (name, dt, doc[name]), flush=True)
    json.dump(doc, open(out, "w"), indent=1)
    open(out, "a").write("\n")


if __name__ == "__main__":
    main()
