#!/usr/bin/env python
"""Times matching recognised text to script lines (taco_amd.alignment) at the shape of the reference's datasets/moon: 4 877 utterances,
each scored against the ~230 lines of its script, about 1.13 million (line, utterance) pairs.  Nothing outside the repository is read:
the committed fixture (tests/golden/align_moon: the lines and the recognised utterances of two of moon's scripts) is tiled from a seed --
every script holds the fixture's lines, filled up with lines spliced from two of them, and utterances drawn from the fixture's.

Timed, on the GPU:
  * the two launches of taco_text_matches alone (device events around windows of calls, after a warm-up), next to the four-column kernel
    forced on the same pairs (taco_debug_text_matches_cols), alternating;
  * the whole align_text_batch: cleaning and packing the texts, upload, both kernels, download, the string logic on the host;
and on the host, one thread: difflib on a random sample of the same pairs, extrapolated to all of them -- the yardstick.

    python tools/bench_align.py [--utterances 4877] [--scripts 21] [--sample 20000] [--windows 5] [--calls 100] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

FIXTURE = os.path.join(ROOT, "tests", "golden", "align_moon")


def fixture_texts():
    """(the fixture's distinct non-empty script lines, its recognised utterances)"""
    from taco_amd.alignment import clean_candidates
    lines = []
    for name in sorted(os.listdir(os.path.join(FIXTURE, "assets"))):
        with open(os.path.join(FIXTURE, "assets", name), encoding="utf-8") as f:
            lines += [c for c in clean_candidates(f.readlines()) if c]
    with open(os.path.join(FIXTURE, "recognition.json"), encoding="utf-8") as f:
        rec = json.load(f)
    return list(dict.fromkeys(lines)), list(rec.values())


def make_corpus(n_utterances, n_scripts, seed=0):
    """-> (recognition {audio path: text}, scripts {name: lines}).  A script is the fixture's lines in a random order, filled up to the number
    of its utterances with lines spliced from the halves of two of them; its utterances are drawn from the fixture's."""
    rs = random.Random(seed)
    lines, utts = fixture_texts()
    per = -(-n_utterances // n_scripts)
    recognition, scripts = {}, {}
    for s in range(n_scripts):
        name = "%03d" % (s + 1)
        mine = list(lines)
        rs.shuffle(mine)
        while len(set(mine)) < per:
            x, y = rs.choice(lines), rs.choice(lines)
            mine.append(x[:len(x) // 2] + y[len(y) // 2:])
        scripts[name] = [ln + "\n" for ln in dict.fromkeys(mine)]
        for u in range(min(per, n_utterances - len(recognition))):
            recognition["./datasets/bench/audio/%s.%04d.wav" % (name, u)] = rs.choice(utts)
    return recognition, scripts


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--utterances", type=int, default=4877)
    ap.add_argument("--scripts", type=int, default=21)
    ap.add_argument("--sample", type=int, default=20000, help="pairs difflib scores on the host")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ctypes as C
    import torch
    from taco_amd import _lib, alignment as A
    if not torch.cuda.is_available():
        sys.exit("bench_align.py needs a GPU: nothing here is timed on the host in its place")
    lib = _lib.load_library()
    recognition, scripts = make_corpus(a.utterances, a.scripts)

    # the pool and the pairs exactly as align_text_batch forms them
    texts, pairs = [], []
    by_script = {}
    for path, text in recognition.items():
        by_script.setdefault(A.script_of(path)[1], []).append(text)
    for name, utts in by_script.items():
        cands = A.clean_candidates(scripts[name])
        c0 = len(texts)
        texts += [A.plain_text(c) for c in cands]
        for t in utts:
            texts.append(A.plain_text(t))
            pairs.append(np.stack([np.arange(c0, c0 + len(cands)), np.full(len(cands), len(texts) - 1)], 1))
    pairs = np.concatenate(pairs).astype(np.int32)
    n_pairs = len(pairs)
    max_b = max(len(texts[b]) for b in set(pairs[:, 1].tolist()))
    chars, offsets = A.pack_texts(texts)
    d_chars, d_off, d_pairs = (torch.as_tensor(x).cuda() for x in (chars, offsets, pairs))
    d_m = torch.empty(n_pairs, dtype=torch.int32, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def launch(cols):
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.taco_debug_text_matches_cols(st, ptr(d_chars), len(chars), ptr(d_off), len(texts), ptr(d_pairs), n_pairs, ptr(d_m), cols))

    results = {}
    for cols in (0, 4):
        for _ in range(3):
            launch(cols)
        torch.cuda.synchronize()
        results[cols] = d_m.cpu().numpy().copy()
    assert np.array_equal(results[0], results[4]) and (results[0] >= 0).all()
    ms = {0: [], 4: []}
    for _ in range(a.windows):
        for cols in (0, 4):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                launch(cols)
            e1.record()
            e1.synchronize()
            ms[cols].append(e0.elapsed_time(e1) / a.calls)

    A.align_text_batch(recognition, scripts)                 # warm-up of the whole path
    torch.cuda.synchronize()
    whole = []
    for _ in range(3):
        t0 = time.perf_counter()
        out = A.align_text_batch(recognition, scripts)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    aligned = sum(isinstance(v, str) for v in out.values())

    rs = random.Random(1)
    sample = rs.sample(range(n_pairs), min(a.sample, n_pairs))
    t0 = time.perf_counter()
    host = [A.host_match_count(texts[pairs[p, 0]], texts[pairs[p, 1]]) for p in sample]
    host_s = time.perf_counter() - t0
    assert np.array_equal(np.array(host), results[0][sample]), "the device and difflib disagree on the sample"
    host_ms = host_s / len(sample) * n_pairs * 1e3

    med = lambda v: float(np.median(v))
    line = {"metric": "k_text_matches on every (script line, utterance) pair of a corpus shaped like datasets/moon, against difflib on the host for the same pairs",
            "pairs": n_pairs, "utterances": len(recognition), "scripts": len(scripts), "texts": len(texts), "characters": int(len(chars)),
            "longest_utterance": int(max_b),
            "kernel_ms": med(ms[0]), "kernel_ms_windows": ms[0], "kernel_pairs_per_s": n_pairs / (med(ms[0]) * 1e-3),
            "four_column_kernel_ms": med(ms[4]), "four_column_kernel_ms_windows": ms[4],
            "align_text_batch_ms": med(whole), "align_text_batch_ms_runs": whole, "align_text_batch_pairs_per_s": n_pairs / (med(whole) * 1e-3),
            "aligned_as_str": aligned,
            "difflib_host_ms_extrapolated": host_ms, "difflib_us_per_pair": host_s / len(sample) * 1e6, "difflib_sample_pairs": len(sample),
            "difflib_pairs_per_s": len(sample) / host_s,
            "windows": "%d windows of %d calls per kernel, the two alternating, after 3 warm-up calls each; align_text_batch: 3 runs after a warm-up, host clock to a synchronise"
                       % (a.windows, a.calls),
            "checked": "device M equals difflib on the %d sampled pairs; both kernels agree on all pairs" % len(sample)}
    text = json.dumps(line, ensure_ascii=False)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
