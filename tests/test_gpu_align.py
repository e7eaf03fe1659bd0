"""Matching recognised text to script lines on the device (k_text_matches / k_text_best_two, taco_amd.alignment; recognition/alignment.py).
Everything is integer and is compared for EQUALITY with difflib (the Python standard library is the reference's arithmetic), the top-two
decision with Python's sorted on the host ratios and with exact fractions; the end-to-end results with what the reference's own align_text_fn
produced (tests/golden/alignment_vectors.json).  Inputs are small: every test takes a few seconds at the most."""
import importlib.util
import json
import os
import random
import shutil

import numpy as np
import pytest

import align_reference as R
from util import dev, ptr, stream

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
LANE_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 199)
CANARY = -77


def lib():
    from taco_amd import _lib
    return _lib.load_library()


def rand_text(rs, n, alphabet):
    return "".join(rs.choice(alphabet) for _ in range(n))


def run_matches(chars, offsets, pairs, n_chars=None, n_texts=None, n_pairs=None, cols=None):
    """taco_text_matches on explicit arrays -> (rc, matches [n_pairs], the canary words behind them).  chars may be longer than n_chars."""
    import torch
    chars, offsets = np.asarray(chars, np.int32), np.asarray(offsets, np.int32)
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    n_chars = len(chars) if n_chars is None else n_chars
    n_texts = len(offsets) - 1 if n_texts is None else n_texts
    n_pairs = len(pairs) if n_pairs is None else n_pairs
    dc, do, dp = dev(chars if len(chars) else np.zeros(1, np.int32)), dev(offsets), dev(pairs if len(pairs) else np.zeros((1, 2), np.int32))
    out = torch.full((n_pairs + 8,), CANARY, dtype=torch.int32, device="cuda")
    if cols is None:
        rc = lib().taco_text_matches(stream(), ptr(dc), n_chars, ptr(do), n_texts, ptr(dp), n_pairs, ptr(out))
    else:
        rc = lib().taco_debug_text_matches_cols(stream(), ptr(dc), n_chars, ptr(do), n_texts, ptr(dp), n_pairs, ptr(out), cols)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    return rc, out[:n_pairs], out[n_pairs:]


def device_counts(texts, pairs, cols=None):
    from taco_amd.alignment import pack_texts
    chars, offsets = pack_texts(texts)
    rc, m, canary = run_matches(chars, offsets, pairs, cols=cols)
    assert rc == 0 and (canary == CANARY).all()
    return m


def want_counts(texts, pairs):
    return np.array([R.difflib_count(texts[a], texts[b]) for a, b in pairs], np.int32)


def fixture():
    with open(os.path.join(GOLD, "align_moon", "recognition.json"), encoding="utf-8") as f:
        rec = json.load(f)
    scripts = {}
    for name in ("005", "006"):
        with open(os.path.join(GOLD, "align_moon", "assets", name + ".txt"), encoding="utf-8") as f:
            scripts[name] = f.readlines()
    with open(os.path.join(GOLD, "alignment_vectors.json"), encoding="utf-8") as f:
        vec = json.load(f)
    return rec, scripts, vec


def test_every_pair_of_the_fixture_scripts():
    """every (line, utterance) pair of the two fixture scripts, each line of the files as it stands -- blank and repeated ones too,
    which align_texts would collapse: about 56 000 pairs"""
    from taco_amd import alignment as A
    rec, scripts, _ = fixture()
    total = 0
    for name, lines in scripts.items():
        cands = [A.plain_text(c) for c in lines]
        utts = [A.plain_text(t) for p, t in rec.items() if A.script_of(p)[1] == name]
        assert max(len(u) for u in utts) <= 64
        pairs = [(i, j) for j in range(len(utts)) for i in range(len(cands))]
        want = np.array([R.difflib_count(cands[i], utts[j]) for i, j in pairs])
        got = A.match_counts(cands, utts, pairs)
        assert np.array_equal(got, want), (name, int((got != want).sum()))
        texts = cands + utts                            # the four-column kernel on the same pairs
        wide = device_counts(texts, [(i, len(cands) + j) for i, j in pairs], cols=4)
        assert np.array_equal(wide, want)
        total += len(pairs)
    assert total > 40000


@pytest.mark.parametrize("alphabet", ["ab", "abc"])
def test_tie_storm(alphabet):
    """random strings over two and three letters, where equally long blocks are everywhere: len(b) at every lane boundary of both
    kernels, len(a) from nothing to several passes of 64 rows; texts shared between pairs; every pair in both orders (the reversed ones
    with b of 300 or 1000 characters are refused by the device and scored by the host inside match_counts)."""
    from taco_amd import alignment as A
    rs = random.Random(7 + len(alphabet))
    ta = [rand_text(rs, n, alphabet) for n in (0, 1, 2, 64, 65) for _ in range(3)] + [rand_text(rs, n, alphabet) for n in (300, 1000)]
    tb = [rand_text(rs, n, alphabet) for n in LANE_EDGES for _ in range(3)]
    texts = ta + tb
    fwd = [(i, len(ta) + j) for i in range(len(ta)) for j in range(len(tb))]
    both = fwd + [(b, a) for a, b in fwd]
    got = A.match_counts(texts, texts, both)
    want = want_counts(texts, both)
    assert np.array_equal(got, want), [(len(texts[a]), len(texts[b]), g, w) for (a, b), g, w in zip(both, got, want) if g != w][:10]
    raw = device_counts(texts, both)
    refused = np.array([len(texts[b]) >= 200 for _, b in both])
    assert refused.sum() == 2 * len(tb) and np.array_equal(raw[refused], np.full(refused.sum(), -1)) and np.array_equal(raw[~refused], want[~refused])
    assert np.array_equal(device_counts(texts, fwd, cols=4), want[:len(fwd)])


def test_deep_stack():
    """99 distinct syllables, each followed by '?' in a and by '!' in b (198 characters): difflib finds 99 blocks of one character, each
    one leaving a right piece waiting; and the mirror image, the marks in front, which leaves the left pieces."""
    syl = [chr(0xAC00 + 37 * k) for k in range(99)]
    assert len(set(syl)) == 99
    a, b = "".join(s + "?" for s in syl), "".join(s + "!" for s in syl)
    ma, mb = "".join("?" + s for s in syl), "".join("!" + s for s in syl)
    texts = [a, b, ma, mb, a[::-1], b[::-1]]
    pairs = [(0, 1), (2, 3), (1, 0), (3, 2), (4, 5), (0, 3), (2, 1)]
    want = want_counts(texts, pairs)
    assert want[0] == 99 and want[1] == 99
    assert np.array_equal(device_counts(texts, pairs), want)


def test_neighbours_in_the_pool_do_not_leak_in():
    """Texts packed back to back: in front of a's range and of b's range sits the same character, behind them too, and a and b begin and
    end alike -- a run that looked one character past a range would grow.  The slack behind the last text holds that character as well."""
    rs = random.Random(11)
    texts, pairs = [], []
    for k in range(40):
        core_a, core_b = rand_text(rs, rs.choice((3, 20, 63, 70)), "ab"), rand_text(rs, rs.choice((2, 30, 64, 65, 130)), "ab")
        texts += ["q", "m" + core_a + "n", "zq", "m" + core_b + "n", "z"]
        pairs += [(5 * k + 1, 5 * k + 3), (5 * k + 3, 5 * k + 1), (5 * k + 1, 5 * k + 1), (5 * k, 5 * k + 2), (5 * k + 2, 5 * k + 4)]
    from taco_amd.alignment import pack_texts
    chars, offsets = pack_texts(texts)
    padded = np.concatenate([chars, np.full(512, ord("z"), np.int32)])
    rc, got, canary = run_matches(padded, offsets, pairs, n_chars=len(chars))
    assert rc == 0 and (canary == CANARY).all()
    assert np.array_equal(got, want_counts(texts, pairs))


def test_refusals():
    from taco_amd import alignment as A
    rs = random.Random(5)
    texts = [rand_text(rs, n, "abc") for n in (30, 199, 200, 201, 1000, 40)]
    chars, offsets = A.pack_texts(texts)
    ok = (0, 1)
    for bad in [(0, 2), (0, 3), (0, 4), (-1, 1), (0, -1), (len(texts), 1), (0, len(texts)), (2 ** 31 - 1, 0), (-2 ** 31, 0)]:
        for cols in (None, 4):
            rc, got, canary = run_matches(chars, offsets, [ok, bad, (5, 0), bad, ok], cols=cols)
            assert rc == 0 and (canary == CANARY).all()
            w = [R.difflib_count(texts[0], texts[1]), -1, R.difflib_count(texts[5], texts[0]), -1, R.difflib_count(texts[0], texts[1])]
            assert got.tolist() == w, (bad, cols)
    # long a is not refused
    rc, got, _ = run_matches(chars, offsets, [(4, 0), (3, 1)])
    assert got.tolist() == [R.difflib_count(texts[4], texts[0]), R.difflib_count(texts[3], texts[1])]
    # offsets that decrease, go negative or run outside the pool: only the pairs that use such a text
    off = np.array([0, 30, 20, 60, 100], np.int32)              # text 1 = [30, 20): decreasing; text 2 = [20, 60) is sound
    pool = np.asarray(chars[:100])
    s = lambda t: "".join(chr(c) for c in pool[off[t]:off[t + 1]])
    rc, got, canary = run_matches(pool, off, [(0, 2), (1, 2), (2, 1), (3, 0), (2, 2)])
    assert rc == 0 and (canary == CANARY).all()
    assert got.tolist() == [R.difflib_count(s(0), s(2)), -1, -1, R.difflib_count(s(3), s(0)), 40]
    for off in ([0, 30, 60, 101], [-1, 30, 60, 100], [0, 30, 60, 2 ** 31 - 1]):       # past the pool's end / before its start
        off = np.array(off, np.int32)
        bad_text = 2 if off[3] != 100 else 0
        rc, got, canary = run_matches(pool, off, [(1, bad_text), (bad_text, 1), (1, 1)], n_chars=100)
        assert rc == 0 and (canary == CANARY).all() and got.tolist() == [-1, -1, 30], off
    # the public function scores what the device refuses with difflib on the host
    pairs = [(0, 2), (0, 3), (0, 4), (1, 1), (5, 0)]
    assert np.array_equal(A.match_counts(texts, texts, pairs), want_counts(texts, pairs))


def test_grid_edges():
    import torch
    rs = random.Random(2)
    texts = [rand_text(rs, rs.randint(0, 70), "abc") for _ in range(12)]
    from taco_amd.alignment import pack_texts
    chars, offsets = pack_texts(texts)
    all_pairs = [(rs.randrange(12), rs.randrange(12)) for _ in range(9)]
    for n in (1, 3, 4, 5, 9):                                # a workgroup scores four pairs
        rc, got, canary = run_matches(chars, offsets, all_pairs[:n])
        assert rc == 0 and (canary == CANARY).all() and np.array_equal(got, want_counts(texts, all_pairs[:n])), n
    rc, got, canary = run_matches(chars, offsets, all_pairs, n_pairs=0)
    assert rc == 0 and len(got) == 0 and (canary == CANARY).all()
    out = torch.full((8, 4), CANARY, dtype=torch.int32, device="cuda")
    z = dev(np.zeros(4, np.int32))
    assert lib().taco_text_best_two(stream(), ptr(z), ptr(z), ptr(z), 1, ptr(z), 0, ptr(out)) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY).all()


def run_best_two(lengths, pair_list, matches, groups):
    """taco_text_best_two on texts of the given lengths (their characters do not matter) -> best [n_groups, 4]"""
    import torch
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    goff = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    order = [p for g in groups for p in g]
    pairs = np.array([pair_list[p] for p in order], np.int32).reshape(-1, 2)
    m = np.array([matches[p] for p in order], np.int32)
    dm, dp, do, dg = dev(m if len(m) else np.zeros(1, np.int32)), dev(pairs if len(pairs) else np.zeros((1, 2), np.int32)), dev(offsets), dev(goff)
    out = torch.full((len(groups) + 2, 4), CANARY, dtype=torch.int32, device="cuda")
    rc = lib().taco_text_best_two(stream(), ptr(dm), ptr(dp), ptr(do), len(lengths), ptr(dg), len(groups), ptr(out))
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    assert rc == 0 and (out[len(groups):] == CANARY).all()
    T = [int(lengths[a] + lengths[b]) if 0 <= a < len(lengths) and 0 <= b < len(lengths) else 0 for a, b in pairs]
    want = []
    for g0, g1 in zip(goff[:-1], goff[1:]):
        i, M, Tt, f = R.best_two(m[g0:g1], T[g0:g1])
        want.append([i + g0 if i >= 0 else -1, M, Tt, f])
        live = [k for k in range(g0, g1) if m[k] >= 0]
        if len(live) == g1 - g0 and len(live) >= 2:          # the reference's own statement: sorted on the doubles (:109-113)
            ratios = [2.0 * m[k] / T[k] if T[k] else 1.0 for k in live]
            s = sorted(ratios)[::-1]
            assert (s[0] > s[1]) == bool(f) and ratios[i] == s[0]
    return out[:len(groups)], np.array(want, np.int32).reshape(-1, 4)


def test_best_two():
    lengths = [0, 0, 10, 20, 30, 100, 201, 203, 150, 153, 7]
    P = [(2, 3), (2, 4), (3, 4), (4, 5), (0, 1), (2, 2), (6, 5), (7, 5), (8, 8), (9, 9), (10, 2), (0, 2), (1, 0)]
    #     T: 30     40      50      130     0       20      301     303     300     306     17       10      0
    M = {0: 9, 1: 12, 2: 15, 3: 20, 4: 0, 5: 10, 6: 100, 7: 101, 8: 100, 9: 102, 10: 5, 11: 0, 12: 0}
    groups = [
        [3, 0, 10],              # a strict winner: 9/30 against 20/130 and 5/17
        [0, 1, 3],               # a tie at the top: 9/30 = 12/40 -> flag 0, the first of them reported
        [1, 0, 2],               # all three equal
        [5, 3, 3],               # a tie below the top is ignored: 10/20 wins
        [10],                    # one pair
        [],                      # no pair
        [0, -1, 3],              # a refused pair: flag 0, the best of the others
        [-1, -1],                # nothing but refused pairs
        [4, 5],                  # T == 0 counts as ratio 1: it wins over 10/20 = 1 ... which is 2*10/20 = 1 too: a tie
        [4, 0],                  # T == 0 against 0.6: a strict winner
        [4, 12],                 # two empty pairs tie
        [11, 0],                 # M == 0, T > 0: ratio 0 loses
        [6, 7], [7, 6],          # 100/301 < 101/303, in both orders
        [8, 9], [9, 8],          # 100/300 = 102/306: equal fractions of different integers
        [6, 8], [8, 6],          # 100/301 < 100/300
    ]
    matches = dict(M)
    matches[-1] = -1
    pl = dict(enumerate(P))
    pl[-1] = (2, 3)
    got, want = run_best_two(lengths, pl, matches, groups)
    assert np.array_equal(got, want), np.concatenate([got, want], 1)
    flags = got[:, 3].tolist()
    assert flags == [1, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 1]
    assert got[5].tolist() == [-1, 0, 0, 0] and got[7].tolist() == [-1, 0, 0, 0] and got[6, 0] == 13     # the group's first pair (9/30 > 20/130)
    # groups longer than a wave: the winner, its first duplicate and a refused pair anywhere among 150 pairs
    rs = random.Random(4)
    lengths = [rs.randint(1, 120) for _ in range(40)]
    pl = {k: (rs.randrange(40), rs.randrange(40)) for k in range(150)}
    base = {k: rs.randint(0, min(lengths[pl[k][0]], lengths[pl[k][1]]) // 2) for k in pl}
    groups = []
    for case in range(12):
        g = list(range(150))
        rs.shuffle(g)
        groups.append(g[:rs.choice((64, 65, 129, 150))])
    matches = dict(base)
    got, want = run_best_two(lengths, pl, matches, groups)
    assert np.array_equal(got, want)
    matches[77] = -1                                         # refused somewhere in most groups
    matches[5] = min(lengths[pl[5][0]], lengths[pl[5][1]])   # and a clear winner
    got, want = run_best_two(lengths, pl, matches, groups)
    assert np.array_equal(got, want) and set(got[:, 3].tolist()) == {0, 1}
    # a text index out of range counts as refused
    got, want = run_best_two([5, 5], {0: (0, 1), 1: (0, 2), 2: (-1, 0)}, {0: 2, 1: 5, 2: 5}, [[0, 1], [2, 0], [0]])
    assert got.tolist() == [[0, 2, 10, 0], [3, 2, 10, 0], [4, 2, 10, 1]]


def test_both_calls_in_one_captured_graph():
    """Both entry points captured once and replayed twice on new inputs of the same shape: bit-equal to eager calls."""
    import torch
    from taco_amd.alignment import pack_texts
    rs = random.Random(9)
    n_c, n_u = 6, 5

    def problem():
        texts = [rand_text(rs, 40, "abc") for _ in range(n_c)] + [rand_text(rs, L, "abc") for L in (10, 64, 65, 199, 200)]
        chars, offsets = pack_texts(texts)
        return texts, chars, offsets

    pairs = np.array([(i, n_c + j) for j in range(n_u) for i in range(n_c)], np.int32)
    goff = np.arange(0, n_c * n_u + 1, n_c, dtype=np.int32)
    texts, chars, offsets = problem()
    dc, do, dp, dg = dev(chars), dev(offsets), dev(pairs), dev(goff)
    dm = torch.full((len(pairs),), CANARY, dtype=torch.int32, device="cuda")
    db = torch.full((n_u, 4), CANARY, dtype=torch.int32, device="cuda")

    def launch():
        assert lib().taco_text_matches(stream(), ptr(dc), len(chars), ptr(do), len(texts), ptr(dp), len(pairs), ptr(dm)) == 0
        assert lib().taco_text_best_two(stream(), ptr(dm), ptr(dp), ptr(do), len(texts), ptr(dg), n_u, ptr(db)) == 0

    def expect(texts):
        m, best = R.scores(texts, pairs, goff, count=R.difflib_count)
        return m, best

    launch()
    torch.cuda.synchronize()
    m0, b0 = expect(texts)
    assert np.array_equal(dm.cpu().numpy(), m0) and np.array_equal(db.cpu().numpy(), b0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            launch()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        texts, chars, offsets = problem()                    # same lengths, other characters
        dc.copy_(torch.from_numpy(chars))
        dm.fill_(CANARY)
        db.fill_(CANARY)
        g.replay()
        torch.cuda.synchronize()
        gm, gb = dm.cpu().numpy().copy(), db.cpu().numpy().copy()
        dm.fill_(CANARY)
        db.fill_(CANARY)
        launch()
        torch.cuda.synchronize()
        assert np.array_equal(gm, dm.cpu().numpy()) and np.array_equal(gb, db.cpu().numpy())
        m1, b1 = expect(texts)
        assert np.array_equal(gm, m1) and np.array_equal(gb, b1) and (gm == -1).sum() == n_c


def test_end_to_end_equals_the_reference_results(tmp_path):
    """align_text_batch on the two fixture scripts against what the reference's align_text_fn returned, entry for entry; then the tool on
    a directory laid out like the reference's datasets."""
    from taco_amd import alignment as A
    rec, scripts, vec = fixture()
    got = A.align_text_batch(rec, scripts, vec["score_threshold"])
    assert list(got) == list(rec) and len(vec["results"]) == 298
    for path, want in vec["results"].items():
        assert got[path] == want, path
    for u in vec["unrecorded"]:                              # the reference needs the jamo package there: held to the Python restatement
        v = got[u["path"]]
        assert isinstance(v, list) and v[-1] == rec[u["path"]] and len(v) in (1, 2)
    # the same through difflib on the host, all 310 of them
    orig = A._device_scores
    try:
        A._device_scores = lambda *a, **k: R.scores(*a, count=R.difflib_count, **k)
        assert A.align_text_batch(rec, scripts, vec["score_threshold"]) == got
    finally:
        A._device_scores = orig

    root = tmp_path / "datasets" / "moon"
    shutil.copytree(os.path.join(GOLD, "align_moon"), str(root))
    spec = importlib.util.spec_from_file_location("align_text_tool", os.path.join(HERE, "..", "tools", "align_text.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    cwd = os.getcwd()
    os.chdir(str(tmp_path))                                  # the audio paths of recognition.json lead to the scripts from here ...
    try:
        tool.main(["--recognition_path", "./datasets/moon/recognition.json"])
    finally:
        os.chdir(cwd)
    # ... and from anywhere else they are found in `assets` beside recognition.json; the first alignment.json is backed up
    tool.main(["--recognition_path", str(root / "recognition.json"), "--alignment_filename", "alignment.json", "--score_threshold", "0.4"])
    with open(str(root / "alignment.json"), encoding="utf-8") as f:
        written = json.load(f)
    assert written == got and list(written) == sorted(written)
    backups = [n for n in os.listdir(str(root)) if n.startswith("alignment.backup_") and n.endswith(".json")]
    assert len(backups) == 1
    with open(str(root / backups[0]), encoding="utf-8") as f:
        assert json.load(f) == got
