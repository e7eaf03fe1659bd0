"""Matching recognised text to script lines (taco_text_matches / taco_text_best_two, taco_amd.alignment; recognition/alignment.py), the
part that needs no GPU: the dense restatement the kernel is specified by against difflib, the cap at len(b) = 199, the C ABI (symbols,
prototypes, declarations, every argument error -- all returned before any HIP call), and the Python logic on hand-written cases and on the
reference's own results (tests/golden/alignment_vectors.json).  The kernels are held to difflib in tests/test_gpu_align.py."""
import ctypes as C
import difflib
import json
import os
import random
import re

import pytest

import align_reference as R
from taco_amd import _lib, alignment as A

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
HEADER = os.path.join(HERE, "..", "include", "taco_abi.h")
LANE_EDGES = (0, 1, 63, 64, 65, 127, 128, 129, 199)


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


def rand_text(rs, n, alphabet):
    return "".join(rs.choice(alphabet) for _ in range(n))


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_difflib_on_fixture_pairs():
    rec, scripts, _ = fixture()
    rs = random.Random(3)
    n = 0
    for name, lines in scripts.items():
        cands = [A.plain_text(c) for c in A.clean_candidates(lines)]
        utts = [A.plain_text(t) for p, t in rec.items() if A.script_of(p)[1] == name]
        for u in rs.sample(utts, min(len(utts), 12)):
            for c in rs.sample(cands, min(len(cands), 40)):
                assert R.match_count(c, u) == R.difflib_count(c, u), (c, u)
                n += 1
    assert n > 500


@pytest.mark.parametrize("alphabet", ["ab", "abc"])
def test_restatement_equals_difflib_where_ties_are_everywhere(alphabet):
    rs = random.Random(len(alphabet))
    for lb in LANE_EDGES:
        for la in (0, 1, 2, 3, 17, 64, 65, 150, 300):
            a, b = rand_text(rs, la, alphabet), rand_text(rs, lb, alphabet)
            assert R.match_count(a, b) == R.difflib_count(a, b), (a, b)
    assert A.ratio_of(R.match_count("", ""), 0) == difflib.SequenceMatcher(None, "", "").ratio() == 1.0


def test_the_cap_difflib_changes_behaviour_at_200(monkeypatch):
    """Random 8-letter strings from random.Random(0): at len(b) = 199 the restatement is difflib; at 200 and 201 every letter of b is
    'popular' (more than 1 + len(b)//100 occurrences), autojunk empties difflib's index and it matches nothing, the restatement 52.
    The public match_counts equals difflib there all the same: the device refuses such a pair and the host scores it."""
    for lb in (199, 200, 201):
        rs = random.Random(0)
        a, b = rand_text(rs, 150, "abcdefgh"), rand_text(rs, lb, "abcdefgh")
        if lb == 199:
            assert R.match_count(a, b) == R.difflib_count(a, b)
            continue
        assert R.match_count(a, b) == 52 and R.difflib_count(a, b) == 0
        monkeypatch.setattr(A, "_device_scores", R.scores)
        got = A.match_counts([a, "xyz"], [b, b[:50]], [(0, 0), (0, 1), (1, 0)])
        assert got.tolist() == [0, R.difflib_count(a, b[:50]), 0]
        assert R.scores([a, b], [(0, 1)])[0].tolist() == [-1]


# ------------------------------------------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_prototypes():
    lib = _lib.load_library()
    assert lib.taco_abi_version() == 1                  # additive: the version stays
    P, I, LL = C.c_void_p, C.c_int, C.c_longlong
    want = {"taco_text_matches": [P, P, LL, P, I, P, I, P], "taco_text_best_two": [P, P, P, P, I, P, I, P],
            "taco_debug_text_matches_cols": [P, P, LL, P, I, P, I, P, I]}
    for name, args in want.items():
        assert name in _lib.PROTOTYPES
        fn = getattr(lib, name)
        assert fn.restype is I and list(fn.argtypes) == args, name


def test_header_declarations_and_their_comment():
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+taco_text_matches\s*\(([^;]*)\)\s*;\s*int\s+taco_text_best_two\s*\(([^;]*)\)\s*;", text, flags=re.S)
    assert m, "not declared"
    comment = re.sub(r"\s+", " ", m.group(1).replace("\n *", " "))
    strip = lambda s: [re.sub(r"\s+", " ", a).strip() for a in re.sub(r"/\*.*?\*/", "", s, flags=re.S).split(",")]
    assert strip(m.group(2)) == ["void* hip_stream", "const int32_t* d_chars", "long long n_chars", "const int32_t* d_offsets", "int n_texts",
                                 "const int32_t* d_pairs", "int n_pairs", "int32_t* d_matches"]
    assert strip(m.group(3)) == ["void* hip_stream", "const int32_t* d_matches", "const int32_t* d_pairs", "const int32_t* d_offsets", "int n_texts",
                                 "const int32_t* d_group_offsets", "int n_groups", "int32_t* d_best"]
    for words in ("recognition/alignment.py:21-26,107-113", "starts earliest in a", "starts earliest in b", "len(b) <= 199", "autojunk", "-1 convention",
                  "REFUSED", "stream capture", "TACO_ERR_ARG", "{-1, 0, 0, 0}"):
        assert words in comment, words
    dbg = open(os.path.join(HERE, "..", "include", "taco_debug.h")).read()
    assert re.search(r"int\s+taco_debug_text_matches_cols\s*\(", dbg)


def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory: validation rejects every one of these calls before it is touched."""
    lib = _lib.load_library()
    CH, OF, PA, MA, GO, BE = (k << 24 for k in range(1, 7))               # 16 MiB apart: disjoint for every size used here
    v = lambda x: C.c_void_p(x) if x else None

    def matches(ch=CH, n_chars=100, of=OF, n_texts=5, pa=PA, n_pairs=7, ma=MA, fn=lib.taco_text_matches, extra=()):
        rc = fn(None, v(ch), n_chars, v(of), n_texts, v(pa), n_pairs, v(ma), *extra)
        return rc, lib.taco_last_error()

    def best(ma=MA, pa=PA, of=OF, n_texts=5, go=GO, n_groups=3, be=BE):
        rc = lib.taco_text_best_two(None, v(ma), v(pa), v(of), n_texts, v(go), n_groups, v(be))
        return rc, lib.taco_last_error()

    for kw in (dict(ch=0), dict(of=0), dict(pa=0), dict(ma=0)):
        rc, msg = matches(**kw)
        assert rc == _lib.TACO_ERR_ARG and b"null" in msg, kw
    for kw in (dict(n_chars=-1), dict(n_texts=-1), dict(n_pairs=-1), dict(n_pairs=-2 ** 31), dict(n_chars=-2 ** 63)):
        rc, msg = matches(**kw)
        assert rc == _lib.TACO_ERR_ARG and b">= 0" in msg, kw
    for kw in (dict(ma=CH), dict(ma=CH + 396), dict(ma=CH - 24), dict(ma=OF + 20), dict(ma=PA + 52), dict(ma=PA - 4), dict(ch=MA + 24, n_chars=1)):
        rc, msg = matches(**kw)
        assert rc == _lib.TACO_ERR_ARG and b"overlap" in msg, kw
    # a pool whose byte count does not fit 64 bits is not mistaken for a small one
    rc, msg = matches(ch=8, n_chars=2 ** 63 - 1)
    assert rc == _lib.TACO_ERR_ARG and b"overlap" in msg
    # no pairs: nothing to do, and a null pool is fine without characters
    assert matches(n_pairs=0) == (0, lib.taco_last_error()) and matches(ch=0, n_chars=0, n_pairs=0)[0] == 0
    for cols in (1, 2, 3, 5, -1):
        rc, msg = matches(fn=lib.taco_debug_text_matches_cols, extra=(cols,))
        assert rc == _lib.TACO_ERR_ARG and b"cols" in msg
    assert matches(fn=lib.taco_debug_text_matches_cols, extra=(4,), n_pairs=0)[0] == 0

    for kw in (dict(ma=0), dict(pa=0), dict(of=0), dict(go=0), dict(be=0)):
        rc, msg = best(**kw)
        assert rc == _lib.TACO_ERR_ARG and b"null" in msg, kw
    for kw in (dict(n_texts=-1), dict(n_groups=-1)):
        rc, msg = best(**kw)
        assert rc == _lib.TACO_ERR_ARG and b">= 0" in msg, kw
    for kw in (dict(be=OF), dict(be=OF + 20), dict(be=GO + 12), dict(be=GO - 44), dict(be=MA), dict(be=MA - 44), dict(be=PA - 40), dict(be=PA + 4)):
        rc, msg = best(**kw)
        assert rc == _lib.TACO_ERR_ARG and b"overlap" in msg, kw
    assert best(n_groups=0)[0] == 0
    # buffers that touch but do not overlap pass the checks (no pairs / groups: still no device call)
    assert matches(ma=CH + 400, n_pairs=0)[0] == 0 and best(be=GO + 4, n_groups=0)[0] == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the Python logic
# ------------------------------------------------------------------------------------------------------------------------------
def test_plain_text_add_punctuation_similarity():
    assert A.plain_text("  안녕, 하세요!  \n") == "안녕하세요" and A.plain_text("a.b c\td") == "abcd" and A.plain_text(" ") == ""
    assert A.plain_text("“따옴표”…") == "“따옴표”…"                      # only ASCII punctuation goes
    assert A.add_punctuation("했습니다") == "했습니다." and A.add_punctuation("했습니다.") == "했습니다." and A.add_punctuation("네") == "네"
    assert A.similarity("가 나, 다", "가나다") == 1.0 and A.similarity("", " .") == 1.0
    assert A.similarity("abcd", "bcde") == difflib.SequenceMatcher(None, "abcd", "bcde").ratio() == 0.75
    _, _, vec = fixture()
    for a, b, want in vec["similarity"]:
        assert A.similarity(a, b) == want
        assert A.ratio_of(R.difflib_count(A.plain_text(a), A.plain_text(b)), len(A.plain_text(a)) + len(A.plain_text(b))) == want
    for text, want in vec["plain_text"]:
        assert A.plain_text(text) == want


def test_search_optimal_branch_by_branch():
    so = A.search_optimal
    assert so("가나 다라, 마바.", "다라 마바") == "다라 마바"                     # contained, punctuation aside: the recognised text as it is
    assert so("하나 둘 셋 넷 다섯.", "둘 셋 넷넷") == "둘 셋 넷 다섯."            # cut at the first word; the last word is not in the line
    assert so("하나 둘 셋 넷, 다섯.", "둘 삼 넷") == "둘 셋 넷,"                  # first and last word: the mark after the last word stays
    assert so("하나 둘 셋 넷 다섯", "둘 삼 넷") == "둘 셋 넷"                     # ... and a letter after it does not
    assert so("하나 둘 셋 넷", "영 삼 넷") == "하나 둘 셋 넷"                     # the last word alone
    assert so("하나 둘 셋", "넷 다섯") is None                                     # neither
    assert so("가 나 다 라", "가나 x") == "가 나 다 라"                              # the first two words of the line joined
    assert so("가나다 라마 바", "다라마 x") == "나다 라마 바"                        # ... the cut then lands one character early, as in the reference
    assert so("그는 바로이 자리에서 했다", "바로 이 자리 끝") == "바로이 자리에서 했다"  # the first two words of the utterance joined
    assert so("그는 바로 이 자리에서 했다", "바로이 자리 끝") is None                 # joined in the utterance only, deeper in the line: not found
    assert so("가 나", "가나 다") == "가 나"                                        # a two-word line, joined
    assert so("", "가") is None
    _, _, vec = fixture()
    assert len(vec["search_optimal"]) > 30
    for found, rec, want in vec["search_optimal"]:
        assert so(found, rec) == want, (found, rec)


def test_candidates_and_the_script_of_a_path():
    assert A.clean_candidates([' "가" \n', "가", "", "나'다\n", "\n"]) == ["가", "", "나다"]
    assert A.script_of("./datasets/moon/audio/005.0012.wav") == ("./datasets/moon/assets/005.txt", "005")
    assert A.script_of("d/audio/a.b.0001.mp3") == ("d/assets/a.b.txt", "a.b")


@pytest.fixture
def host_scores(monkeypatch):
    monkeypatch.setattr(A, "_device_scores", lambda *a, **k: R.scores(*a, count=R.difflib_count, **k))


def test_align_texts_decisions(host_scores):
    lines = ["오늘은 날씨가 좋습니다.", "내일은 비가 옵니다", "내일은 비가 옵니다", ' "모레는 눈이 옵니다" ']
    got = A.align_texts(lines, ["날씨가 좋습니다", "내일은 비가 옵니까", "전혀 다른 말", "비가"], 0.4)
    assert got[0] == "날씨가 좋습니다."                       # contained -> the recognised text, full stop added
    assert got[1] == "내일은 비가 옵니다."                    # duplicates collapsed: no tie with itself; cut from the line
    assert got[2] == ["전혀 다른 말"]                         # under the threshold
    assert got[3] == "비가"                                   # 2*2/10 = 0.4: the threshold itself passes (>=); contained
    assert A.align_texts(lines, ["비가"], 0.41) == [["비가"]]
    # the tie at the top: two different lines score the same -> nothing is aligned, whichever comes first
    for cands in (["가나다라 x", "가나다라 y", "zzz"], ["zzz", "가나다라 y", "가나다라 x"]):
        assert A.align_texts(cands, ["가나다라"], 0.1) == [["가나다라"]]
    # lines that differ only in what plain_text removes tie as well
    assert A.align_texts(["가나, 다", "가나 다", "q"], ["가나다"], 0.1) == [["가나다"]]
    # a tie below the top does not matter
    assert A.align_texts(["가나다라마", "가나x", "가나y"], ["가나다라"], 0.1) == ["가나다라"]
    # nothing can be cut out and the symbol counts are close: both texts; far apart: the recognised text alone
    assert A.align_texts(["일이삼사 오육칠팔", "zzzz"], ["이일 삼사오 팔칠"], 0.1) == [["일이삼사 오육칠팔", "이일 삼사오 팔칠"]]
    assert A.align_texts(["일이삼사 오육칠팔다", "zzzz"], ["이일 삼사오 팔칠"], 0.1) == [["일이삼사 오육칠팔다.", "이일 삼사오 팔칠"]]
    assert A.align_texts(["일이삼사 오육칠팔 아야어여오요우유", "zzzz"], ["이일 삼사오 팔칠"], 0.1) == [["이일 삼사오 팔칠"]]      # 8 syllables = 16 symbols more
    assert A.align_texts(["a", "b"], []) == []
    for cands in ([], ["가"], ["가", " 가 ", '"가"']):
        with pytest.raises(ValueError):
            A.align_texts(cands, ["가"])


def test_an_utterance_past_the_cap_goes_to_the_host(host_scores):
    rs = random.Random(0)
    a, b = rand_text(rs, 150, "abcdefgh"), rand_text(rs, 200, "abcdefgh")
    # difflib's own answer at 200 characters: autojunk finds nothing in `a`, only the identical line scores
    assert A.align_texts([a, b, "q"], [b], 0.4) == [b]
    assert difflib.SequenceMatcher(None, a, b).ratio() == 0.0


def test_align_text_batch_equals_the_reference_results(host_scores):
    rec, scripts, vec = fixture()
    assert len(rec) == 310 and len(vec["results"]) + len(vec["unrecorded"]) == 310
    got = A.align_text_batch(rec, scripts, vec["score_threshold"])
    assert list(got) == list(rec)
    for path, want in vec["results"].items():
        assert got[path] == want, path
    # the utterances the reference could not be run on (its symbol count needs the jamo package): the line was chosen, nothing could be cut out
    for u in vec["unrecorded"]:
        v = got[u["path"]]
        assert v == [rec[u["path"]]] or (isinstance(v, list) and len(v) == 2 and v[1] == rec[u["path"]]), u
    with pytest.raises(KeyError):
        A.align_text_batch(rec, {"005": scripts["005"]})


def test_decide_is_the_top_two_of_sorted():
    assert A.decide([0.1, 0.5, 0.3]) == (1, True) and A.decide([0.5, 0.5, 0.3])[1] is False and A.decide([0.2, 0.5, 0.2]) == (1, True)
    assert R.best_two([3, 3, -1], [10, 10, 4]) == (0, 3, 10, 0) and R.best_two([3, 2], [10, 10]) == (0, 3, 10, 1)
    assert R.best_two([], []) == (-1, 0, 0, 0) and R.best_two([0, 0], [0, 5]) == (0, 0, 0, 1) and R.best_two([-1], [3]) == (-1, 0, 0, 0)
