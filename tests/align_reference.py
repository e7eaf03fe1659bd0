"""The matched-character count of difflib.SequenceMatcher(None, a, b) restated as a dense run-length recurrence in NumPy: the
specification of k_text_matches (csrc/taco_align.h), and of k_text_best_two in exact rational arithmetic.

L[i][j] = L[i-1][j-1] + 1 where a[i] == b[j], else 0, evaluated inside the current sub-rectangle a[alo:ahi] x b[blo:bhi] only, so that a
run never crosses alo or blo.  The best block is the one of the largest length, then the smallest start in a, then the smallest start
in b (difflib's tie rule); its length is added, and the pieces left of it in both strings and right of it in both strings follow.
Equal to difflib for len(b) <= 199; from 200 on difflib's autojunk takes popular characters of b out of its index and the two differ."""
import difflib
from fractions import Fraction

import numpy as np

MAX_B = 199


def codes(s):
    return np.frombuffer(s.encode("utf-32-le", "surrogatepass"), np.int32) if not isinstance(s, np.ndarray) else s


def longest_block(a, b, alo, ahi, blo, bhi):
    """(start in a, start in b, length) of the best block of a[alo:ahi] and b[blo:bhi]; length 0 when nothing matches"""
    eq = a[alo:ahi, None] == b[None, blo:bhi]
    best, run = (0, 0, 0), np.zeros(bhi - blo, np.int64)
    for r in range(ahi - alo):
        run = np.where(eq[r], np.concatenate([[0], run[:-1]]) + 1, 0)          # the diagonal: one column to the right per row
        m = int(run.max()) if run.size else 0
        if m > best[2]:          # strict: of equal lengths the earliest row stays (earliest start in a); argmax: the earliest column
            j = int(run.argmax())
            best = (alo + r - m + 1, blo + j - m + 1, m)
    return best


def match_count(a, b):
    """M: the total length of the matching blocks"""
    a, b = codes(a), codes(b)
    total, todo = 0, [(0, len(a), 0, len(b))]
    while todo:
        alo, ahi, blo, bhi = todo.pop()
        if alo >= ahi or blo >= bhi:
            continue
        i, j, k = longest_block(a, b, alo, ahi, blo, bhi)
        if k:
            total += k
            todo.append((alo, i, blo, j))
            todo.append((i + k, ahi, j + k, bhi))
    return total


def difflib_count(a, b):
    return sum(m.size for m in difflib.SequenceMatcher(None, a, b).get_matching_blocks())


def ratio_fraction(M, T):
    return Fraction(2 * M, T) if T else Fraction(1)


def best_two(matches, totals):
    """k_text_best_two for one group: (index of the first pair of the largest ratio, its M, its T, flag) over the pairs with matches >= 0;
    the flag is 0 when another pair's ratio is not strictly smaller or the group holds a refused pair; (-1, 0, 0, 0) without a pair."""
    live = [i for i, m in enumerate(matches) if m >= 0]
    if not live:
        return (-1, 0, 0, 0)
    r = {i: ratio_fraction(int(matches[i]), int(totals[i])) for i in live}
    top = max(r.values())
    i = min(k for k in live if r[k] == top)
    alone = sum(1 for k in live if r[k] == top) == 1 and len(live) == len(matches)
    return (i, int(matches[i]), int(totals[i]), int(alone))


def scores(texts, pairs, group_offsets=None, device=None, count=match_count):
    """What taco_amd.alignment._device_scores returns, computed here: -1 for len(b) >= 200.  count: the restatement, or difflib_count
    (equal below the cap and much faster) where a test is about the logic around the scores."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    m = np.array([count(texts[a], texts[b]) if len(texts[b]) <= MAX_B else -1 for a, b in pairs], np.int32)
    if group_offsets is None:
        return m, None
    T = [len(texts[a]) + len(texts[b]) for a, b in pairs]
    best = []
    for g0, g1 in zip(group_offsets[:-1], group_offsets[1:]):
        i, M, Tt, f = best_two(m[g0:g1], T[g0:g1])
        best.append((i + g0 if i >= 0 else -1, M, Tt, f))
    return m, np.array(best, np.int32).reshape(-1, 4)
