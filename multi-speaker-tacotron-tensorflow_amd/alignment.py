"""Matching recognised utterances to the lines of the speaker's script: step 3 of the reference's data pipeline
(recognition/alignment.py), between speech recognition and the training targets.  Behaviour re-authored, nothing copied.

Every (script line, utterance) pair of a script is scored with difflib.SequenceMatcher(None, a, b).ratio() = 2*M/(len(a)+len(b)) in the
reference (:21-26,107-108).  The matched-character count M of every pair comes from the device here (taco_text_matches: one wavefront
per pair, exact equality with difflib for len(b) <= 199), and so does the top-two decision per utterance (taco_text_best_two, :109-113).
The ratio itself is formed on the host as 2.0 * M / T in Python floats, which makes the threshold test and every score bit-equal to
difflib's.  What the device refuses -- an utterance of 200 characters or more, where difflib's autojunk changes what it finds -- is
scored with difflib on the host.  The string logic around the scores (plain_text, search_optimal, add_punctuation) is host code."""
import difflib
import os
import string

import numpy as np
import torch

from . import _lib
from ._device import STREAM, call, tensor

_PUNCTUATION = str.maketrans({c: None for c in string.punctuation})


def plain_text(text):
    """:12-13: stripped, ASCII punctuation removed, all white space removed."""
    return "".join(text.strip().translate(_PUNCTUATION).split())


def add_punctuation(text):
    """:15-19: a sentence that ends in '다' gets its full stop."""
    return text + "." if text.endswith("다") else text


def host_match_count(a, b):
    """M of difflib for two strings as they are: the total size of its matching blocks."""
    return sum(m.size for m in difflib.SequenceMatcher(None, a, b).get_matching_blocks())


def ratio_of(M, T):
    """difflib's ratio() from its matched count M and T = len(a) + len(b), in its own arithmetic (1.0 when both are empty)."""
    return 2.0 * M / T if T else 1.0


def similarity(text_a, text_b):
    """:21-26: one ratio on the host (the batched form is match_counts / align_texts)."""
    return difflib.SequenceMatcher(None, plain_text(text_a), plain_text(text_b)).ratio()


def _head_joined_texts(text):
    """the text, and the text with its first two words written as one (:36-46)"""
    words = text.split()
    if len(words) < 2:
        return [text]
    return [text, " ".join([words[0] + words[1]] + words[2:])]


def _head_words(text):
    """the first word, and the first two written as one (:28-34)"""
    words = text.split()
    return [words[0], words[0] + words[1]] if len(words) > 1 else [words[0]]


def search_optimal(found_text, recognition_text):
    """:48-90: the part of the script line `found_text` that the utterance covers, or None.  The recognised text wins as it is when the
    line contains it (punctuation and spaces aside); otherwise the line is cut to start at the utterance's first word (also tried with
    the first two words of either text joined) and to end with its last word plus the punctuation mark that follows it in the line."""
    if plain_text(recognition_text) in plain_text(found_text):
        return recognition_text
    hit = False
    for variant in _head_joined_texts(found_text):
        word = next((w for w in _head_words(recognition_text) if w in variant), None)
        if word is not None:
            start = variant.find(word)
            if variant != found_text:                  # a space of the line is missing in the joined variant
                start = max(0, start - 1)
            found_text = found_text[start:].strip()
            hit = True
            break
    last = recognition_text.split()[-1]
    if last in found_text:
        end = found_text.find(last) + len(last)
        mark = found_text[end] if end < len(found_text) and found_text[end] in string.punctuation else ""
        found_text = found_text[:end] + mark
        hit = True
    return found_text if hit else None


# ------------------------------------------------------------------------------------------------------------------------------
# the device calls
# ------------------------------------------------------------------------------------------------------------------------------
def pack_texts(texts):
    """strings -> (code points int32 [n_chars], offsets int32 [len(texts) + 1]): the pool of taco_text_matches"""
    offsets = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=offsets[1:])
    if offsets[-1] > 2 ** 31 - 1:
        raise ValueError("the texts hold %d characters, offsets are 32-bit" % offsets[-1])
    chars = np.frombuffer("".join(texts).encode("utf-32-le", "surrogatepass"), np.int32).copy()
    return chars, offsets.astype(np.int32)


def _device_scores(texts, pairs, group_offsets=None, device=None):
    """taco_text_matches (and taco_text_best_two when group_offsets is given) on the current stream -> (matches [n_pairs], best
    [n_groups, 4] or None) as NumPy arrays."""
    lib = _lib.load_library()
    dev = torch.device(device or "cuda:0")
    chars, offsets = pack_texts(texts)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    n_pairs = len(pairs)
    up = lambda x, what: tensor(x, dev, torch.int32, what)
    d_chars, d_off = up(chars if len(chars) else np.zeros(1, np.int32), "chars"), up(offsets, "offsets")
    d_pairs = up(pairs if n_pairs else np.zeros((1, 2), np.int32), "pairs")
    d_m = torch.empty(max(n_pairs, 1), dtype=torch.int32, device=dev)
    call(dev, lib.taco_text_matches, STREAM, d_chars, len(chars), d_off, len(texts), d_pairs, n_pairs, d_m)
    best = None
    if group_offsets is not None:
        g = np.ascontiguousarray(group_offsets, np.int32)
        d_best = torch.empty((max(len(g) - 1, 1), 4), dtype=torch.int32, device=dev)
        call(dev, lib.taco_text_best_two, STREAM, d_m, d_pairs, d_off, len(texts), up(g, "group_offsets"), len(g) - 1, d_best)
        best = d_best[:len(g) - 1].cpu().numpy()
    return d_m[:n_pairs].cpu().numpy(), best


def match_counts(texts_a, texts_b, pairs, device=None):
    """M of difflib.SequenceMatcher(None, texts_a[i], texts_b[j]) for every (i, j) of `pairs`, int64 [n_pairs].  The strings are compared
    as they are (apply plain_text first for the reference's similarity).  Computed on the device; the pairs it refuses
    (len(texts_b[j]) >= 200) are recomputed with difflib on the host, so every value equals difflib's."""
    texts_a, texts_b = list(texts_a), list(texts_b)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    if len(pairs) and (pairs.min() < 0 or pairs[:, 0].max() >= len(texts_a) or pairs[:, 1].max() >= len(texts_b)):
        raise IndexError("a pair names a text that does not exist")
    if not len(pairs):
        return np.zeros(0, np.int64)
    m, _ = _device_scores(texts_a + texts_b, pairs + np.array([0, len(texts_a)]), device=device)
    m = m.astype(np.int64)
    for p in np.nonzero(m < 0)[0]:
        m[p] = host_match_count(texts_a[pairs[p, 0]], texts_b[pairs[p, 1]])
    return m


def clean_candidates(lines):
    """:104-108: script lines stripped, quotation marks removed, duplicates collapsed in order of first appearance."""
    return list(dict.fromkeys(line.strip().replace('"', "").replace("'", "") for line in lines))


def decide(ratios):
    """:109-113 on one utterance's scores in candidate order: (index of the best, whether it is strictly ahead of every other)."""
    order = sorted(range(len(ratios)), key=lambda i: ratios[i])[::-1]
    return order[0], ratios[order[0]] > ratios[order[1]]


def _result(found_text, recognition_text, normalizer):
    """:114-129 once a line is chosen: the aligned text, or both texts for a person to pick from, or None (nothing usable)."""
    from .text import text_to_sequence
    aligned = search_optimal(found_text, recognition_text)
    if aligned is not None:
        return add_punctuation(aligned)
    if abs(len(text_to_sequence(found_text, normalizer)) - len(text_to_sequence(recognition_text, normalizer))) > 10:
        return None
    return [add_punctuation(found_text), recognition_text]


def _align_groups(groups, score_threshold, normalizer, device):
    """groups: [(candidates as cleaned, recognition texts)] -> per group the list of result values.  One pool, one launch of each
    kernel for all groups."""
    from .korean import KoreanNormalizer
    normalizer = normalizer if normalizer is not None else KoreanNormalizer()
    texts, pairs, group_offsets, where = [], [], [0], []
    for gi, (cands, recs) in enumerate(groups):
        if len(cands) < 2:
            raise ValueError("a script needs at least two distinct lines to align against, got %d" % len(cands))
        c0 = len(texts)
        texts.extend(plain_text(c) for c in cands)
        for ui, rec in enumerate(recs):
            texts.append(plain_text(rec))
            pairs.append(np.stack([np.arange(c0, c0 + len(cands)), np.full(len(cands), len(texts) - 1)], 1))
            group_offsets.append(group_offsets[-1] + len(cands))
            where.append((gi, ui))
    out = [[None] * len(recs) for _, recs in groups]
    if not where:
        return out
    pairs = np.concatenate(pairs)
    matches, best = _device_scores(texts, pairs, group_offsets, device)
    for (gi, ui), g0, g1, (bp, M, T, flag) in zip(where, group_offsets[:-1], group_offsets[1:], best):
        cands, rec = groups[gi][0], groups[gi][1][ui]
        if (matches[g0:g1] < 0).any():                     # a refused pair (an utterance of 200 characters or more): this group on the host
            ratios = [ratio_of(m if m >= 0 else host_match_count(texts[a], texts[b]), len(texts[a]) + len(texts[b]))
                      for m, (a, b) in zip(matches[g0:g1], pairs[g0:g1])]
            idx, ahead = decide(ratios)
            score = ratios[idx]
        else:
            idx, ahead, score = int(bp) - g0, bool(flag), ratio_of(int(M), int(T))
        value = _result(cands[idx], rec, normalizer) if ahead and score >= score_threshold else None
        out[gi][ui] = value if value is not None else [rec]
    return out


def align_texts(candidates, recognition_texts, score_threshold=0.4, normalizer=None, device=None):
    """The body of align_text_fn (:104-136) for one script: `candidates` are its lines, `recognition_texts` the recognised utterances.
    Returns per utterance the reference's result value: the aligned text (str), [script line, recognised text] where no part of the line
    could be cut out, or [recognised text] where no line is strictly best, the best is under score_threshold, or the two texts differ by
    more than ten symbols.  `normalizer` (korean.KoreanNormalizer, with the caller's dictionaries) serves that symbol count.  Raises
    ValueError for fewer than two distinct candidates (the reference: IndexError at :111)."""
    return _align_groups([(clean_candidates(candidates), list(recognition_texts))], score_threshold, normalizer, device)[0]


def script_of(audio_path):
    """:101-102: the script an audio path belongs to -- 'audio' becomes 'assets' in the path, the segment number goes, the extension
    becomes .txt: './datasets/moon/audio/005.0012.wav' -> ('./datasets/moon/assets/005.txt', '005')."""
    head, number, ext = audio_path.replace("audio", "assets").rsplit(".", 2)
    path = os.path.splitext(head + "." + ext)[0] + ".txt"
    return path, os.path.splitext(os.path.basename(path))[0]


def align_text_batch(recognition, scripts, score_threshold=0.4, normalizer=None, device=None):
    """:138-158: `recognition` is the mapping recognition.json holds (audio path -> recognised text), `scripts` maps a script's name
    (script_of(path)[1]) to its lines.  Returns {audio path: result value} in the order of `recognition`, what the reference writes to
    alignment.json."""
    by_script = {}
    for path, text in recognition.items():
        by_script.setdefault(script_of(path)[1], []).append((path, text))
    missing = sorted(set(by_script) - set(scripts))
    if missing:
        raise KeyError("no script lines for %s" % ", ".join(missing))
    names = list(by_script)
    values = _align_groups([(clean_candidates(scripts[n]), [t for _, t in by_script[n]]) for n in names], score_threshold, normalizer, device)
    found = {path: v for n, vals in zip(names, values) for (path, _), v in zip(by_script[n], vals)}
    return {path: found[path] for path in recognition}
