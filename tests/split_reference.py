"""Float64 restatement of the reference's audio/silence.py:21-76 -- `librosa.effects.split`, `remove_breath` and
`split_on_silence_with_librosa` without its file I/O -- test infrastructure only: nothing in the product imports it.

UNPINNED on librosa.  The reference pins librosa==0.5.1; librosa is not a dependency of this project and is not available to its
tests, so this file restates the documented algorithm and could NOT be checked against librosa's source or output.  What it
restates, for `split(y, top_db, ref=np.max, frame_length, hop_length)`:

  1. mse, db and non_silent = db > -top_db exactly as tests/trim_reference.py has them for `trim` (frame_mse: np.pad, explicit frames,
     rfft of the windowed frames for the 0.5.x energy, the unwindowed mean square for the >= 0.6 one).
  2. edges = flatnonzero(diff(non_silent)) + 1; a 0 is prepended if non_silent[0]; len(non_silent) is appended if non_silent[-1];
     edges = frames_to_samples(edges, hop_length) = edges * hop_length; edges = minimum(edges, len(y)); edges.reshape(-1, 2).

Written the long way on purpose -- np.diff, flatnonzero, in-place muting on a view of the array, exactly as the reference does it -- so
that it checks the shortcuts the kernels take (a prefix count of state changes; sums and a running total instead of re-evaluated
means).  A row of fewer than two samples has nothing to reflect: no frames, no intervals (include/taco_abi.h).

Every result carries the margins that make a comparison for equality meaningful: the smallest |db + top_db| over the frames it
looked at, and the smallest |abs_mean_k - (running_mean - threshold)| over the decisions it took (inf where there was none)."""
import numpy as np

import trim_reference as T

ENERGIES = T.ENERGIES
INF = float("inf")


def runs_of(non_silent, n, hop_length):
    """Steps 2 above on a boolean frame pattern: int64 [K, 2]."""
    non_silent = np.asarray(non_silent, bool)
    if len(non_silent) == 0:
        return np.zeros((0, 2), np.int64)
    edges = [np.flatnonzero(np.diff(non_silent.astype(int))) + 1]
    if non_silent[0]:
        edges.insert(0, [0])
    if non_silent[-1]:
        edges.append([len(non_silent)])
    edges = np.concatenate(edges).astype(np.int64) * hop_length          # frames_to_samples
    edges = np.minimum(edges, n)
    return edges.reshape((-1, 2))


def split(y, top_db=60, frame_length=2048, hop_length=512, energy="spectral"):
    """-> (intervals int64 [K, 2], db [1 + n // hop] float64, margin: the smallest |db + top_db|, inf for no frames)."""
    y = np.asarray(y, np.float64)
    n = len(y)
    if n < 2:
        return np.zeros((0, 2), np.int64), np.zeros(0), INF
    mse = T.frame_mse(y, frame_length, hop_length, energy)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
    return runs_of(db > -top_db, n, hop_length), db, float(np.abs(db + top_db).min())


def abs_mean(x):
    return float(np.abs(x).mean()) if len(x) else float("nan")      # NumPy's mean of nothing is NaN (and a warning)


def remove_breath(audio, top_db=40, frame_length=128, hop_length=32, threshold=0.05, energy="spectral", frozen_mean=False, edges=None):
    """audio/silence.py:21-31 on a float64 copy, muting IN PLACE as the reference does, so that abs_mean(audio) moves with every mute.
    frozen_mean=True is a control only: the mean taken once, before any mute.  edges (int [K, 2]) replaces the split's answer, for a test
    that writes the interval table by hand.
    -> (audio after the mutes, dict(intervals [K, 2], muted bool [K], abs_mean float64 [1 + K]: the row's mean before any mute, then
    each interval's (NaN for an empty one), db_margin, decision_margin))."""
    audio = np.array(audio, np.float64, copy=True)
    if edges is None:
        edges, _, db_margin = split(audio, top_db, frame_length, hop_length, energy)
    else:
        edges, db_margin = np.asarray(edges, np.int64).reshape(-1, 2), INF
    first = abs_mean(audio)
    muted = np.zeros(len(edges), bool)
    means = [first]
    decision = INF
    for idx in range(len(edges)):
        start_idx, end_idx = edges[idx][0], edges[idx][1]
        m = abs_mean(audio[start_idx:end_idx])
        means.append(m)
        if start_idx < len(audio):
            bar = (first if frozen_mean else abs_mean(audio)) - threshold
            decision = min(decision, abs(m - bar))
            if m < bar:
                audio[start_idx:end_idx] = 0
                muted[idx] = True
    return audio, dict(intervals=edges, muted=muted, abs_mean=np.array(means, np.float64), db_margin=db_margin, decision_margin=decision)


def split_on_silence(audio, sample_rate, top_db=40, frame_length=1024, hop_length=256, skip_idx=0, min_segment_length=3, max_segment_length=8,
                     energy="spectral", threshold=0.05):
    """audio/silence.py:33-76 without load_audio / save_audio.  -> dict(no_breath float64 [n], first: the first split's intervals, second:
    the second split's, kept: [(idx, start, end)] with the reference's idx, db_margin and decision_margin: the smallest over both
    splits of the recording and over every interval's remove_breath)."""
    audio = np.asarray(audio, np.float64)
    edges, _, db_margin = split(audio, top_db, frame_length, hop_length, energy)
    first = edges
    decision = INF
    new_audio = np.zeros_like(audio)
    for idx, (start, end) in enumerate(edges[skip_idx:]):
        new_audio[start:end], info = remove_breath(audio[start:end], energy=energy, threshold=threshold)
        db_margin, decision = min(db_margin, info["db_margin"]), min(decision, info["decision_margin"])
    audio = new_audio
    edges, _, m2 = split(audio, top_db, frame_length, hop_length, energy)
    kept = []
    for idx, (start, end) in enumerate(edges[skip_idx:]):
        duration = len(audio[start:end]) / float(sample_rate)
        if duration <= min_segment_length or duration >= max_segment_length:
            continue
        kept.append((idx, int(start), int(end)))
    return dict(no_breath=audio, first=first, second=edges, kept=kept, db_margin=min(db_margin, m2), decision_margin=decision)


class StandIn(object):
    """Answers split_on_silence's device object (silence.SilenceDevice: upload, split, remove_breath, download) from the restatement."""

    def __init__(self, energy="spectral"):
        self.energy, self.calls = energy, []

    def upload(self, audio):
        return np.asarray(audio, np.float64).reshape(-1)

    def download(self, x):
        return x.astype(np.float32)

    def split(self, x, top_db, frame_length, hop_length):
        self.calls.append(("split", top_db, frame_length, hop_length))
        return split(x, top_db, frame_length, hop_length, self.energy)[0]

    def remove_breath(self, x, edges):
        self.calls.append(("remove_breath", len(edges)))
        new = np.zeros_like(x)
        for start, end in np.asarray(edges).reshape(-1, 2).tolist():
            new[start:end] = remove_breath(x[start:end], energy=self.energy)[0]
        return new

    def close(self):
        pass


def pieces(n, segments, seed, noise=1e-4):
    """The test signal: noise * randn over n samples, then level * randn on every [lo, hi) of segments = [(lo, hi, level)], drawn in
    that order from RandomState(seed).  float32 [n]."""
    rs = np.random.RandomState(seed)
    x = noise * rs.randn(n)
    for lo, hi, level in segments:
        x[lo:hi] = level * rs.randn(hi - lo)
    return x.astype(np.float32)
