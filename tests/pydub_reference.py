"""Restatement of `pydub.silence.detect_silence` / `detect_nonsilent` (seek_step = 1) and of the two places the reference calls them:
`split_on_silence_with_pydub` (audio/silence.py:81-117) and `amplify` (app.py:27-53), without their file I/O -- test infrastructure only:
nothing in the product imports it.

UNPINNED on pydub.  The reference pins pydub==0.20.0; pydub is not a dependency of this project and is not available to its tests, so
this file restates pydub's published silence.py and the parts of AudioSegment it leans on (len() in milliseconds, slicing by
milliseconds with missing frames padded by silence, rms, dBFS, apply_gain) and could NOT be checked against pydub's source or output.
What it CAN lean on is the standard library's audioop, which is what pydub calls for every number: rms and mul.

Written twice:
  LITERAL  pydub's loops, as pydub runs them: a `Segment` of bytes, one slice and one audioop.rms per window start, the list of silent
           starts walked with `continuous` / `silence_has_gap`; audioop.mul per range.  Needs audioop (gone from the standard library
           in Python 3.13: HAVE_AUDIOOP is then False and the tests that need it skip).
  FAST     NumPy int64 prefix sums over the squared samples and the integer comparison S < (k + 1)^2 * c the kernels use
           (include/taco_abi.h), the same walk over the silent starts; floor / clip in float64 for the gain.
tests/test_pydub_host.py holds the two equal; the GPU tests compare the device with FAST (and with audioop directly)."""
import math

import numpy as np

try:
    import audioop
    HAVE_AUDIOOP = True
except ImportError:      # Python >= 3.13
    audioop = None
    HAVE_AUDIOOP = False


# ---- what both forms share: the millisecond grid ----
def frame_of_ms_pydub(j, sr):
    """AudioSegment._parse_position / frame_count(ms=j): int(j * (frame_rate / 1000.0)), in double"""
    return int(j * (sr / 1000.0))


def frame_of_ms(j, sr):
    """The integer form the kernels use: floor(j * sr / 1000)"""
    return int(j) * int(sr) // 1000


def len_ms(n, sr):
    """len(AudioSegment): round(1000 * (frame_count / frame_rate)), Python's round"""
    return int(round(1000 * (float(n) / sr)))


def threshold(silence_thresh):
    """db_to_float(silence_thresh) * max_possible_amplitude, in double"""
    return 10 ** (float(silence_thresh) / 20) * 32768.0


def as_frames(pcm):
    a = np.asarray(pcm)
    assert a.dtype == np.int16 and a.ndim in (1, 2)
    return np.ascontiguousarray(a[:, None] if a.ndim == 1 else a)


# ---- LITERAL ----
class Segment(object):
    """As much of pydub.AudioSegment as silence.py and app.py use, on interleaved 16-bit frames held as bytes."""

    def __init__(self, data, sr, channels):
        self.data, self.sr, self.channels, self.frame_width = bytes(data), int(sr), int(channels), 2 * int(channels)

    @classmethod
    def of(cls, pcm, sr):
        a = as_frames(pcm)
        return cls(a.astype("<i2").tobytes(), sr, a.shape[1])

    def frame_count(self):
        return len(self.data) // self.frame_width

    def __len__(self):
        return len_ms(self.frame_count(), self.sr)

    def slice(self, start, end):
        """AudioSegment.__getitem__(slice(start, end)) in milliseconds: None is an open end, both ends are clamped to len(self),
        and frames the data does not have are padded with silence."""
        start = 0 if start is None else min(start, len(self))
        end = len(self) if end is None else min(end, len(self))
        a, b = frame_of_ms_pydub(start, self.sr) * self.frame_width, frame_of_ms_pydub(end, self.sr) * self.frame_width
        data = self.data[a:b]
        missing = ((b - a) - len(data)) // self.frame_width      # "ensure the output is as long as the requester is expecting"
        if missing > 0:
            data += b"\0" * (missing * self.frame_width)
        return Segment(data, self.sr, self.channels)

    @property
    def rms(self):
        return audioop.rms(self.data, 2)

    @property
    def dBFS(self):
        ratio = self.rms / 32768.0
        return -float("inf") if ratio == 0 else 20 * math.log10(ratio)

    def apply_gain(self, change):
        return Segment(audioop.mul(self.data, 2, 10 ** (float(change) / 20)), self.sr, self.channels)

    def append(self, other):
        return Segment(self.data + other.data, self.sr, self.channels)

    def frames(self):
        return np.frombuffer(self.data, "<i2").reshape(-1, self.channels).astype(np.int16)


def ranges_from_starts(silence_starts, seg_len, min_silence_len):
    """detect_silence's walk over the sorted silent starts (seek_step = 1), then nothing else: the silent ranges"""
    if not silence_starts:
        return []
    silence_starts = list(silence_starts)
    silent_ranges = []
    prev_i = silence_starts.pop(0)
    current_range_start = prev_i
    for silence_start_i in silence_starts:
        continuous = silence_start_i == prev_i + 1
        silence_has_gap = silence_start_i > prev_i + min_silence_len
        if not continuous and silence_has_gap:
            silent_ranges.append([current_range_start, prev_i + min_silence_len])
            current_range_start = silence_start_i
        prev_i = silence_start_i
    silent_ranges.append([current_range_start, prev_i + min_silence_len])
    return silent_ranges


def invert(silent_ranges, len_seg):
    """detect_nonsilent after its call of detect_silence"""
    if not silent_ranges:
        return [[0, len_seg]]
    if silent_ranges[0][0] == 0 and silent_ranges[0][1] == len_seg:
        return []
    prev_end_i = 0
    nonsilent_ranges = []
    for start_i, end_i in silent_ranges:
        nonsilent_ranges.append([prev_end_i, start_i])
        prev_end_i = end_i
    if end_i != len_seg:
        nonsilent_ranges.append([prev_end_i, len_seg])
    if nonsilent_ranges[0] == [0, 0]:
        nonsilent_ranges.pop(0)
    return nonsilent_ranges


def detect_silence_literal(seg, min_silence_len=1000, silence_thresh=-16):
    seg_len = len(seg)
    if seg_len < min_silence_len:
        return []
    thresh = threshold(silence_thresh)
    silence_starts = []
    for i in range(0, seg_len - min_silence_len + 1):
        if seg.slice(i, i + min_silence_len).rms <= thresh:
            silence_starts.append(i)
    return ranges_from_starts(silence_starts, seg_len, min_silence_len)


def detect_nonsilent_literal(seg, min_silence_len=1000, silence_thresh=-16):
    return invert(detect_silence_literal(seg, min_silence_len, silence_thresh), len(seg))


def amplify_literal(pcm, sr, target_dbfs=-20.0, silence_thresh=-50, min_silence_len=300, zero_rms_is_copy=True):
    """app.py:27-53 up to the export, on the literal Segment.  zero_rms_is_copy: the one departure (include/taco_abi.h): a stretch whose
    rms is 0 is appended unchanged where the reference would multiply it by infinity.  -> int16 [m, channels]"""
    sound = Segment.of(pcm, sr)
    nonsilent_ranges = detect_nonsilent_literal(sound, min_silence_len, silence_thresh)
    new_sound = None
    for idx, (start_i, end_i) in enumerate(nonsilent_ranges):
        if idx == len(nonsilent_ranges) - 1:
            end_i = None
        piece = sound.slice(start_i, end_i)
        amplified = piece if (zero_rms_is_copy and piece.rms == 0) else piece.apply_gain(target_dbfs - piece.dBFS)
        new_sound = amplified if idx == 0 else new_sound.append(amplified)
        if idx < len(nonsilent_ranges) - 1:
            new_sound = new_sound.append(sound.slice(end_i, nonsilent_ranges[idx + 1][0]))
    return np.zeros((0, sound.channels), np.int16) if new_sound is None else new_sound.frames()


# ---- FAST ----
def prefix_squares(pcm, sr):
    """(cs, n, C, M): cs[f] = the sum of squares of frames [0, f) over all channels, int64, continued flat over the zero frames up to p(M)"""
    a = as_frames(pcm).astype(np.int64)
    n, C = a.shape
    M = len_ms(n, sr)
    top = max(n, frame_of_ms(M, sr))
    cs = np.zeros(top + 1, np.int64)
    np.cumsum((a * a).sum(axis=1), out=cs[1:n + 1])
    cs[n + 1:] = cs[n]
    return cs, n, C, M


def window_sumsq(pcm, sr, min_silence_len):
    """-> (S int64 [max(0, M - W + 1)], c int64 alike, M)"""
    cs, n, C, M = prefix_squares(pcm, sr)
    W = int(min_silence_len)
    if M < W:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), M
    i = np.arange(0, M - W + 1, dtype=np.int64)
    lo, hi = i * sr // 1000, (i + W) * sr // 1000
    return cs[hi] - cs[lo], (hi - lo) * C, M


def silent_flags(pcm, sr, min_silence_len, silence_thresh):
    S, c, M = window_sumsq(pcm, sr, min_silence_len)
    k = int(math.floor(threshold(silence_thresh)))
    return (c == 0) | (S < (k + 1) ** 2 * c), M


def detect_nonsilent(pcm, sr, min_silence_len=1000, silence_thresh=-16):
    """-> (non-silent ranges [[start_ms, end_ms]], M)"""
    flags, M = silent_flags(pcm, sr, min_silence_len, silence_thresh)
    return invert(ranges_from_starts(np.flatnonzero(flags).tolist(), M, min_silence_len), M), M


def frames_of(pcm, a, b):
    """Frames [a, b), zero frames at or past the recording's end: int16 [b - a, channels]"""
    x = as_frames(pcm)
    out = np.zeros((max(0, b - a), x.shape[1]), np.int16)
    lo, hi = min(a, len(x)), min(b, len(x))
    out[:hi - lo] = x[lo:hi]
    return out


def range_sumsq(pcm, sr, ranges):
    cs, n, C, M = prefix_squares(pcm, sr)
    S = [int(cs[frame_of_ms(e, sr)] - cs[frame_of_ms(s, sr)]) for s, e in ranges]
    return S, [(frame_of_ms(e, sr) - frame_of_ms(s, sr)) * C for s, e in ranges]


def mul(x, factor):
    """audioop.mul on int16 samples: clip(floor((double)x * factor))"""
    return np.clip(np.floor(np.asarray(x, np.float64) * float(factor)), -32768, 32767).astype(np.int16)


def gain(S, c, target_dbfs=-20.0):
    rms = int(math.sqrt(S / float(c))) if c else 0
    return 1.0 if rms == 0 else 10 ** ((float(target_dbfs) - 20 * math.log10(rms / 32768.0)) / 20)


def apply_gains(pcm, sr, ranges, gains):
    """The frames [p(s_0), p(M)), every range multiplied by its gain, the gaps copied: int16 [m, channels]"""
    M = len_ms(len(as_frames(pcm)), sr)
    if not len(ranges):
        return np.zeros((0, as_frames(pcm).shape[1]), np.int16)
    first = frame_of_ms(ranges[0][0], sr)
    out = frames_of(pcm, first, frame_of_ms(M, sr))
    for (s, e), g in zip(ranges, gains):
        a, b = frame_of_ms(s, sr) - first, frame_of_ms(e, sr) - first
        out[a:b] = mul(out[a:b], g)
    return out


def amplify(pcm, sr, target_dbfs=-20.0, silence_thresh=-50, min_silence_len=300):
    ranges, M = detect_nonsilent(pcm, sr, min_silence_len, silence_thresh)
    if not ranges:
        return np.zeros((0, as_frames(pcm).shape[1]), np.int16)
    ranges[-1][1] = M
    S, c = range_sumsq(pcm, sr, ranges)
    return apply_gains(pcm, sr, ranges, [gain(s, k, target_dbfs) for s, k in zip(S, c)])


def split_on_silence_with_pydub(pcm, sr, skip_idx=0, silence_thresh=-40, min_silence_len=400, silence_chunk_len=100, keep_silence=100,
                                include_last_range=False, literal=False):
    """audio/silence.py:81-117 without read_audio / export.  -> [(idx, start_ms, end_ms, frames int16 [m, channels])]; the slice is
    AudioSegment's (both ends clamped to the length, missing frames zero).  include_last_range=True lets the merge loop visit the
    last range, which the reference's `range(1, len(not_silence_ranges) - 1)` never does."""
    if literal:
        not_silence_ranges = detect_nonsilent_literal(Segment.of(pcm, sr), silence_chunk_len, silence_thresh)
    else:
        not_silence_ranges = detect_nonsilent(pcm, sr, silence_chunk_len, silence_thresh)[0]
    M = len_ms(len(as_frames(pcm)), sr)
    edges = [not_silence_ranges[0]]
    for idx in range(1, len(not_silence_ranges) - (0 if include_last_range else 1)):
        cur_start = not_silence_ranges[idx][0]
        prev_end = edges[-1][1]
        if cur_start - prev_end < min_silence_len:
            edges[-1][1] = not_silence_ranges[idx][1]
        else:
            edges.append(not_silence_ranges[idx])
    out = []
    for idx, (start_idx, end_idx) in enumerate(edges[skip_idx:]):
        start_idx = max(0, start_idx - keep_silence)
        end_idx += keep_silence
        start_idx, end_idx = min(start_idx, M), min(end_idx, M)
        out.append((idx, start_idx, end_idx, frames_of(pcm, frame_of_ms(start_idx, sr), frame_of_ms(end_idx, sr))))
    return out


class StandIn(object):
    """Answers silence.PcmDevice's methods (upload, nonsilent, frames, range_sumsq, apply_gains, close) from the FAST form."""

    def __init__(self):
        self.calls = []

    def upload(self, pcm):
        return as_frames(pcm)

    def nonsilent(self, x, sample_rate, min_silence_len, silence_thresh):
        self.calls.append(("nonsilent", sample_rate, min_silence_len, silence_thresh))
        ranges, M = detect_nonsilent(x, sample_rate, min_silence_len, silence_thresh)
        return np.asarray(ranges, np.int64).reshape(-1, 2), M

    def frames(self, x, start, end):
        return frames_of(x, start, end)

    def range_sumsq(self, x, sample_rate, ranges):
        self.calls.append(("range_sumsq", len(ranges)))
        return range_sumsq(x, sample_rate, ranges)

    def apply_gains(self, x, sample_rate, ranges, gains):
        self.calls.append(("apply_gains", len(ranges)))
        return apply_gains(x, sample_rate, ranges, gains)

    def close(self):
        pass


# ---- test signals ----
def bursts(n, channels, segments, seed, noise=2):
    """int16 [n, channels]: uniform noise in [-noise, noise], then on every [lo, hi) of segments = [(lo, hi, amplitude)] uniform values in
    [-amplitude, amplitude], drawn in that order from RandomState(seed)"""
    rs = np.random.RandomState(seed)
    x = rs.randint(-noise, noise + 1, size=(n, channels))
    for lo, hi, amp in segments:
        x[lo:hi] = rs.randint(-amp, amp + 1, size=(hi - lo, channels))
    return x.astype(np.int16)


def render(pattern, sr, channels, levels=(0, 3000, 500)):
    """One millisecond of constant amplitude levels[v] per entry v of a pattern (0: quiet, 1: loud, 2: medium): int16 [p(len(pattern)), channels]"""
    n = frame_of_ms(len(pattern), sr)
    x = np.zeros((n, channels), np.int16)
    for j, v in enumerate(pattern):
        x[frame_of_ms(j, sr):frame_of_ms(j + 1, sr)] = levels[v]
    return x


# Every branch of detect_silence / detect_nonsilent on one millisecond of constant amplitude per entry (render), at 8 kHz and W = 4
PATTERN_SR, PATTERN_W = 8000, 4
PATTERNS = {      # 1: a loud millisecond.  name: (pattern, non-silent ranges at W = 4)
    "no silence": ([1] * 12, [[0, 12]]),
    "all silent": ([0] * 12, []),
    "silence at the head": ([0] * 6 + [1] * 6, [[6, 12]]),                  # the [0, 0] range is removed
    "silence at the tail": ([1] * 6 + [0] * 6, [[0, 6]]),
    "silence in the middle": ([1] * 4 + [0] * 5 + [1] * 4, [[0, 4], [9, 13]]),
    "a silence shorter than W": ([1] * 4 + [0] * 3 + [1] * 4, [[0, 11]]),
    # 2: a millisecond at 500 -- one of them in a window of four leaves it silent (rms 250 <= 327), two do not (rms 353)
    "two silent runs closer than W": ([0, 0, 0, 2, 0, 2, 0, 0, 0, 1, 1, 1], [[9, 12]]),           # starts {0, 1} and {4, 5}: 4 <= 1 + 4, ONE range [0, 9]
    "two silent runs just past W apart": ([0] * 4 + [1] + [0] * 4 + [1] * 3, [[4, 5], [9, 12]]),  # starts 0 and 5: 5 > 0 + 4, two ranges
    "two silent runs W + 1 apart": ([0] * 4 + [1] * 2 + [0] * 4 + [1] * 3, [[4, 6], [10, 13]]),     # starts 0 and 6: 6 > 0 + 4
    "M < W": ([0] * 3, [[0, 3]]),
    "M == W, silent": ([0] * 4, []),
    "M == W, loud": ([0, 0, 1, 0], [[0, 4]]),
    "an isolated silent window": ([1] * 3 + [0] * 4 + [1] * 3, [[0, 3], [7, 10]]),
}


def speech(sr=8000, channels=1):
    """Four utterances: 40-300, 420-700 (120 ms after the first), 1300-1500, 2150-2290 ms of 2400 ms"""
    ms = lambda a: a * sr // 1000
    return bursts(ms(2400), channels, [(ms(40), ms(300), 8000), (ms(420), ms(700), 6000), (ms(1300), ms(1500), 9000), (ms(2150), ms(2290), 7000)], seed=11, noise=3)
