"""Splitting a long recording into utterances on the GPU: `split_on_silence_with_librosa` of the reference's audio/silence.py:33-76
without the file I/O -- the first stage of building a multi-speaker corpus from long recordings.  The reference splits the recording
with librosa.effects.split (top_db=40, frame_length=1024, hop_length=256), passes every interval through remove_breath (:21-31: a
second split at 128 / 32 and a mute of the quiet sub-intervals), writes the results into a zeroed copy of the recording, splits that
copy again and keeps the segments whose duration lies strictly between min_segment_length and max_segment_length seconds.

All arithmetic on samples is in libtaco_hip: taco_wav_split (both splits of the recording, and the 128 / 32 split of the intervals),
taco_collate (the intervals gathered into padded rectangles) and taco_wav_breath_mute.  The host sees the interval tables -- this is
corpus preparation, and it needs them to name the segments -- and the finished recording.  UNPINNED on librosa, as the trim is
(include/taco_abi.h): held by tests/split_reference.py, not by librosa.

The reference's other method, `split_on_silence_with_pydub` (:81-117, the one its README and scripts/prepare_*.sh run), is
split_on_silence_pydub below, and `amplify` of app.py:27-53, which shares its detection, is amplify: pydub.silence.detect_nonsilent on
16-bit PCM as taco_pcm_nonsilent restates it, the range sums by taco_pcm_range_sumsq and audioop.mul by taco_pcm_apply_gains; the host
walks the small table of ranges.  UNPINNED on pydub (include/taco_abi.h): held by tests/pydub_reference.py and the standard library's
audioop, not by pydub.  Decoding audio files and the mp3 export stay outside."""
import math

import numpy as np

from .feeder import collate_streams

RECT_WORDS = 1 << 26      # a rectangle of intervals holds at most this many samples (256 MB), however many rows chunk_rows allows


class SilenceDevice(object):
    """The device side of split_on_silence: a recording lives on the device as a [1, n] float32 tensor from `upload` to `download`.
    One instance serves any number of recordings (tools/split_on_silence.py); anything with these four methods can stand in for it."""

    def __init__(self, hparams, device="cuda:0", chunk_rows=32, griffin_lim=None):
        from .audio import GriffinLim
        self.gl = griffin_lim or GriffinLim(hparams, device)
        self._own = griffin_lim is None
        self.chunk_rows = max(1, int(chunk_rows))
        self.sample_rate = int(getattr(hparams, "sample_rate", 24000))
        self._resamplers = {}

    def resample(self, audio, orig_sr):
        """A recording at orig_sr -- 1-D, or [n, channels] interleaved; int16 is 16-bit PCM -- -> [1, n'] float32 on the device at
        hparams.sample_rate (audio.Resampler: librosa.core.load's resampling; channels are averaged)."""
        import torch
        from .audio import Resampler
        a = np.asarray(audio)
        a = np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32))
        if a.ndim > 2:
            raise Exception("a recording is [n] or [n, channels], got shape %s" % (a.shape,))
        rs = self._resamplers.get(int(orig_sr))
        if rs is None:
            rs = self._resamplers[int(orig_sr)] = Resampler(orig_sr, self.sample_rate, device=self.gl.device)
        return rs.resample(torch.as_tensor(a.reshape((1,) + a.shape)), channels=a.shape[1] if a.ndim == 2 else 1)[0]

    def upload(self, audio):
        import torch
        return torch.as_tensor(np.ascontiguousarray(np.asarray(audio, np.float32).reshape(1, -1))).to(self.gl.device)

    def download(self, x):
        return x[0].cpu().numpy()

    def split(self, x, top_db, frame_length, hop_length):
        """-> the recording's non-silent intervals, int64 [K, 2] on the host"""
        intervals, counts = self.gl.split(x, None, top_db=top_db, frame_length=frame_length, hop_length=hop_length)
        return intervals[0, :int(counts[0])].cpu().numpy().astype(np.int64)

    def chunks(self, edges):
        """Consecutive runs of at most chunk_rows intervals whose padded rectangle stays within RECT_WORDS samples (one interval always fits)."""
        k = 0
        while k < len(edges):
            rows, longest = 0, 1
            while k + rows < len(edges) and rows < self.chunk_rows:
                grown = max(longest, int(edges[k + rows][1] - edges[k + rows][0]))
                if rows and (rows + 1) * grown > RECT_WORDS:
                    break
                rows, longest = rows + 1, grown
            yield k, rows, longest
            k += rows

    def remove_breath(self, x, edges):
        """The reference's `new_audio`: zeros, and remove_breath(audio[start:end]) on every interval of edges (disjoint, in order)."""
        import torch
        dev = self.gl.device
        new = torch.zeros_like(x)
        for k, rows, longest in self.chunks(edges):
            e = np.asarray(edges[k:k + rows], np.int64)
            start = torch.as_tensor(np.ascontiguousarray(e[:, 0])).to(dev)
            length = torch.as_tensor((e[:, 1] - e[:, 0]).astype(np.int32)).to(dev)
            index = torch.arange(rows, dtype=torch.int32, device=dev)
            rect = torch.empty((rows, longest), dtype=torch.float32, device=dev)
            ns = torch.empty((rows,), dtype=torch.int32, device=dev)
            collate_streams(dev, [dict(pack=x, start=start, rows=length, width=1, rows_out=longest, out=rect, counts=ns)], index, rows, rows)
            out = self.gl.remove_breath(rect, ns)
            for j, (a, b) in enumerate(e.tolist()):
                new[0, a:b] = out[j, :b - a]
        return new

    def close(self):
        for rs in self._resamplers.values():
            rs.close()
        self._resamplers = {}
        if self._own:
            self.gl.close()


def split_on_silence(audio, hparams, top_db=40, frame_length=1024, hop_length=256, skip_idx=0, min_segment_length=3, max_segment_length=8,
                     pre_silence_length=0, post_silence_length=0, device="cuda:0", chunk_rows=32, orig_sr=None):
    """audio: one recording, 1-D float samples at hparams.sample_rate -- or, with orig_sr given, at orig_sr (1-D or [n, channels]; int16
    is 16-bit PCM): it is then resampled to hparams.sample_rate on the device before anything else (SilenceDevice.resample), and
    every sample index below counts at hparams.sample_rate.  -> (no_breath, segments): the recording after remove_breath on
    every interval [skip_idx:] of the first split and zeros elsewhere (what the reference saves as NAME.no_breath), float32; and a
    list of (idx, start, end, segment) for the intervals [skip_idx:] of the second split whose duration (end - start) / sample_rate
    lies strictly between min_segment_length and max_segment_length -- idx counts as the reference's `enumerate(edges[skip_idx:])`
    does (it is the number in the file name NAME.%04d), segment = no_breath[start:end] between sample_rate * pre_silence_length and
    sample_rate * post_silence_length zeros.  device: a device name, or a SilenceDevice to reuse (chunk_rows is then its own)."""
    sr = int(getattr(hparams, "sample_rate", 24000))
    dev = device if hasattr(device, "remove_breath") else SilenceDevice(hparams, device, chunk_rows)
    try:
        x = dev.upload(audio) if orig_sr is None else dev.resample(audio, orig_sr)
        edges = dev.split(x, top_db, frame_length, hop_length)
        y = dev.remove_breath(x, edges[skip_idx:])
        edges = dev.split(y, top_db, frame_length, hop_length)
        no_breath = np.asarray(dev.download(y), np.float32)
    finally:
        if dev is not device:
            dev.close()
    pre, post = np.zeros(int(sr * pre_silence_length), np.float32), np.zeros(int(sr * post_silence_length), np.float32)
    segments = []
    for idx, (start, end) in enumerate(np.asarray(edges).reshape(-1, 2)[skip_idx:].tolist()):
        duration = (end - start) / float(sr)
        if duration <= min_segment_length or duration >= max_segment_length:      # audio/silence.py:61: both bounds are excluded
            continue
        segments.append((idx, int(start), int(end), np.concatenate([pre, no_breath[start:end], post])))
    return no_breath, segments


class PcmDevice(object):
    """The device side of split_on_silence_pydub and amplify: a recording lives on the device as a [1, n, channels] int16 tensor from
    `upload` on, beside the per-millisecond energies its last `nonsilent` left.  One instance serves any number of recordings
    (tools/split_on_silence.py --method pydub); anything with these methods can stand in for it."""

    def __init__(self, hparams=None, device="cuda:0", griffin_lim=None):
        from .audio import GriffinLim
        from .hparams import hparams as default_hparams
        self.gl = griffin_lim or GriffinLim(hparams or default_hparams, device)
        self._own = griffin_lim is None

    def upload(self, pcm):
        """[n] or [n, channels] int16 -> the recording on the device"""
        import torch
        a = np.asarray(pcm)
        if a.dtype != np.int16 or a.ndim not in (1, 2):
            raise Exception("a recording is int16 PCM, [n] or [n, channels], got %s %s" % (a.dtype, a.shape))
        a = np.ascontiguousarray((a[:, None] if a.ndim == 1 else a)[None])
        return dict(pcm=torch.as_tensor(a).to(self.gl.device), energy=None)

    def nonsilent(self, x, sample_rate, min_silence_len, silence_thresh):
        """-> (the recording's non-silent ranges in milliseconds, int64 [K, 2] on the host, its length in milliseconds)"""
        if x["pcm"].shape[1] == 0:      # pydub: an empty segment is shorter than any window, [[0, 0]]
            return np.zeros((1, 2), np.int64), 0
        ranges, counts, len_ms, x["energy"] = self.gl.nonsilent(x["pcm"], None, sample_rate, min_silence_len, silence_thresh, return_energy=True)
        return ranges[0, :int(counts[0])].cpu().numpy().astype(np.int64), int(len_ms[0])

    def frames(self, x, start, end):
        """Frames [start, end) of the recording, zero frames at or past its end: int16 [end - start, channels] on the host"""
        n, ch = x["pcm"].shape[1], x["pcm"].shape[2]
        out = np.zeros((max(0, end - start), ch), np.int16)
        lo, hi = min(start, n), min(end, n)
        if hi > lo:
            out[:hi - lo] = x["pcm"][0, lo:hi].cpu().numpy()
        return out

    def range_sumsq(self, x, sample_rate, ranges):
        """-> ([S_k], [c_k]): every range's exact sum of squares and number of samples as Python integers (after `nonsilent` on x)"""
        r = np.asarray(ranges, np.int32).reshape(1, -1, 2)
        s, c = self.gl.range_sumsq(x["energy"], r, [r.shape[1]], x["pcm"].shape[1], x["pcm"].shape[2], None, sample_rate)
        return [int(v) for v in s[0].cpu().tolist()], [int(v) for v in c[0].cpu().tolist()]

    def apply_gains(self, x, sample_rate, ranges, gains):
        """-> the recording from its first range on, every range multiplied by its gain as audioop.mul does: int16 [m, channels] on the host"""
        r = np.asarray(ranges, np.int32).reshape(1, -1, 2)
        out, m = self.gl.apply_gains(x["pcm"], r, [r.shape[1]], np.asarray(gains, np.float64).reshape(1, -1), None, sample_rate)
        return out[0, :int(m[0])].cpu().numpy()

    def close(self):
        if self._own:
            self.gl.close()


def merge_ranges_pydub(ranges, min_silence_len=400, include_last_range=False):
    """The merge loop of audio/silence.py:94-103 on detect_nonsilent's ranges: a range that starts less than min_silence_len after the
    edge before it ends extends that edge.  As written there, `range(1, len(ranges) - 1)` never visits the LAST range, so the last
    utterance of every recording is dropped (a recording of one range keeps it: it is edges[0]); include_last_range=True visits it."""
    r = [[int(a), int(b)] for a, b in ranges]
    edges = [r[0]]      # IndexError for no range, as the reference's not_silence_ranges[0]
    for idx in range(1, len(r) if include_last_range else len(r) - 1):
        if r[idx][0] - edges[-1][1] < min_silence_len:
            edges[-1][1] = r[idx][1]
        else:
            edges.append(r[idx])
    return edges


def split_on_silence_pydub(pcm, sample_rate, skip_idx=0, silence_thresh=-40, min_silence_len=400, silence_chunk_len=100, keep_silence=100,
                           include_last_range=False, device="cuda:0"):
    """split_on_silence_with_pydub of audio/silence.py:81-117 without the file I/O.  pcm: one recording, int16, [n] or [n, channels]
    interleaved, at sample_rate.  detect_nonsilent(min_silence_len=silence_chunk_len, silence_thresh) on the device, then on the
    host: merge_ranges_pydub (the reference drops the last range; include_last_range=True keeps it), and for every edge [skip_idx:]
    start = max(0, start - keep_silence), end = end + keep_silence, both clamped to the recording's length in milliseconds, as a
    pydub slice clamps them.  -> [(idx, start_ms, end_ms, segment)]: idx counts as the reference's `enumerate(edges[skip_idx:])` does
    (the number in the file name NAME.%04d), segment = the frames [p(start_ms), p(end_ms)) with p(j) = j * sample_rate // 1000, zero
    frames at or past n, int16 shaped as pcm.  A recording without a non-silent range (all silent) raises, as the reference's
    not_silence_ranges[0] does.  device: a device name, or a PcmDevice (or a stand-in) to reuse."""
    from .audio import pcm_frame_of_ms
    sr = int(sample_rate)
    mono = np.asarray(pcm).ndim == 1
    dev = device if hasattr(device, "nonsilent") else PcmDevice(device=device)
    try:
        x = dev.upload(pcm)
        ranges, M = dev.nonsilent(x, sr, silence_chunk_len, silence_thresh)
        if len(ranges) == 0:
            raise Exception("no non-silent range: the recording is silent at %s dBFS throughout" % (silence_thresh,))
        edges = merge_ranges_pydub(ranges, min_silence_len, include_last_range)
        segments = []
        for idx, (start, end) in enumerate(edges[skip_idx:]):
            start, end = min(max(0, start - keep_silence), M), min(end + keep_silence, M)
            seg = dev.frames(x, pcm_frame_of_ms(start, sr), pcm_frame_of_ms(end, sr))
            segments.append((idx, int(start), int(end), seg[:, 0] if mono else seg))
    finally:
        if dev is not device:
            dev.close()
    return segments


def amplify_gain(sumsq, samples, target_dbfs=-20.0):
    """match_target_amplitude of app.py:27-29 for one stretch, from its exact sum of squares and number of samples, in double on the host
    as pydub forms it: rms = (unsigned)sqrt(S / c) (audioop.rms), dBFS = 20 log10(rms / 32768), factor = 10^((target - dBFS) / 20).
    (pydub's published ratio_to_db writes log(ratio, 10), which may part from log10 by an ulp; this follows log10.)  A stretch whose rms
    is 0 -- S = 0, or no sample -- gets 1.0, a copy: the reference would multiply it by infinity."""
    rms = int(math.sqrt(sumsq / float(samples))) if samples else 0
    if rms == 0:
        return 1.0
    return 10 ** ((float(target_dbfs) - 20 * math.log10(rms / 32768.0)) / 20)


def amplify(pcm, sample_rate, target_dbfs=-20.0, silence_thresh=-50, min_silence_len=300, device="cuda:0"):
    """amplify of app.py:27-53 without the file I/O and the mp3 export: detect_nonsilent(silence_thresh, min_silence_len), the last
    range's end moved to the end of the recording, every range brought to target_dbfs by its own factor (amplify_gain; audioop.mul:
    clip(floor(x * factor))), what lies between two ranges unchanged, what precedes the first dropped, as the reference drops it.
    pcm: int16, [n] or [n, channels] -> int16 shaped alike, the frames [p(start_0), p(M)) with M the length in milliseconds; no range
    (a silent recording) gives an empty result."""
    sr = int(sample_rate)
    a = np.asarray(pcm)
    dev = device if hasattr(device, "nonsilent") else PcmDevice(device=device)
    try:
        x = dev.upload(a)
        ranges, M = dev.nonsilent(x, sr, min_silence_len, silence_thresh)
        if len(ranges) == 0 or M == 0:      # (M == 0: the frames [p(0), p(0)))
            return np.zeros((0,) + a.shape[1:], np.int16)
        ranges = [[int(s), int(e)] for s, e in ranges]
        ranges[-1][1] = M
        sumsq, samples = dev.range_sumsq(x, sr, ranges)
        out = dev.apply_gains(x, sr, ranges, [amplify_gain(s, c, target_dbfs) for s, c in zip(sumsq, samples)])
    finally:
        if dev is not device:
            dev.close()
    return out[:, 0] if a.ndim == 1 else out
