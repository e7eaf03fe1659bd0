"""Splitting a long recording into utterances on the GPU: `split_on_silence_with_librosa` of the reference's audio/silence.py:33-76
without the file I/O -- the first stage of building a multi-speaker corpus from long recordings.  The reference splits the recording
with librosa.effects.split (top_db=40, frame_length=1024, hop_length=256), passes every interval through remove_breath (:21-31: a
second split at 128 / 32 and a mute of the quiet sub-intervals), writes the results into a zeroed copy of the recording, splits that
copy again and keeps the segments whose duration lies strictly between min_segment_length and max_segment_length seconds.

All arithmetic on samples is in libtaco_hip: taco_wav_split (both splits of the recording, and the 128 / 32 split of the intervals),
taco_collate (the intervals gathered into padded rectangles) and taco_wav_breath_mute.  The host sees the interval tables -- this is
corpus preparation, and it needs them to name the segments -- and the finished recording.  UNPINNED on librosa, as the trim is
(include/taco_abi.h): held by tests/split_reference.py, not by librosa.  The pydub method (:81-117) and decoding audio files stay
outside."""
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
