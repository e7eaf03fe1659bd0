"""Host side of splitting on silence (taco_wav_split, taco_wav_breath_mute, silence.split_on_silence): everything that needs no GPU --
the restatement tests/split_reference.py on hand-written frame patterns, the identity that ties the split to the trim, the argument
errors of both entry points through the library, and split_on_silence's own logic (strict duration bounds, the numbering of the
segments, the silence padding) over a stand-in for the device that answers from the restatement."""
import ctypes as C

import numpy as np
import pytest

import split_reference as R
import trim_reference as T
from taco_amd import _lib, silence


def test_restatement_on_hand_written_patterns():
    f = lambda pattern, n, hop: R.runs_of(np.array(pattern, bool), n, hop).tolist()
    assert f([1, 1, 0, 0, 1, 0], 50, 10) == [[0, 20], [40, 50]]               # a run at frame 0: the prepended 0
    assert f([0, 0, 1, 1], 35, 10) == [[20, 35]]                              # a run at the last frame: len(non_silent) appended, min(n, .)
    assert f([0, 0, 0, 0], 35, 10) == []
    assert f([0, 0, 1, 0], 35, 10) == [[20, 30]]                              # all silent below one loud frame
    assert f([1, 1, 1, 1], 35, 10) == [[0, 35]]                               # all non-silent
    assert f([0, 0, 0, 1], 30, 10) == [[30, 30]]                              # n % hop == 0, the last frame alone: the empty interval
    assert f([1, 0, 1, 0, 1], 40, 10) == [[0, 10], [20, 30], [40, 40]]
    assert f([1], 1, 10) == [[0, 1]] and f([], 0, 10) == []
    assert R.split(np.zeros(1), 40, 16, 2)[0].shape == (0, 2)                # fewer than two samples: no frames, no intervals
    iv, db, margin = R.split(np.zeros(40), 40, 16, 4)                         # an all-zero row: every frame clamps to 1e-10, 0 dB
    assert iv.tolist() == [[0, 40]] and np.all(db == 0.0)


@pytest.mark.parametrize("energy", R.ENERGIES)
@pytest.mark.parametrize("N,hop", [(16, 2), (64, 8), (16, 16)])
def test_the_outer_ends_of_the_split_are_the_trim_index(N, hop, energy):
    lengths = [700, 451, 64, 33, 9, 2]
    x = T.burst_rows(700, lengths, [(0.3, 0.7), (0.5, 1.0), (0.4, 1.0), (0.2, 0.6), (0.3, 0.8), (0.0, 1.0)], 0)
    x[0, :60] = R.pieces(60, [(0, 60, 0.3)], 1)                               # more than one run on the long row
    for b, n in enumerate(lengths):
        iv = R.split(x[b, :n], 40, N, hop, energy)[0]
        index = T.trim(x[b, :n], 40, N, hop, energy)[0]
        assert len(iv) >= 1 and [iv[0][0], iv[-1][1]] == index.tolist(), (b, iv.tolist(), index.tolist())
    assert len(R.split(x[0], 40, N, hop, energy)[0]) >= 2
    quiet = np.zeros(64)
    quiet[58:] = 0.3 * np.random.RandomState(0).randn(6)
    if (N, hop) == (16, 16):
        assert R.split(quiet, 40, N, hop, energy)[0].tolist() == [[64, 64]] and T.trim(quiet, 40, N, hop, energy)[0].tolist() == [64, 64]


def test_remove_breath_restatement_mutes_in_place():
    x = R.pieces(2000, [(0, 500, 0.45), (700, 1200, 0.06), (1400, 1900, 0.085)], 0)
    y, info = R.remove_breath(x)
    assert info["muted"].tolist() == [False, True, False] and R.remove_breath(x, frozen_mean=True)[1]["muted"].tolist() == [False, True, True]
    (a, b), (c, d) = info["intervals"][1], info["intervals"][2]
    assert not y[a:b].any() and np.array_equal(y[c:d], x[c:d].astype(np.float64)) and np.array_equal(y[:a], x[:a].astype(np.float64))
    assert np.isnan(R.abs_mean(np.zeros(0))) and info["abs_mean"][0] == np.abs(x.astype(np.float64)).mean()


def test_library_exports_the_split_entry_points():
    lib = _lib.load_library()
    for name in ("taco_wav_split", "taco_wav_split_workspace_bytes", "taco_wav_breath_mute"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    assert int(lib.taco_wav_split_workspace_bytes(3, 1000, 64, 8)) == int(lib.taco_wav_trim_workspace_bytes(3, 1000, 64, 8)) > 0


def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory: validation rejects every one of these calls before it is touched."""
    lib = _lib.load_library()
    d = C.c_void_p(4096)
    big = 1 << 20

    def split(wav=d, ns=None, B=2, L=1000, top_db=40.0, N=64, hop=8, energy=_lib.TACO_TRIM_SPECTRAL, M=4, intervals=d, counts=d, db=None, ws=d, ws_bytes=big):
        return lib.taco_wav_split(None, wav, ns, B, L, top_db, N, hop, energy, M, intervals, counts, db, ws, ws_bytes)

    assert split(hop=0) == _lib.TACO_ERR_ARG and split(hop=-3) == _lib.TACO_ERR_ARG
    assert split(N=1) == _lib.TACO_ERR_ARG and split(N=0) == _lib.TACO_ERR_ARG
    assert split(M=0) == _lib.TACO_ERR_ARG and split(M=-1) == _lib.TACO_ERR_ARG
    assert b"max_intervals" in lib.taco_last_error()
    assert split(energy=2) == _lib.TACO_ERR_ARG and split(energy=-1) == _lib.TACO_ERR_ARG
    assert split(wav=None) == _lib.TACO_ERR_ARG and split(intervals=None) == _lib.TACO_ERR_ARG and split(counts=None) == _lib.TACO_ERR_ARG
    assert split(ws=None) == _lib.TACO_ERR_ARG
    assert split(B=0) == _lib.TACO_ERR_ARG and split(L=0) == _lib.TACO_ERR_ARG
    need = int(lib.taco_wav_split_workspace_bytes(2, 1000, 64, 8))
    assert split(ws_bytes=need - 1) == _lib.TACO_ERR_ARG and split(ws_bytes=0) == _lib.TACO_ERR_ARG
    assert b"workspace" in lib.taco_last_error()
    assert split(N=65) == _lib.TACO_ERR_UNSUPPORTED and split(N=8194, hop=256) == _lib.TACO_ERR_UNSUPPORTED      # as the trim
    assert split(N=16386, hop=256, energy=_lib.TACO_TRIM_TIME) == _lib.TACO_ERR_UNSUPPORTED

    def mute(wav=d, ns=None, S=2, L=1000, intervals=d, counts=d, M=4, threshold=0.05, out=d, muted=None, mean=None):
        return lib.taco_wav_breath_mute(None, wav, ns, S, L, intervals, counts, M, threshold, out, muted, mean)

    assert mute(wav=None) == _lib.TACO_ERR_ARG and mute(intervals=None) == _lib.TACO_ERR_ARG
    assert mute(counts=None) == _lib.TACO_ERR_ARG and mute(out=None) == _lib.TACO_ERR_ARG
    assert mute(S=0) == _lib.TACO_ERR_ARG and mute(L=0) == _lib.TACO_ERR_ARG
    assert mute(M=0) == _lib.TACO_ERR_ARG
    assert b"max_intervals" in lib.taco_last_error()


class _HP(object):
    sample_rate = 100


class _Scripted(R.StandIn):
    """The restatement's stand-in with the SECOND split's answer written by hand, so that durations fall exactly on the bounds."""

    def __init__(self, second):
        super(_Scripted, self).__init__()
        self.second = np.array(second, np.int64)

    def split(self, x, top_db, frame_length, hop_length):
        first = super(_Scripted, self).split(x, top_db, frame_length, hop_length)
        return first if sum(c[0] == "split" for c in self.calls) == 1 else self.second


def test_duration_bounds_are_strict_and_idx_counts_from_skip_idx():
    """At 100 Hz with bounds 3 s and 8 s: 300 and 800 samples are excluded, 301 and 799 kept (audio/silence.py:61); idx is the position
    in edges[skip_idx:], and the segment carries sample_rate * pre / post zeros."""
    x = np.arange(1, 4001, dtype=np.float32) / 4000.0
    second = [[0, 100], [100, 400], [400, 701], [1000, 1800], [1800, 2599], [2600, 2900], [3000, 3301]]
    dev = _Scripted(second)
    no_breath, seg = silence.split_on_silence(x, _HP(), top_db=40, frame_length=64, hop_length=8, device=dev)
    assert [s[:3] for s in seg] == [(2, 400, 701), (4, 1800, 2599), (6, 3000, 3301)]
    assert [c[0] for c in dev.calls] == ["split", "remove_breath", "split"] and dev.calls[0] == ("split", 40, 64, 8)
    assert no_breath.dtype == np.float32 and all(np.array_equal(s[3], no_breath[s[1]:s[2]]) for s in seg)
    dev = _Scripted(second)
    no_breath, seg = silence.split_on_silence(x, _HP(), top_db=40, frame_length=64, hop_length=8, skip_idx=2, pre_silence_length=1, post_silence_length=2, device=dev)
    assert [s[:3] for s in seg] == [(0, 400, 701), (2, 1800, 2599), (4, 3000, 3301)]
    assert dev.calls[1] == ("remove_breath", max(0, len(R.split(x, 40, 64, 8)[0]) - 2))
    for idx, start, end, s in seg:
        assert len(s) == 100 + (end - start) + 200 and not s[:100].any() and not s[-200:].any() and np.array_equal(s[100:-200], no_breath[start:end])


def test_split_on_silence_host_logic_equals_the_restatement():
    """The recording of tests/test_gpu_split.py's end-to-end case, with the restatement standing in for the device."""
    segs = [(100, 500, 0.3), (640, 760, 0.001), (760, 960, 0.03), (960, 1080, 0.001), (1080, 1400, 0.3), (1700, 1900, 0.3), (2200, 2700, 0.25),
            (2700, 2800, 0.001), (2800, 3000, 0.25), (3300, 3600, 0.3), (3900, 4500, 0.3)]
    x = R.pieces(4800, segs, 4, noise=1e-5)
    kw = dict(top_db=60, frame_length=64, hop_length=8, min_segment_length=0.2, max_segment_length=0.5)

    class HP(object):
        sample_rate = 1600
    for skip in (0, 1):
        ref = R.split_on_silence(x, 1600, skip_idx=skip, **kw)
        no_breath, seg = silence.split_on_silence(x, HP(), skip_idx=skip, device=R.StandIn(), **kw)
        assert np.array_equal(no_breath, ref["no_breath"].astype(np.float32)) and [s[:3] for s in seg] == ref["kept"]
    assert [k[0] for k in R.split_on_silence(x, 1600, **kw)["kept"]] == [0, 2, 5, 6]
    assert (R.split_on_silence(x, 1600, **kw)["no_breath"] != x.astype(np.float64)).any()


def test_chunks_respect_the_row_and_the_size_limit():
    dev = silence.SilenceDevice.__new__(silence.SilenceDevice)
    dev.chunk_rows = 3
    edges = np.array([[0, 10], [20, 50], [60, 61], [70, 70], [80, 200]])
    assert list(dev.chunks(edges)) == [(0, 3, 30), (3, 2, 120)]
    assert list(dev.chunks(edges[:0])) == []
    big = np.array([[0, silence.RECT_WORDS], [0, 5], [0, silence.RECT_WORDS // 2 + 1], [0, silence.RECT_WORDS // 2 + 1]])
    assert [c[:2] for c in dev.chunks(big)] == [(0, 1), (1, 1), (2, 1), (3, 1)]
