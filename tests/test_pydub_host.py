"""Host side of the pydub method (taco_pcm_nonsilent, taco_pcm_range_sumsq, taco_pcm_apply_gains, silence.split_on_silence_pydub,
silence.amplify): everything that needs no GPU -- the restatement tests/pydub_reference.py in its two forms against each other and
against the standard library's audioop, the millisecond grid against pydub's double expression, every branch of detect_silence and
detect_nonsilent on hand-written patterns, the reference's merge loop with its dropped last range, amplify's cut, the argument
errors of the four entry points through the library, and the host logic of both functions over a stand-in for the device."""
import ctypes as C
import math

import numpy as np
import pytest

import pydub_reference as R
from taco_amd import _lib, audio, silence

needs_audioop = pytest.mark.skipif(not R.HAVE_AUDIOOP, reason="audioop left the standard library in Python 3.13")
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)


def test_library_exports_the_pcm_entry_points():
    lib = _lib.load_library()
    for name in ("taco_pcm_rate_supported", "taco_pcm_nonsilent_workspace_bytes", "taco_pcm_nonsilent", "taco_pcm_range_sumsq", "taco_pcm_apply_gains",
                 "taco_debug_pcm_energy"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
    M = R.len_ms(1000, 8000)
    assert int(lib.taco_pcm_nonsilent_workspace_bytes(3, 1000, 8000)) >= 3 * M * 9
    assert int(lib.taco_pcm_nonsilent_workspace_bytes(0, 1000, 8000)) == 0 and int(lib.taco_pcm_nonsilent_workspace_bytes(3, 1000, 0)) == 0


@pytest.mark.parametrize("sr", RATES)
def test_millisecond_grid_equals_pydubs_double_expression_out_to_one_hour(sr):
    """p(j) = floor(j*sr/1000) against int(j * (sr/1000.0)), evaluated in float64 as Python evaluates it, at every millisecond of an hour"""
    j = np.arange(0, 3600001, dtype=np.int64)
    assert np.array_equal(j * sr // 1000, (j.astype(np.float64) * (sr / 1000.0)).astype(np.int64))
    for jj in (0, 1, 999, 1000, 3599999, 3600000):
        assert R.frame_of_ms(jj, sr) == R.frame_of_ms_pydub(jj, sr) == audio.pcm_frame_of_ms(jj, sr)


def test_the_rates_the_entry_point_accepts_are_the_ones_whose_grid_is_pydubs():
    """The library takes a rate iff fl(sr/1000.0) >= sr/1000 (include/taco_abi.h; taco_pcm_rate_supported, host arithmetic): at such a
    rate the two expressions agree at every millisecond (checked here for an hour and at large j), and a refused rate is one where they
    can part -- 1001 Hz parts at j = 1000.  Only REFUSED rates go through the entry points here: they return before any device call."""
    from fractions import Fraction
    lib = _lib.load_library()
    d = C.c_void_p(4096)
    j = np.concatenate([np.arange(0, 3600001, dtype=np.int64), np.arange(10 ** 9, 10 ** 9 + 100000, dtype=np.int64)])
    for sr in RATES:
        assert lib.taco_pcm_rate_supported(sr) == 1, sr                                              # each of the usual rates is taken
    refused = []
    for sr in RATES + (1, 7, 999, 1000, 1001, 6000, 8192, 11024, 12000, 37800, 44056, 47952, 50000, 88200, 96000, 176400, 192000):
        up = Fraction(sr / 1000.0) >= Fraction(sr, 1000)
        assert lib.taco_pcm_rate_supported(sr) == int(up), sr
        if up:
            assert np.array_equal(j * sr // 1000, (j.astype(np.float64) * (sr / 1000.0)).astype(np.int64)), sr
        else:
            refused.append(sr)
    assert set(refused) >= {999, 1001, 11024, 37800, 44056, 47952} and not set(refused) & set(RATES)
    assert lib.taco_pcm_rate_supported(0) == 0 and lib.taco_pcm_rate_supported(-8000) == 0
    assert R.frame_of_ms(1000, 1001) != R.frame_of_ms_pydub(1000, 1001)
    for sr in refused:
        assert lib.taco_pcm_nonsilent(None, d, None, 1, 1000, 1, sr, 100, 327, 4, d, d, None, None, d, 1 << 30) == _lib.TACO_ERR_UNSUPPORTED, sr
        assert b"sample_rate" in lib.taco_last_error()
        assert lib.taco_pcm_range_sumsq(None, d, None, 1, 1000, 1, sr, d, d, 4, d, d) == _lib.TACO_ERR_UNSUPPORTED
        assert lib.taco_pcm_apply_gains(None, d, None, 1, 1000, 1, sr, d, d, 4, d, d, 1000, None) == _lib.TACO_ERR_UNSUPPORTED
        assert lib.taco_debug_pcm_energy(None, d, None, 1, 1000, 1, sr, d) == _lib.TACO_ERR_UNSUPPORTED


def test_length_in_milliseconds_rounds_half_to_even():
    assert R.len_ms(4, 8000) == 0 and R.len_ms(12, 8000) == 2 and R.len_ms(20, 8000) == 2 and R.len_ms(28, 8000) == 4      # 0.5, 1.5, 2.5, 3.5
    assert R.len_ms(44100, 44100) == 1000 and R.len_ms(0, 8000) == 0
    for n, sr in [(4, 8000), (12, 8000), (20, 8000), (28, 8000), (22, 44100), (23, 44100), (66, 44100), (67, 44100)]:
        assert audio.pcm_len_ms(n, sr) == R.len_ms(n, sr)


def test_threshold_bound():
    assert audio.pcm_threshold(-40) == int(math.floor(R.threshold(-40))) == 327 and audio.pcm_threshold(-50) == 103
    assert audio.pcm_threshold(0) == 32768 and audio.pcm_threshold(60) == 32768 and audio.pcm_threshold(-400) == 0


# ---- literal == fast ----
@needs_audioop
@pytest.mark.parametrize("sr,channels", [(8000, 1), (8000, 2), (11025, 1), (44100, 2)])
def test_literal_and_fast_forms_agree_on_random_recordings(sr, channels):
    n = sr * 6 // 10 + 3
    segs = [(sr // 20, sr // 8, 9000), (sr // 5, sr // 4, 2000), (sr // 4, sr * 3 // 10, 32767), (sr * 45 // 100, sr // 2, 1500)]
    x = R.bursts(n, channels, segs, seed=sr + channels, noise=150)
    x[sr // 4] = -32768
    seg = R.Segment.of(x, sr)
    for W, db in [(10, -40), (25, -30), (100, -40), (7, -46.5)]:
        assert R.detect_nonsilent_literal(seg, W, db) == R.detect_nonsilent(x, sr, W, db)[0], (W, db)
        S, c, M = R.window_sumsq(x, sr, W)
        lit = [seg.slice(i, i + W) for i in range(0, M - W + 1, 37)]
        assert [len(s.data) // 2 for s in lit] == c[::37].tolist()
        assert [int(np.sum(s.frames().astype(np.int64) ** 2)) for s in lit] == S[::37].tolist()
    assert len(R.detect_nonsilent(x, sr, 10, -40)[0]) >= 3


@needs_audioop
def test_the_integer_comparison_is_audioops_rms_on_boundary_windows():
    """Windows built to sit on the boundary: constant amplitude k + 1 (rms = k + 1: not silent), one sample lowered by one (rms = k:
    silent), and random windows whose mean square falls within a few units of (k + 1)^2."""
    rs = np.random.RandomState(5)
    for k in (0, 1, 103, 327, 5000, 32766, 32767):
        kk = (k + 1) ** 2
        for c in (1, 2, 7, 80, 441, 8820):
            a = np.full(c, min(k + 1, 32767), np.int64)
            cases = [a.copy(), a.copy()]
            cases[1][rs.randint(c)] -= 1
            for _ in range(20):
                v = np.clip(a + rs.randint(-3, 4, size=c), -32768, 32767)
                cases.append(v)
            for v in cases:
                S = int((v * v).sum())
                rms = R.audioop.rms(v.astype("<i2").tobytes(), 2)
                assert (rms <= k) == (S < kk * c), (k, c, S, rms)
    assert R.audioop.rms(b"", 2) == 0      # an empty fragment is silent: the c == 0 clause


@needs_audioop
def test_amplify_literal_and_fast_forms_agree():
    sr = 8000
    x = R.bursts(sr * 2, 2, [(1000, 4000, 700), (7000, 7600, 12000), (11000, 15000, 90)], seed=3, noise=1)
    x[7100] = (-32768, 32767)
    for db, W in [(-50, 300), (-40, 100), (-60, 50)]:
        assert np.array_equal(R.amplify_literal(x, sr, -20.0, db, W), R.amplify(x, sr, -20.0, db, W)), (db, W)
        assert np.array_equal(R.amplify_literal(x, sr, -3.0, db, W), R.amplify(x, sr, -3.0, db, W)), (db, W)      # a target that clips
    for f in (0.0, 1.0, 2.0, 0.5, 1.5, 3.3333, 45.0, -1.0, -0.5):
        v = np.array([-32768, -32767, -3, -2, -1, 0, 1, 2, 3, 77, 32767], np.int16)
        assert np.array_equal(np.frombuffer(R.audioop.mul(v.astype("<i2").tobytes(), 2, f), "<i2"), R.mul(v, f)), f


# ---- every branch of detect_silence / detect_nonsilent, on one millisecond of constant amplitude per pattern entry ----
SR, W, PATTERNS = R.PATTERN_SR, R.PATTERN_W, R.PATTERNS


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_hand_written_patterns(name):
    pattern, want = PATTERNS[name]
    for channels in (1, 2):
        x = R.render(pattern, SR, channels)
        assert R.detect_nonsilent(x, SR, W, -40) == (want, len(pattern)), name
        if R.HAVE_AUDIOOP:
            assert R.detect_nonsilent_literal(R.Segment.of(x, SR), W, -40) == want, name


def test_the_walk_over_silent_starts():
    f = lambda starts, M: R.invert(R.ranges_from_starts(starts, M, 4), M)
    assert R.ranges_from_starts([0, 1, 2, 7, 8], 20, 4) == [[0, 6], [7, 12]]          # 7 > 2 + 4: a new range
    assert R.ranges_from_starts([0, 1, 2, 6, 7], 20, 4) == [[0, 11]]                   # 6 <= 2 + 4: the range goes on
    assert f([0, 1, 2, 7, 8], 20) == [[6, 7], [12, 20]] and f([], 20) == [[0, 20]] and f([16], 20) == [[0, 16]]
    assert f(list(range(17)), 20) == [] and f([0], 20) == [[4, 20]]


def test_length_rounded_up_reads_zero_frames_that_count():
    """20 frames at 8 kHz are 2.5 ms -> M = 2 (half to even, rounded down: the last 4 frames are never looked at); 28 frames are 3.5 ms ->
    M = 4 (rounded up): window [2, 4) covers frames [16, 32), of which 4 are zero frames that still count in c."""
    x = np.full((28, 1), 1000, np.int16)
    S, c, M = R.window_sumsq(x, SR, 2)
    assert M == 4 and c.tolist() == [16, 16, 16] and S.tolist() == [16 * 10 ** 6, 16 * 10 ** 6, 12 * 10 ** 6]
    S, c, M = R.window_sumsq(x[:20], SR, 2)
    assert M == 2 and c.tolist() == [16] and S.tolist() == [16 * 10 ** 6]
    if R.HAVE_AUDIOOP:
        seg = R.Segment.of(x, SR).slice(2, 4)
        assert len(seg.data) == 32 and seg.frames()[12:].tolist() == [[0]] * 4
    assert R.len_ms(12, SR) == 2 and R.len_ms(4, SR) == 0


# ---- split_on_silence_with_pydub: the merge loop, keep_silence, skip_idx ----
def test_merge_loop_drops_the_last_range_unless_asked():
    r = [[0, 100], [300, 500], [1000, 1200], [1500, 1700], [2500, 2600]]
    assert silence.merge_ranges_pydub(r, 400) == [[0, 500], [1000, 1700]]                          # [2500, 2600] is never visited
    assert silence.merge_ranges_pydub(r, 400, include_last_range=True) == [[0, 500], [1000, 1700], [2500, 2600]]
    assert silence.merge_ranges_pydub(r, 300) == [[0, 500], [1000, 1200], [1500, 1700]]           # 1500 - 1200 < 300 is false: strict
    assert silence.merge_ranges_pydub(r, 301) == [[0, 500], [1000, 1700]] and silence.merge_ranges_pydub(r, 501) == [[0, 1700]]
    assert silence.merge_ranges_pydub(r, 900, include_last_range=True) == [[0, 2600]]
    assert silence.merge_ranges_pydub([[5, 9]], 400) == [[5, 9]] and silence.merge_ranges_pydub([[5, 9], [20, 30]], 400) == [[5, 9]]
    assert silence.merge_ranges_pydub([[5, 9], [20, 30]], 400, include_last_range=True) == [[5, 30]]
    with pytest.raises(IndexError):
        silence.merge_ranges_pydub([], 400)


_speech = R.speech


@pytest.mark.parametrize("channels", [1, 2])
def test_split_on_silence_pydub_host_logic_equals_the_restatement(channels):
    sr = 8000
    x = _speech(sr, channels)
    for kw in (dict(), dict(include_last_range=True), dict(skip_idx=1), dict(keep_silence=1000), dict(min_silence_len=50, include_last_range=True),
               dict(silence_thresh=-30, silence_chunk_len=50, keep_silence=0)):
        ref = R.split_on_silence_with_pydub(x, sr, **kw)
        dev = R.StandIn()
        got = silence.split_on_silence_pydub(x if channels == 2 else x[:, 0], sr, device=dev, **kw)
        assert [g[:3] for g in got] == [r[:3] for r in ref] and len(got) >= 1, kw
        for g, r in zip(got, ref):
            assert g[3].dtype == np.int16 and np.array_equal(g[3].reshape(len(g[3]), -1), r[3])
        assert dev.calls == [("nonsilent", sr, kw.get("silence_chunk_len", 100), kw.get("silence_thresh", -40))]
    base = silence.split_on_silence_pydub(x, sr, device=R.StandIn())
    full = silence.split_on_silence_pydub(x, sr, include_last_range=True, device=R.StandIn())
    assert len(base) == 2 and len(full) == 3 and [s[:3] for s in full[:2]] == [s[:3] for s in base]      # the reference drops the last utterance
    assert [s[0] for s in full] == [0, 1, 2] and full[0][1] < 40 and 700 <= full[0][2] <= 801       # the first two utterances merged, 100 ms kept
    assert full[2][2] <= 2400
    skipped = silence.split_on_silence_pydub(x, sr, skip_idx=1, include_last_range=True, device=R.StandIn())
    assert [s[:3] for s in skipped] == [(0,) + full[1][1:3], (1,) + full[2][1:3]]                   # idx counts from skip_idx
    clamped = silence.split_on_silence_pydub(x, sr, keep_silence=5000, include_last_range=True, device=R.StandIn())
    assert all(s[1] == 0 and s[2] == 2400 and len(s[3]) == len(x) for s in clamped)                 # both ends clamped to [0, M]
    if R.HAVE_AUDIOOP:
        lit = R.split_on_silence_with_pydub(x, sr, literal=True)
        assert [s[:3] for s in lit] == [s[:3] for s in base]


def test_an_all_silent_recording_is_an_error_for_the_split():
    with pytest.raises(Exception, match="no non-silent range"):
        silence.split_on_silence_pydub(np.zeros(8000, np.int16), 8000, device=R.StandIn())
    with pytest.raises(IndexError):      # the reference's not_silence_ranges[0]
        R.split_on_silence_with_pydub(np.zeros(8000, np.int16), 8000)


# ---- amplify ----
def test_amplify_drops_the_head_runs_the_last_range_to_the_end_and_copies_zero_energy():
    sr = 8000
    ms = lambda a: a * sr // 1000
    x = R.bursts(ms(2000), 1, [(ms(350), ms(700), 500), (ms(1200), ms(1500), 2000)], seed=2, noise=0)[:, 0]
    x[ms(1500):ms(1650)] = 1                               # below -50 dBFS, but not zero: the tail the last range takes in
    dev = R.StandIn()
    y = silence.amplify(x, sr, device=dev)
    ranges, M = R.detect_nonsilent(x, sr, 300, -50)
    assert M == 2000 and len(ranges) == 2 and ranges[0][0] > 300 and ranges[1][1] < 1700
    assert y.dtype == np.int16 and y.ndim == 1 and len(y) == ms(M) - ms(ranges[0][0])              # the head is dropped
    assert np.array_equal(y, R.amplify(x, sr)[:, 0])
    assert [c[0] for c in dev.calls] == ["nonsilent", "range_sumsq", "apply_gains"]
    first = ms(ranges[0][0])
    gap = slice(ms(ranges[0][1]) - first, ms(ranges[1][0]) - first)
    assert np.array_equal(y[gap], x[ms(ranges[0][1]):ms(ranges[1][0])])                             # between two ranges: unchanged
    S, c = R.range_sumsq(x, sr, [ranges[0], [ranges[1][0], M]])
    g = [silence.amplify_gain(s, k) for s, k in zip(S, c)]
    assert g == [R.gain(s, k) for s, k in zip(S, c)] and g[0] > g[1] > 1.0
    tail = slice(ms(1500) - first, ms(1650) - first)
    assert np.array_equal(y[tail], R.mul(x[ms(1500):ms(1650)], g[1])) and y[tail].max() >= 1        # the last range runs to M
    rms = int(math.sqrt(S[0] / float(c[0])))
    assert abs(20 * math.log10(rms * g[0] / 32768.0) + 20.0) < 1e-9
    # a range of zero energy: a recording shorter than the window is one range [0, M], and silent samples give S = 0 -> a copy
    z = np.zeros(ms(200), np.int16)
    assert silence.amplify_gain(0, 1600) == 1.0 and silence.amplify_gain(0, 0) == 1.0 and silence.amplify_gain(1599, 1600) == 1.0
    assert np.array_equal(silence.amplify(z, sr, device=R.StandIn()), z)
    # no range at all: empty
    assert silence.amplify(np.zeros(ms(1000), np.int16), sr, device=R.StandIn()).shape == (0,)
    assert silence.amplify(np.zeros((ms(1000), 2), np.int16), sr, device=R.StandIn()).shape == (0, 2)
    st = np.stack([x, x[::-1]], axis=1)
    assert np.array_equal(silence.amplify(st, sr, device=R.StandIn()), R.amplify(st, sr))


# ---- the entry points' argument errors ----
def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory: validation rejects every one of these calls before it is touched."""
    lib = _lib.load_library()
    d = C.c_void_p(4096)
    E, U = _lib.TACO_ERR_ARG, _lib.TACO_ERR_UNSUPPORTED

    def ns(pcm=d, nf=None, B=2, L=1000, ch=1, sr=8000, W=100, k=327, R_=4, ranges=d, counts=d, len_ms=None, wss=None, ws=d, ws_bytes=1 << 20):
        return lib.taco_pcm_nonsilent(None, pcm, nf, B, L, ch, sr, W, k, R_, ranges, counts, len_ms, wss, ws, ws_bytes)

    assert ns(pcm=None) == E and ns(ranges=None) == E and ns(counts=None) == E and ns(ws=None) == E
    assert ns(B=0) == E and ns(L=0) == E and ns(ch=0) == E and ns(sr=0) == E and ns(W=0) == E and ns(W=-5) == E
    assert ns(R_=0) == E and ns(R_=-1) == E
    assert b"max_ranges" in lib.taco_last_error()
    assert ns(k=-1) == E
    need = int(lib.taco_pcm_nonsilent_workspace_bytes(2, 1000, 8000))
    assert need > 0 and ns(ws_bytes=need - 1) == E and ns(ws_bytes=0) == E
    assert b"workspace" in lib.taco_last_error()
    assert ns(pcm=C.c_void_p(4097)) == E and ns(ws=C.c_void_p(4100)) == E
    assert ns(W=7905) == U and b"min_silence_len" in lib.taco_last_error()                          # 256 + W energies of 8 bytes pass 64 KB
    assert ns(k=32768, W=7000, sr=48000, ch=16, L=1 << 20, ws_bytes=1 << 30) == U and b"2^52" in lib.taco_last_error()
    assert ns(k=2 ** 31 - 1, W=7000, sr=48000, ch=16, L=1 << 20, ws_bytes=1 << 30) == U and b"k 32768" in lib.taco_last_error()      # taken as 32768
    assert ns(sr=1001) == U
    assert ns(sr=30000000, ch=2, ws_bytes=1 << 30) == U and b"LDS" in lib.taco_last_error()     # one millisecond of samples exceeds the tile

    def rs(e=d, nf=None, B=2, L=1000, ch=1, sr=8000, ranges=d, counts=d, R_=4, sumsq=d, samples=d):
        return lib.taco_pcm_range_sumsq(None, e, nf, B, L, ch, sr, ranges, counts, R_, sumsq, samples)

    assert rs(e=None) == E and rs(ranges=None) == E and rs(counts=None) == E and rs(sumsq=None) == E and rs(samples=None) == E
    assert rs(B=0) == E and rs(L=0) == E and rs(ch=0) == E and rs(sr=0) == E and rs(R_=0) == E
    assert rs(e=C.c_void_p(4100)) == E and rs(sr=1001) == U

    def ag(pcm=d, nf=None, B=2, L=1000, ch=1, sr=8000, ranges=d, counts=d, R_=4, gains=d, out=d, L_out=1000, on=None):
        return lib.taco_pcm_apply_gains(None, pcm, nf, B, L, ch, sr, ranges, counts, R_, gains, out, L_out, on)

    assert ag(pcm=None) == E and ag(ranges=None) == E and ag(counts=None) == E and ag(gains=None) == E and ag(out=None) == E
    assert ag(B=0) == E and ag(L=0) == E and ag(ch=0) == E and ag(sr=0) == E and ag(R_=0) == E and ag(L_out=0) == E
    assert ag(gains=C.c_void_p(4100)) == E and ag(sr=1001) == U
