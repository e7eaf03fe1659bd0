"""The pydub method on the device (taco_pcm_nonsilent, taco_pcm_range_sumsq, taco_pcm_apply_gains, GriffinLim.nonsilent / range_sumsq /
apply_gains, silence.split_on_silence_pydub, silence.amplify) against the restatement tests/pydub_reference.py and the standard library's
audioop.  UNPINNED on pydub (see the restatement's header): what is held here is the kernels against that restatement, not against pydub.

Everything is integer arithmetic, or one correctly rounded double product followed by floor: every comparison is for EQUALITY, there
is no tolerance anywhere in this file.  Samples past a row's own frames are filled with 32767: read, they would change a sum."""
import functools
import math

import numpy as np
import pytest

import pydub_reference as R

pytestmark = pytest.mark.gpu


class _HP(object):
    sample_rate, num_freq, frame_length_ms, frame_shift_ms = 1600, 65, 50, 12.5      # (the handle's STFT is not used here; every call names its rate)


@pytest.fixture(scope="module")
def gl():
    import taco_amd
    g = taco_amd.GriffinLim(_HP())
    yield g
    g.close()


def _rounded_up(sr, W):
    """The smallest n of more than W + 1 milliseconds whose length in milliseconds is rounded UP past it: p(M) > n"""
    n = R.frame_of_ms(W + 1, sr) + 1
    while R.frame_of_ms(R.len_ms(n, sr), sr) <= n:
        n += 1
    return n


@functools.lru_cache(maxsize=None)
def _ragged(sr, channels, W):
    """(rectangle int16 [B, L, channels] with 32767 past every row's frames, lengths): n in {0, 1, fewer than W ms, exactly W ms, W ms
    and a half (rounded to even), rounded up past n, about 2600 ms}"""
    p = lambda j: R.frame_of_ms(j, sr)
    lengths = [0, 1, p(W) - p(1) - 1, p(W), _rounded_up(sr, W), p(2600) + 3, p(W) + p(1) // 2, p(900)]
    L = max(lengths)
    x = np.full((len(lengths), L, channels), 32767, np.int16)
    for b, n in enumerate(lengths):
        segs = [(lo * n // 100, hi * n // 100, amp) for lo, hi, amp in [(5, 20, 9000), (30, 33, 32767), (45, 60, 700), (62, 63, 330), (80, 95, 4000)]]
        x[b, :n] = R.bursts(n, channels, segs, seed=100 * b + channels, noise=120)
        if n > 4:
            x[b, n // 3, 0], x[b, n // 3 + 1, -1], x[b, n - 1, 0] = -32768, 32767, -32767
    x.setflags(write=False)
    return x, lengths


@functools.lru_cache(maxsize=None)
def _ragged_reference(sr, channels, W):
    """Per row (S, c, M, E, ranges): computed once, shared, not modified."""
    x, lengths = _ragged(sr, channels, W)
    out = []
    for b, n in enumerate(lengths):
        S, c, M = R.window_sumsq(x[b, :n], sr, W)
        cs = R.prefix_squares(x[b, :n], sr)[0]
        j = np.arange(M + 1, dtype=np.int64) * sr // 1000
        out.append((S, c, M, cs[j[1:]] - cs[j[:-1]], R.detect_nonsilent(x[b, :n], sr, W, -40)[0]))
    return out


@pytest.mark.parametrize("sr,channels,W", [(8000, 1, 30), (8000, 2, 100), (44100, 1, 100), (44100, 2, 30)])
def test_energies_window_sums_and_ranges_of_ragged_rows_equal_the_restatement(gl, sr, channels, W):
    import torch
    x, lengths = _ragged(sr, channels, W)
    ref = _ragged_reference(sr, channels, W)
    B, L = len(lengths), x.shape[1]
    mmax = R.len_ms(L, sr)
    assert R.frame_of_ms(ref[4][2], sr) > lengths[4] and ref[4][2] >= W and ref[2][2] < W and ref[3][2] == W      # the rows are what they are meant to be
    assert len(ref[5][0]) > 2 * 256 and ref[5][2] > 64 and len(ref[5][4]) >= 3
    nf = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    ranges, counts, len_ms, wss, energy = gl.nonsilent(torch.from_numpy(np.array(x)).cuda(), nf, sr, W, -40, return_window_sumsq=True, return_energy=True)
    assert ranges.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(wss.shape) == (B, mmax) == tuple(energy.shape)
    assert tuple(ranges.shape) == (B, mmax // (W + 1) + 2, 2)
    ranges, counts, len_ms, wss, energy = [t.cpu().numpy() for t in (ranges, counts, len_ms, wss, energy)]
    for b, (S, c, M, E, rr) in enumerate(ref):
        print("%d Hz x %d, W %d, row %d: n %d, M %d, %d windows, %d ranges %s" % (sr, channels, W, b, lengths[b], M, len(S), len(rr), rr[:4]))
        assert len_ms[b] == M
        assert np.array_equal(energy[b, :M], E), (b, np.flatnonzero(energy[b, :M] != E)[:5])
        assert np.array_equal(wss[b, :len(S)], S) and not wss[b, len(S):].any(), (b, np.flatnonzero(wss[b, :len(S)] != S)[:5])
        assert counts[b] == len(rr) and ranges[b, :len(rr)].tolist() == rr, (b, counts[b], ranges[b, :counts[b]].tolist(), rr)
        assert not ranges[b, len(rr):].any()
    assert counts[0] == 1 and ranges[0, 0].tolist() == [0, 0]      # an empty row: pydub's [[0, len]] with len = 0


def test_the_energy_pass_alone_writes_the_same_energies(gl):
    """taco_debug_pcm_energy (the timing hook of tools/bench_audio.py --pydub) is the first launch of taco_pcm_nonsilent and nothing else"""
    import ctypes as C
    import torch
    import taco_amd
    sr, channels, W = 44100, 2, 30
    x, lengths = _ragged(sr, channels, W)
    xs = torch.from_numpy(np.array(x)).cuda()
    nf = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    B, L = xs.shape[0], xs.shape[1]
    energy = torch.full((B, R.len_ms(L, sr)), -1, dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    taco_amd._lib.check(gl._lib.taco_debug_pcm_energy(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(xs), p(nf), B, L, channels, sr, p(energy)))
    energy = energy.cpu().numpy()
    for b, (S, c, M, E, rr) in enumerate(_ragged_reference(sr, channels, W)):
        assert np.array_equal(energy[b, :M], E) and (energy[b, M:] == -1).all(), b                   # nothing at or past M_b is written


def test_threshold_edge_at_a_tile_boundary_and_in_the_last_window(gl):
    """Constant amplitude k + 1 is NOT silent (rms = k + 1 > thresh); the same windows with one sample lowered by one are (rms = k).  The
    lowered sample sits in millisecond 260, so the silent starts 251..260 straddle the boundary between the first two tiles of 256
    starts -- and, in another row, in the last millisecond, so that the last window of the row alone is silent."""
    import torch
    sr, W, db, M = 8000, 10, -40, 530
    k = int(math.floor(R.threshold(db)))
    assert k == 327
    n = R.frame_of_ms(M, sr)
    x = np.full((4, n, 1), k + 1, np.int16)
    x[1, R.frame_of_ms(260, sr) + 3] -= 1
    x[2, n - 1] -= 1
    x[3] = -(k + 1)
    x[3, R.frame_of_ms(255, sr)] += 1                      # (negative samples: |x| one lower) silent starts 246..255, the last of the first tile
    want = [[[0, M]], [[0, 251], [270, M]], [[0, M - W]], [[0, 246], [265, M]]]
    for b in range(4):
        assert R.detect_nonsilent(x[b], sr, W, db)[0] == want[b]
    ranges, counts, len_ms, wss = gl.nonsilent(torch.from_numpy(x).cuda(), None, sr, W, db, return_window_sumsq=True)
    ranges, counts, wss = ranges.cpu().numpy(), counts.cpu().numpy(), wss.cpu().numpy()
    c = W * 8
    for b in range(4):
        assert ranges[b, :counts[b]].tolist() == want[b], (b, ranges[b, :counts[b]].tolist())
        assert np.array_equal(wss[b, :M - W + 1], R.window_sumsq(x[b], sr, W)[0])
    assert (wss[0, :M - W + 1] == (k + 1) ** 2 * c).all()                                             # S == (k + 1)^2 c: not below it
    assert (wss[1, 251:261] == (k + 1) ** 2 * c - (2 * k + 1)).all() and wss[1, 250] == wss[1, 261] == (k + 1) ** 2 * c
    assert wss[2, M - W] == (k + 1) ** 2 * c - (2 * k + 1) and wss[2, M - W - 1] == (k + 1) ** 2 * c


def test_ranges_and_counts_on_the_hand_written_patterns(gl):
    """The patterns of tests/test_pydub_host.py rendered as samples, one row each, in one ragged rectangle"""
    import torch
    sr, W = R.PATTERN_SR, R.PATTERN_W
    names = sorted(R.PATTERNS)
    for channels in (1, 2):
        rows = [R.render(R.PATTERNS[nm][0], sr, channels) for nm in names]
        L = max(len(r) for r in rows)
        x = np.full((len(rows), L, channels), 32767, np.int16)
        for b, r in enumerate(rows):
            x[b, :len(r)] = r
        nf = torch.tensor([len(r) for r in rows], dtype=torch.int32, device="cuda")
        ranges, counts, len_ms = gl.nonsilent(torch.from_numpy(x).cuda(), nf, sr, W, -40)
        ranges, counts, len_ms = ranges.cpu().numpy(), counts.cpu().numpy(), len_ms.cpu().numpy()
        for b, nm in enumerate(names):
            pattern, want = R.PATTERNS[nm]
            assert len_ms[b] == len(pattern) and ranges[b, :counts[b]].tolist() == want, (nm, ranges[b, :counts[b]].tolist(), want)
            assert not ranges[b, counts[b]:].any()


@functools.lru_cache(maxsize=None)
def _long_patterns():
    """Row 0: more ranges than the table holds.  Row 1: 700 ms, W = 4, three chunks of 256 starts: silent runs that straddle the wave
    edge 63|64 and the chunk edge 255|256 -- the latter the second run of a range whose first run {251, 252} lies before it (joined
    because 255 <= 252 + 4) -- and an opening whose look back crosses the chunk edge 511|512 (a run that ends at 500, the next opens at 514)."""
    many = ([1] * 2 + [0] * 5) * 20 + [1]
    row = [1] * 700
    for lo, hi in [(60, 70), (120, 124), (300, 340), (497, 504), (514, 520), (680, 700)]:
        row[lo:hi] = [0] * (hi - lo)
    row[251:260] = [0, 0, 0, 2, 0, 2, 0, 0, 0]
    return many, row


def test_more_ranges_than_the_table_holds_and_runs_across_chunk_edges(gl):
    import torch
    sr, W = R.PATTERN_SR, R.PATTERN_W
    many, row = _long_patterns()
    rows = [R.render(many, sr, 1), R.render(row, sr, 1)]
    want = [R.detect_nonsilent(r, sr, W, -40)[0] for r in rows]
    assert len(want[0]) == 21 and [251, 260] not in want[1] and [250, 251] not in want[1]
    flags = R.silent_flags(rows[1], sr, W, -40)[0]
    assert flags[[63, 64, 252, 255, 256, 500, 514]].all() and not flags[[253, 254, 501, 513]].any()
    L = max(len(r) for r in rows)
    x = np.full((2, L, 1), 32767, np.int16)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    nf = torch.tensor([len(r) for r in rows], dtype=torch.int32, device="cuda")
    for max_ranges in (3, 40):
        ranges, counts, _ = gl.nonsilent(torch.from_numpy(x).cuda(), nf, sr, W, -40, max_ranges=max_ranges)
        ranges, counts = ranges.cpu().numpy(), counts.cpu().numpy()
        assert tuple(ranges.shape) == (2, max_ranges, 2)
        for b in range(2):
            kept = min(len(want[b]), max_ranges)
            print("max_ranges %d row %d: count %d, first ranges %s" % (max_ranges, b, counts[b], ranges[b, :4].tolist()))
            assert counts[b] == len(want[b])                                                         # the true count, whatever the table holds
            assert ranges[b, :kept].tolist() == want[b][:kept] and not ranges[b, kept:].any()
    assert len(want[1]) > 3


def _audioop_or_restatement():
    if R.HAVE_AUDIOOP:
        return (lambda v: R.audioop.rms(np.ascontiguousarray(v).astype("<i2").tobytes(), 2),
                lambda v, f: np.frombuffer(R.audioop.mul(np.ascontiguousarray(v).astype("<i2").tobytes(), 2, f), "<i2").reshape(v.shape))
    return (lambda v: int(math.sqrt(float((v.astype(np.int64) ** 2).sum()) / v.size)) if v.size else 0), R.mul


@pytest.mark.parametrize("sr,channels", [(8000, 2), (44100, 1)])
def test_range_sums_and_gains_equal_audioop_on_the_same_slices(gl, sr, channels):
    """Factors that clip (45, -1 on -32768), factors whose product lands exactly on an integer (2, 0.5 on even samples, 1), products
    that need floor on negative samples (0.5, 1.5, 3.3333 on odd negative ones), and a range that runs into the zero frames past n."""
    import torch
    rms_of, mul_of = _audioop_or_restatement()
    W = 30
    x, lengths = _ragged(sr, channels, W)
    rows = [5, 4, 7]
    M = [R.len_ms(lengths[b], sr) for b in rows]
    table = [[[3, 40], [41, 300], [300, 301], [700, 1500], [1500, 1501], [2000, 2450], [2590, M[0]]],
             [[0, 2], [2, W], [W, M[1]], [0, 0], [0, 0], [0, 0], [0, 0]],
             [[10, 200], [250, 251], [400, 899], [899, 900], [0, 0], [0, 0], [0, 0]]]
    count = [7, 3, 4]
    gains = [[45.0, 0.5, 2.0, 1.5, -1.0, 3.3333, 1.0], [2.0, 0.5, 45.0, 9.0, 9.0, 9.0, 9.0], [0.25, -1.0, 1.0 / 3.0, 45.0, 9.0, 9.0, 9.0]]
    xs = torch.from_numpy(np.array(x[rows])).cuda()
    nf = torch.tensor([lengths[b] for b in rows], dtype=torch.int32, device="cuda")
    energy = gl.nonsilent(xs, nf, sr, W, -40, return_energy=True)[3]
    sumsq, samples = gl.range_sumsq(energy, np.array(table, np.int32), count, xs.shape[1], channels, nf, sr)
    out, on = gl.apply_gains(xs, np.array(table, np.int32), count, np.array(gains), nf, sr)
    assert out.dtype == torch.int16 and tuple(out.shape) == (3, R.frame_of_ms(R.len_ms(xs.shape[1], sr), sr), channels)
    sumsq, samples, out, on = sumsq.cpu().numpy(), samples.cpu().numpy(), out.cpu().numpy(), on.cpu().numpy()
    clipped = floored = 0
    for i, b in enumerate(rows):
        n = lengths[b]
        first, end = R.frame_of_ms(table[i][0][0], sr), R.frame_of_ms(M[i], sr)
        assert on[i] == end - first
        want = R.frames_of(x[b, :n], first, end)
        for k in range(count[i]):
            s, e = table[i][k]
            piece = R.frames_of(x[b, :n], R.frame_of_ms(s, sr), R.frame_of_ms(e, sr))          # pydub's slice: zero frames past n
            S = int((piece.astype(np.int64) ** 2).sum())
            assert sumsq[i, k] == S and samples[i, k] == piece.size, (i, k, sumsq[i, k], S)
            assert int(math.sqrt(S / float(piece.size))) == rms_of(piece)
            y = mul_of(piece, gains[i][k])
            clipped += int(((y == 32767) | (y == -32768)).sum())
            floored += int((np.floor(piece * gains[i][k]) != piece * gains[i][k]).sum())
            want[R.frame_of_ms(s, sr) - first:R.frame_of_ms(e, sr) - first] = y
        assert not sumsq[i, count[i]:].any() and not samples[i, count[i]:].any()
        assert np.array_equal(out[i, :on[i]], want), (i, np.argwhere(out[i, :on[i]] != want)[:5])
        assert not out[i, on[i]:].any()
        print("%d Hz x %d row %d: %d frames from %d, %d clipped samples, %d floored products" % (sr, channels, b, on[i], first, clipped, floored))
    assert clipped > 100 and floored > 100
    assert R.frame_of_ms(M[1], sr) > lengths[4]            # row 4's last range ends in zero frames that count


@pytest.mark.parametrize("sr,channels", [(8000, 2), (44100, 1)])
def test_split_and_amplify_end_to_end_equal_the_restatement(gl, sr, channels):
    from taco_amd import silence
    x = R.speech(sr, channels)
    pcm = x if channels == 2 else x[:, 0]
    dev = silence.PcmDevice(griffin_lim=gl)
    for kw in (dict(), dict(include_last_range=True, skip_idx=1), dict(keep_silence=3000, include_last_range=True)):
        ref = R.split_on_silence_with_pydub(x, sr, **kw)
        got = silence.split_on_silence_pydub(pcm, sr, device=dev, **kw)
        assert [g[:3] for g in got] == [r[:3] for r in ref] and len(got) >= 2, (kw, [g[:3] for g in got], [r[:3] for r in ref])
        assert all(g[3].dtype == np.int16 and g[3].shape == pcm[:len(g[3])].shape and np.array_equal(g[3].reshape(r[3].shape), r[3]) for g, r in zip(got, ref))
    y = silence.amplify(pcm, sr, device=dev)
    want = R.amplify(x, sr)
    assert y.dtype == np.int16 and len(want) > sr and np.array_equal(y.reshape(want.shape), want) and not np.array_equal(want, x[len(x) - len(want):])
    y = silence.amplify(pcm, sr, target_dbfs=-1.0, silence_thresh=-40, min_silence_len=100, device=dev)       # a target that clips
    want = R.amplify(x, sr, -1.0, -40, 100)
    assert np.array_equal(y.reshape(want.shape), want) and (want == 32767).any()
    assert silence.amplify(np.zeros(sr, np.int16), sr, device=dev).shape == (0,)
    with pytest.raises(Exception, match="no non-silent range"):
        silence.split_on_silence_pydub(np.zeros(sr, np.int16), sr, device=dev)


def test_a_float_input_is_refused_with_a_pointer_to_pcm16(gl):
    import taco_amd
    with pytest.raises(taco_amd._lib.TacoError) as e:
        gl.nonsilent(np.zeros((1, 800), np.float32), None, 8000, 10, -40)
    assert "pcm16" in str(e.value)


def test_capture_and_replay_of_every_entry_point(gl):
    import torch
    sr, channels, W = 8000, 2, 30
    x, lengths = _ragged(sr, channels, W)
    xs = torch.from_numpy(np.array(x)).cuda()
    nf = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    B, L = xs.shape[0], xs.shape[1]
    gains = torch.linspace(0.3, 40.0, B * (R.len_ms(L, sr) // (W + 1) + 2), dtype=torch.float64, device="cuda").reshape(B, -1)

    def chain():
        ranges, counts, len_ms, wss, energy = gl.nonsilent(xs, nf, sr, W, -40, return_window_sumsq=True, return_energy=True)
        sumsq, samples = gl.range_sumsq(energy, ranges, counts, L, channels, nf, sr)
        out, on = gl.apply_gains(xs, ranges, counts, gains, nf, sr)
        return ranges, counts, len_ms, wss, sumsq, samples, out, on
    eager = [t.clone() for t in chain()]
    again = chain()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))                                       # two calls, the same bits
    assert int(eager[1][5]) >= 3 and bool(eager[6].any())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = chain()
    for _ in range(2):
        for t in captured:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(eager, captured))
