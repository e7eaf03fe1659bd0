"""Splitting on silence on the device (taco_wav_split, taco_wav_breath_mute, GriffinLim.split / remove_breath, split_on_silence) against
the float64 restatement tests/split_reference.py of audio/silence.py:21-76.  UNPINNED on librosa (see the restatement's header): what
is held here is the kernels against that restatement, not against librosa.

Intervals, counts, mute flags and muted waveforms are compared for EQUALITY.  That is meaningful because every input is built so
that no frame of the restatement lies within MARGIN = 0.05 dB of the threshold and no mute decision within DECISION_MARGIN = 1e-3
of its bar (both asserted on the CPU before the device is asked), while the device's dB values are held to DB_BAR -- the trim test's
bar: the same kernel and arithmetic, measured there -- and its abs_mean values to MEAN_BAR.  MEAN_BAR is meant to be ten times the
largest |abs_mean difference| measured on an MI355X over every case of this file (printed per row with -s), rounded up, and at most
2e-4, a fifth of DECISION_MARGIN.  NOT YET MEASURED: this file has not run on a device, so the bar stands at that ceiling.  What
float32 predicts: a mean is a sum of at most 2000 terms below 2 in magnitude, added as 1024 (or 64) partial sums and a butterfly,
so its error is a few units of 6e-8 relative -- some 1e-7 absolute, three orders below the ceiling; lower the bar when it is measured."""
import ctypes as C
import functools

import numpy as np
import pytest

import split_reference as R
import trim_reference as T

pytestmark = pytest.mark.gpu

MARGIN = 0.05            # dB: no frame of the restatement may be this close to -top_db
DB_BAR = 2e-4            # dB: tests/test_gpu_trim.py's bar (ten times the 1.31e-5 measured there, rounded up)
DECISION_MARGIN = 1e-3   # no mute decision of the restatement may be this close to running mean - threshold
MEAN_BAR = 2e-4          # the most the comparison allows (a fifth of DECISION_MARGIN)
assert DB_BAR <= MARGIN / 5 and MEAN_BAR <= DECISION_MARGIN / 5

L = 700
LENGTHS = [700, 451, 64, 33, 9, 1]
BURSTS = [[(0, 60), (150, 260), (300, 330), (480, 560), (640, 700)], [(30, 120), (200, 260), (380, 451)], [(8, 24), (40, 64)], [(0, 10), (20, 33)],
          [(3, 6)], []]                                      # row b: RandomState(b); noise 1e-4, then the bursts at 0.3 in order
PARAMS = [(16, 2), (64, 8)]      # 351 frames: the prefix count crosses waves and a 256-frame chunk; 64/8: repeated reflection on the short rows
TOP_DB = 40.0


class _HP(object):
    sample_rate, num_freq, frame_length_ms, frame_shift_ms = 1600, 65, 50, 12.5


@pytest.fixture(scope="module")
def gl():
    import taco_amd
    g = taco_amd.GriffinLim(_HP())
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _rows():
    x = np.zeros((len(LENGTHS), L), np.float32)
    for b, (n, bursts) in enumerate(zip(LENGTHS, BURSTS)):
        x[b, :n] = R.pieces(n, [(lo, hi, 0.3) for lo, hi in bursts], b)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _split_case(N, hop):
    """{energy: [(intervals, db, margin) per row]}: computed once, shared, not modified."""
    x = _rows()
    return {e: [R.split(x[b, :n], TOP_DB, N, hop, e) for b, n in enumerate(LENGTHS)] for e in R.ENERGIES}


def _check_margins(ref, what):
    for e, rows in ref.items():
        for b, (iv, db, margin) in enumerate(rows):
            print("%s %s row %d: restatement %d intervals %s, margin %.3f dB" % (what, e, b, len(iv), iv.tolist(), margin))
            assert margin >= MARGIN, (what, e, b, margin)


def _device_rows():
    import torch
    xn = np.array(_rows(), copy=True)
    for b, n in enumerate(LENGTHS):
        xn[b, n:] = np.nan                                    # nothing at or past n_b may be read
    return torch.from_numpy(xn).cuda(), torch.tensor(LENGTHS, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("energy", R.ENERGIES)
@pytest.mark.parametrize("N,hop", PARAMS)
def test_ragged_rows_intervals_equal_the_restatement(gl, N, hop, energy):
    import torch
    ref = _split_case(N, hop)
    _check_margins(ref, "%d/%d" % (N, hop))
    assert len(ref["spectral"][0][0]) == (5 if (N, hop) == (16, 2) else 4)
    assert ref["spectral"][0][0].tolist() != ref["time"][0][0].tolist()
    w, ns = _device_rows()
    intervals, counts, db = gl.split(w, ns, top_db=TOP_DB, frame_length=N, hop_length=hop, energy=energy, return_db=True)
    fmax = 1 + L // hop
    M = (fmax + 1) // 2
    assert intervals.dtype == torch.int32 and counts.dtype == torch.int32
    assert tuple(intervals.shape) == (6, M, 2) and tuple(counts.shape) == (6,) and tuple(db.shape) == (6, fmax)
    intervals, counts, db = intervals.cpu().numpy(), counts.cpu().numpy(), db.cpu().numpy()
    assert np.isfinite(db).all()
    for b, (riv, rdb, margin) in enumerate(ref[energy]):
        nf = len(rdb)
        d = float(np.abs(db[b, :nf] - rdb).max()) if nf else 0.0
        print("%d/%d %s row %d: device %d intervals %s, max |dB difference| %.3g over %d frames" % (N, hop, energy, b, counts[b], intervals[b, :counts[b]].tolist(), d, nf))
        assert counts[b] == len(riv) and intervals[b, :len(riv)].tolist() == riv.tolist(), (b, counts[b], intervals[b, :counts[b]].tolist(), riv.tolist())
        assert np.all(intervals[b, len(riv):] == 0) and np.all(db[b, nf:] == 0.0)
        assert d <= DB_BAR, (b, d)
    assert counts[5] == 0 and counts[0] > 1


@pytest.mark.parametrize("energy", R.ENERGIES)
@pytest.mark.parametrize("N,hop", PARAMS)
def test_trim_and_split_return_the_same_frame_db_bits(gl, N, hop, energy):
    """k_trim_index and k_split_edges form a frame's dB with the same device functions, so the two tables are equal as bits, and the
    loudest frame of every row that has frames (two samples or more) is exactly 0 dB (the product is rounded before the subtraction)."""
    w, ns = _device_rows()
    _, tdb = gl.trim(w, ns, top_db=TOP_DB, frame_length=N, hop_length=hop, energy=energy, return_db=True)
    _, _, sdb = gl.split(w, ns, top_db=TOP_DB, frame_length=N, hop_length=hop, energy=energy, return_db=True)
    tdb, sdb = tdb.cpu().numpy(), sdb.cpu().numpy()
    assert tdb.shape == sdb.shape == (6, 1 + L // hop) and np.isfinite(tdb).all()
    assert np.array_equal(tdb.view(np.uint32), sdb.view(np.uint32))
    for b, n in enumerate(LENGTHS):
        nf = 1 + n // hop if n >= 2 else 0
        assert np.all(tdb[b, nf:] == 0.0)
        if nf:
            assert tdb[b, :nf].max() == 0.0 and sdb[b, :nf].max() == 0.0, (b, tdb[b, :nf].max(), sdb[b, :nf].max())


def test_overflow_keeps_the_counts_and_writes_only_zeros_past_the_first_two(gl):
    """max_intervals = 2 on the 16/2 input, through the library into a table with a sentinel on both sides of it."""
    import torch
    from taco_amd import _lib
    ref = _split_case(16, 2)["spectral"]
    w, ns = _device_rows()
    B, M, guard = 6, 2, 64
    buf = torch.full((guard + B * M * 2 + guard,), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    nb = int(gl._lib.taco_wav_split_workspace_bytes(B, L, 16, 2))
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    _lib.check(gl._lib.taco_wav_split(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(w.data_ptr()), C.c_void_p(ns.data_ptr()), B, L,
                                      TOP_DB, 16, 2, _lib.TACO_TRIM_SPECTRAL, M, C.c_void_p(buf[guard:].data_ptr()), C.c_void_p(counts[1:].data_ptr()),
                                      None, C.c_void_p(ws.data_ptr()), nb))
    buf, counts = buf.cpu().numpy(), counts.cpu().numpy()
    assert np.all(buf[:guard] == -7) and np.all(buf[-guard:] == -7) and counts[0] == -7 and counts[-1] == -7
    table = buf[guard:-guard].reshape(B, M, 2)
    for b, (riv, _, _) in enumerate(ref):
        k = min(len(riv), M)
        assert counts[1 + b] == len(riv), (b, counts[1 + b], len(riv))
        assert table[b, :k].tolist() == riv[:k].tolist() and np.all(table[b, k:] == 0)
    assert [len(r[0]) for r in ref][:2] == [5, 3]             # rows that do overflow


@pytest.mark.parametrize("energy", R.ENERGIES)
@pytest.mark.parametrize("N,hop", PARAMS)
def test_the_outer_ends_are_the_trim_index(gl, N, hop, energy):
    w, ns = _device_rows()
    kw = dict(top_db=TOP_DB, frame_length=N, hop_length=hop, energy=energy)
    intervals, counts = gl.split(w, ns, **kw)
    index = gl.trim(w, ns, **kw).cpu().numpy()
    intervals, counts = intervals.cpu().numpy(), counts.cpu().numpy()
    for b, n in enumerate(LENGTHS):
        if n >= 2:
            assert counts[b] >= 1 and [intervals[b, 0, 0], intervals[b, counts[b] - 1, 1]] == index[b].tolist(), (b, index[b].tolist())


def test_only_the_last_frame_non_silent_gives_the_empty_interval(gl):
    """n = 64 = 4 * hop at 16 / 16: frame 4 is samples [56, 72) of the row (the last eight reflected), frame 3 ends at 56; a burst on
    [58, 64) is in frame 4 alone, and min(n, 4 * 16) = min(n, 5 * 16) = 64."""
    import torch
    x = np.stack([R.pieces(64, [(58, 64, 0.3)], 0), R.pieces(64, [(10, 30, 0.3)], 1)])
    lengths = [64, 48]
    ref = [R.split(x[b, :n], TOP_DB, 16, 16, "spectral") for b, n in enumerate(lengths)]
    assert min(r[2] for r in ref) >= MARGIN and ref[0][0].tolist() == [[64, 64]]
    ns = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    kw = dict(top_db=TOP_DB, frame_length=16, hop_length=16)
    intervals, counts = gl.split(torch.from_numpy(x).cuda(), ns, **kw)
    index = gl.trim(torch.from_numpy(x).cuda(), ns, **kw).cpu().numpy()
    intervals, counts = intervals.cpu().numpy(), counts.cpu().numpy()
    for b, r in enumerate(ref):
        assert counts[b] == len(r[0]) and intervals[b, :counts[b]].tolist() == r[0].tolist()
        assert [intervals[b, 0, 0], intervals[b, counts[b] - 1, 1]] == index[b].tolist()
    assert index[0].tolist() == [64, 64]


# ---- remove_breath ----
# every row: RandomState(0); (n, [(lo, hi, level)]) over 1e-4 noise.  Row 0 is the one whose running mean matters: muting its
# second interval lowers the bar enough that the third stays (0.059 against 0.055), while a mean frozen at its first value (bar 0.067)
# would mute it.  Row 1: a breath between two loud bursts is muted; row 2: two loud bursts, nothing muted; row 3: one burst; row 4: n = 1.
MUTE_L = 2000
MUTE_ROWS = [(2000, [(0, 500, 0.45), (700, 1200, 0.06), (1400, 1900, 0.085)]),
             (1500, [(100, 600, 0.4), (800, 1100, 0.03), (1250, 1500, 0.4)]),
             (1200, [(0, 400, 0.3), (600, 1000, 0.2)]),
             (900, [(200, 700, 0.35)]),
             (1, [])]


@functools.lru_cache(maxsize=None)
def _mute_case():
    x = np.zeros((len(MUTE_ROWS), MUTE_L), np.float32)
    for b, (n, segs) in enumerate(MUTE_ROWS):
        x[b, :n] = R.pieces(n, segs, 0)
    ref = [R.remove_breath(x[b, :n]) for b, (n, _) in enumerate(MUTE_ROWS)]
    x.setflags(write=False)
    return x, ref


def _check_mute_case(x, ref):
    for b, (y, info) in enumerate(ref):
        print("row %d: restatement intervals %s muted %s, dB margin %.3f, decision margin %.4f" % (
            b, info["intervals"].tolist(), info["muted"].astype(int).tolist(), info["db_margin"], info["decision_margin"]))
        assert info["db_margin"] >= MARGIN and info["decision_margin"] >= DECISION_MARGIN, (b, info["db_margin"], info["decision_margin"])
    frozen = R.remove_breath(x[0, :MUTE_ROWS[0][0]], frozen_mean=True)[1]
    assert ref[0][1]["muted"].tolist() == [False, True, False] and frozen["muted"].tolist() == [False, True, True]      # the running total is load-bearing
    assert ref[1][1]["muted"].tolist() == [False, True, False] and not ref[2][1]["muted"].any() and len(ref[4][1]["intervals"]) == 0
    assert len(set(len(r[1]["intervals"]) for r in ref)) >= 3                                                        # ragged counts


def _compare_mute(out, ivs, counts, muted, mean, x, ref):
    worst = 0.0
    for b, (y, info) in enumerate(ref):
        n, k = MUTE_ROWS[b][0], len(info["intervals"])
        assert counts[b] == k and ivs[b, :k].tolist() == info["intervals"].tolist()
        assert muted[b, :k].tolist() == info["muted"].astype(int).tolist() and np.all(muted[b, k:] == 0)
        assert np.array_equal(out[b, :n].view(np.int32), y.astype(np.float32).view(np.int32)) and np.all(out[b, n:].view(np.int32) == 0)
        keep = np.ones(n, bool)
        for (lo, hi), m in zip(info["intervals"].tolist(), info["muted"]):
            if m:
                keep[lo:hi] = False
        assert np.array_equal(out[b, :n][keep].view(np.int32), x[b, :n][keep].view(np.int32)) and np.all(out[b, :n][~keep].view(np.int32) == 0)
        d = float(np.abs(mean[b, :1 + k] - info["abs_mean"]).max())
        worst = max(worst, d)
        print("row %d: device muted %s, max |abs_mean difference| %.3g" % (b, muted[b, :k].tolist(), d))
        assert d <= MEAN_BAR and np.all(mean[b, 1 + k:] == 0.0), (b, d)
    return worst


def test_breath_mute_equals_the_restatement(gl):
    import torch
    from taco_amd import _lib
    x, ref = _mute_case()
    _check_mute_case(x, ref)
    xn = np.array(x, copy=True)
    for b, (n, _) in enumerate(MUTE_ROWS):
        xn[b, n:] = np.nan
    w = torch.from_numpy(xn).cuda()
    ns = torch.tensor([n for n, _ in MUTE_ROWS], dtype=torch.int32, device="cuda")
    out, (ivs, counts, muted, mean) = gl.remove_breath(w, ns, return_info=True)
    assert tuple(out.shape) == (5, MUTE_L) and tuple(muted.shape) == (5, ivs.shape[1]) and tuple(mean.shape) == (5, 1 + ivs.shape[1])
    worst = _compare_mute(out.cpu().numpy(), ivs.cpu().numpy(), counts.cpu().numpy(), muted.cpu().numpy(), mean.cpu().numpy(), x, ref)
    print("largest |abs_mean difference| %.3g" % worst)
    # in place (d_out = d_wav), without the diagnostic outputs: the same rows
    inplace = w.clone()
    _lib.check(gl._lib.taco_wav_breath_mute(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(inplace.data_ptr()), C.c_void_p(ns.data_ptr()),
                                            5, MUTE_L, C.c_void_p(ivs.data_ptr()), C.c_void_p(counts.data_ptr()), ivs.shape[1], 0.05,
                                            C.c_void_p(inplace.data_ptr()), None, None))
    assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))


def test_breath_mute_walks_a_table_longer_than_one_batch(gl):
    """1100 hand-written intervals (the kernel holds 1024 sums at a time), through the library: 25 samples each, 5 apart, every third
    one quiet (0.01 against 0.4), the last one empty; the running total crosses the batch boundary."""
    import torch
    from taco_amd import _lib
    K, n = 1100, 1100 * 30
    rs = np.random.RandomState(7)
    x = (1e-4 * rs.randn(n + 50)).astype(np.float32)
    edges = np.array([[30 * k, 30 * k + 25] for k in range(K)], np.int32)
    edges[-1] = [n, n]
    for k, (lo, hi) in enumerate(edges.tolist()):
        x[lo:hi] = (0.01 if k % 3 == 1 else 0.4) * rs.randn(hi - lo)
    y, info = R.remove_breath(x[:n], edges=edges)
    print("restatement: %d of %d muted, decision margin %.4f" % (info["muted"].sum(), K, info["decision_margin"]))
    assert info["decision_margin"] >= DECISION_MARGIN and info["muted"][1::3][:-1].all() and not info["muted"][0::3].any() and not info["muted"][-1]
    xn = np.array(x, copy=True)
    xn[n:] = np.nan
    M = K + 3
    w = torch.from_numpy(xn.reshape(1, -1)).cuda()
    table = torch.zeros((1, M, 2), dtype=torch.int32, device="cuda")
    table[0, :K] = torch.from_numpy(edges).cuda()
    counts = torch.tensor([K], dtype=torch.int32, device="cuda")
    ns = torch.tensor([n], dtype=torch.int32, device="cuda")
    out = torch.empty_like(w)
    muted = torch.full((1, M), -7, dtype=torch.int32, device="cuda")
    mean = torch.full((1, 1 + M), -7.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(gl._lib.taco_wav_breath_mute(C.c_void_p(torch.cuda.current_stream().cuda_stream), p(w), p(ns), 1, n + 50, p(table), p(counts), M, 0.05,
                                            p(out), p(muted), p(mean)))
    out, muted, mean = out.cpu().numpy()[0], muted.cpu().numpy()[0], mean.cpu().numpy()[0]
    assert muted[:K].tolist() == info["muted"].astype(int).tolist() and np.all(muted[K:] == 0) and np.all(mean[1 + K:] == 0.0)
    assert np.array_equal(out[:n].view(np.int32), y.astype(np.float32).view(np.int32)) and np.all(out[n:].view(np.int32) == 0)
    assert np.isnan(mean[K]) and np.isnan(info["abs_mean"][K])                  # the empty interval: NumPy's mean of nothing
    d = float(np.abs(mean[:K] - info["abs_mean"][:K]).max())
    print("max |abs_mean difference| %.3g" % d)
    assert d <= MEAN_BAR


# ---- split_on_silence end to end ----
class _HP1600(object):
    sample_rate, num_freq, frame_length_ms, frame_shift_ms = 1600, 65, 50, 12.5


# 4800 samples at 1600 Hz, noise 1e-5, split at 64 / 8 and 60 dB: the second piece holds two quiet gaps (-50 dB) and a breath between loud
# parts, which the 40 dB split of remove_breath separates and mutes -- the second split then finds seven intervals where the first found six
E2E_SEGMENTS = [(100, 500, 0.3), (640, 760, 0.001), (760, 960, 0.03), (960, 1080, 0.001), (1080, 1400, 0.3), (1700, 1900, 0.3), (2200, 2700, 0.25),
                (2700, 2800, 0.001), (2800, 3000, 0.25), (3300, 3600, 0.3), (3900, 4500, 0.3)]
E2E_KW = dict(top_db=60, frame_length=64, hop_length=8, min_segment_length=0.2, max_segment_length=0.5)


def test_split_on_silence_end_to_end():
    import taco_amd
    x = R.pieces(4800, E2E_SEGMENTS, 4, noise=1e-5)
    ref = R.split_on_silence(x, 1600, **E2E_KW)
    print("restatement: first %s second %s kept %s, dB margin %.3f, decision margin %.4f" % (
        ref["first"].tolist(), ref["second"].tolist(), ref["kept"], ref["db_margin"], ref["decision_margin"]))
    assert ref["db_margin"] >= MARGIN and ref["decision_margin"] >= DECISION_MARGIN
    assert len(ref["first"]) == 6 and len(ref["second"]) == 7 and [k[0] for k in ref["kept"]] == [0, 2, 5, 6]      # too short: 1, 3; too long: 4
    no_breath, segments = taco_amd.split_on_silence(x, _HP1600(), pre_silence_length=0.01, post_silence_length=0.02, chunk_rows=4, **E2E_KW)
    assert no_breath.dtype == np.float32 and np.array_equal(no_breath.view(np.int32), ref["no_breath"].astype(np.float32).view(np.int32))
    assert [s[:3] for s in segments] == ref["kept"]
    for idx, start, end, seg in segments:
        assert len(seg) == 16 + (end - start) + 32 and not seg[:16].any() and not seg[len(seg) - 32:].any()
        assert np.array_equal(seg[16:len(seg) - 32], no_breath[start:end])
    dev = taco_amd.silence.SilenceDevice(_HP1600(), chunk_rows=4)
    assert [c[:2] for c in dev.chunks(ref["first"])] == [(0, 4), (4, 2)]                                             # the chunking ran
    dev.close()


def test_capture_and_replay_of_split_and_breath_mute(gl):
    import torch
    x, ref = _mute_case()
    w = torch.from_numpy(np.array(x)).cuda()
    ns = torch.tensor([n for n, _ in MUTE_ROWS], dtype=torch.int32, device="cuda")

    def chain():
        out, info = gl.remove_breath(w, ns, return_info=True)
        return (out,) + tuple(info)
    eager = [t.clone() for t in chain()]
    again = chain()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager, again))                    # two calls, the same bits
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = chain()
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager, captured))
    assert eager[3][0].tolist()[:3] == [0, 1, 0]
