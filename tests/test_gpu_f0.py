"""Pitch tracking on the device (taco_f0_yin, taco_f0_path_stats: csrc/taco_f0.h) against the NumPy restatement tests/yin_reference.py:
bit equality with yin32 where fp32 is exact (the integer tier, at every width at which the kernel changes path), agreement with yin64 on
random data wherever the float64 decision margin clears a derived fp32 bound, the NaN / slack / null-output rules, determinism under graph
replay, the path statistics, and the Python surface (metrics.f0_track, f0_errors, prosody_distance).

THE BOUNDS of the random tier, u = 2^-24.  Inputs are fp32 and enter the restatement unchanged, so only the device's arithmetic differs.
(1) d'.  yin_reference.dprime_error_bound: d'_dev = d' (1 + e), |e| <= eps = gamma(2 W + 2 C + 12), C = ceil((tau_max + 2) / 64) -- sums of
    non-negative terms, so no cancellation; the derivation is in that function's docstring.
(2) decisions.  Every decision of step 4 compares a d'(tau) with the threshold or with another d'(tau'); both sides move by at most
    eps * max d' of the frame, so a frame whose float64 margin (yin64 returns it) is above 2 * eps * max d' decides the same way on the device.
    Frames below are left out of the lag / voicing equality; their share may not exceed 5 % (tests/test_f0_host.py holds the inputs to
    that with yin32 alone).
(3) aper = d'(tau*): |aper_dev - aper| <= eps * aper.
(4) f0 = sr / (tau* + delta), delta = clamp(0.5 (y0 - y2) / q), q = y0 - 2 y1 + y2.  With e' = eps + 4 u (the parabola's own roundings are
    relative to terms no larger than the y's): |d num| <= e' (y0 + y2) / 2, |d q| <= e' (y0 + 2 y1 + y2), so
    |d delta| <= (|d num| + |delta| |d q|) / (q - |d q|) when q > |d q|, and never more than 1 (delta is clamped to +-1/2 either way);
    the clamp is 1-Lipschitz.  Then |d f0| <= f0 (|d delta| / (tau* - 1/2) + 3 u).
Every test prints measured error / bound."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import yin_reference as R

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _lib():
    from taco_amd import _lib as L
    return L, L.load_library()


def _info():
    """(lanes of a wave, lags per thread block, j per register block, frames per workgroup, threads, largest frame, LDS floats) of k_yin"""
    out = (C.c_int * 7)()
    L, lib = _lib()
    L.check(lib.taco_debug_f0_info(out, 7))
    return tuple(out)


def _up(x, dtype=None):
    import torch
    return None if x is None else torch.as_tensor(np.array(x, dtype=dtype)).cuda()      # a copy: the shared inputs are read-only


def _call(wav, num, sample_rate, hop, window, fmin, fmax, threshold, plain=False, want_aper=True, want_lag=True):
    """taco_f0_yin (or the plain hook) on the current stream through the C ABI, on buffers of this call's own, pre-filled with -7 so that
    what the kernel leaves untouched shows -> dict of NumPy arrays"""
    import torch
    L, lib = _lib()
    x, dn = _up(wav, np.float32), _up(num, np.int32)
    B, Ls = x.shape
    F = 1 + Ls // hop
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    f0 = torch.full((B, F), -7.0, device="cuda")
    aper = torch.full((B, F), -7.0, device="cuda") if want_aper else None
    lag = torch.full((B, F), -7, dtype=torch.int32, device="cuda") if want_lag else None
    fn = lib.taco_debug_f0_yin_plain if plain else lib.taco_f0_yin
    L.check(fn(C.c_void_p(torch.cuda.current_stream().cuda_stream), P(x), P(dn), B, Ls, sample_rate, hop, window, fmin, fmax, threshold,
               P(f0), P(aper), P(lag)))
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in dict(f0=f0, aper=aper, lag=lag).items()}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- 1. the integer tier: bit equality with yin32 ----
@functools.lru_cache(maxsize=None)
def _integer_tier():
    """[(case, wav with NaN in the slack, kwargs, yin32's result)] -- computed once, read-only"""
    wave, LB, JC, FPW, NT, _, lds = _info()
    out = []
    for c in R.integer_cases(wave, LB, JC, FPW, NT, lds):
        assert c["exact_ok"], c
        x = R.integer_rows(c["B"], c["L"], c["seed"], c["period"], c["amp"])
        fmin, fmax = R.exact_lag_args(c["sample_rate"], c["tau_min"], c["tau_max"])
        kw = dict(sample_rate=c["sample_rate"], hop=c["hop"], window=c["window"], fmin=fmin, fmax=fmax, threshold=c["threshold"])
        ref = R.yin32(x, c["num"], **kw)
        if c["num"] is not None:
            for b, n in enumerate(c["num"]):
                x[b, n:] = np.nan                                                       # the slack holds NaN
        x.setflags(write=False)
        out.append((c, x, kw, ref))
    return out


def test_integer_tier_is_bit_equal_with_yin32():
    """Integer samples in [-amp, amp] with (2 amp)^2 * window * (tau_max + 1) <= 2^24: every d, S and d * tau is an integer up to 2^24, exact in fp32
    in any summation order, and d' is one correctly rounded division -- d_lag, d_aper and d_f0 equal yin32's on the bits.  Shapes: window
    and tau_max + 2 at the wave width and at the lag-block and j-block widths, each +-1; frame counts at the frames-per-workgroup span
    +-1; rows of n at hop multiples +-1, below the window, and 0, 1, 2; B of 1 and 3, ragged, NaN filling the slack; window 256 with
    tau_max 255; more lag blocks than threads; a hop too long for the full span; and a thread's part of the j range (what the register-blocked
    loop runs over: ceil(window / parts)) at the j-block width +-1 and twice it +-1 with one part, and at blocks plus a tail with 21, 4 and 5
    parts, the last part cut short -- asserted below from the kernel's own plan.  Columns past a row's frames are exact zeros."""
    L, lib = _lib()
    wave, LB, JC, FPW, NT, _, lds = _info()
    seen_short_span = seen_rounds = False
    seen_parts = set()                                  # (more than one j part?, register blocks in a part, length of its tail)
    voiced = unvoiced = 0
    for c, x, kw, ref in _integer_tier():
        plan = (C.c_int * 5)()
        L.check(lib.taco_debug_f0_plan(c["window"], c["tau_max"], c["hop"], plan))
        seen_short_span |= plan[3] < FPW
        seen_rounds |= plan[0] > NT
        last = c["window"] - (plan[1] - 1) * plan[2]    # the last part, cut short by the window
        seen_parts |= {(plan[1] > 1, jp // JC, jp % JC) for jp in {plan[2], last} if jp > 0}
        got = _call(x, c["num"], **kw)
        assert np.array_equal(got["lag"], ref["lag"]), (c, got["lag"], ref["lag"])
        assert np.array_equal(_bits(got["aper"]), _bits(ref["aper"])), c
        assert np.array_equal(_bits(got["f0"]), _bits(ref["f0"])), c
        for b in range(c["B"]):
            nf = int(ref["frames"][b])
            assert (got["f0"][b, nf:] == 0).all() and (got["aper"][b, nf:] == 0).all() and (got["lag"][b, nf:] == 0).all(), c
        voiced += int(ref["voiced"].sum())
        unvoiced += int(ref["frames"].sum() - ref["voiced"].sum())
    assert seen_short_span and seen_rounds and voiced > 100 and unvoiced > 100
    # the blocked loop's own edges, per part: the tail alone, whole blocks alone, and blocks followed by a tail, with one part and with several
    for several in (False, True):
        assert any(m == several and nb == 0 and tl > 0 for m, nb, tl in seen_parts), (several, sorted(seen_parts))
        assert any(m == several and nb >= 1 and tl == 0 for m, nb, tl in seen_parts), (several, sorted(seen_parts))
        assert any(m == several and nb >= 1 and tl > 0 for m, nb, tl in seen_parts), (several, sorted(seen_parts))
        assert any(m == several and nb >= 2 and tl > 0 for m, nb, tl in seen_parts), (several, sorted(seen_parts))
    assert {(False, 0, JC - 1), (False, 1, 0), (False, 1, 1), (False, 1, JC - 1), (False, 2, 1)} <= seen_parts      # JC - 1, JC, JC + 1, 2 JC - 1, 2 JC + 1
    print("integer tier: %d cases, %d voiced and %d unvoiced frames, all bit-equal" % (len(_integer_tier()), voiced, unvoiced))


def test_plain_variant_equals_the_blocked_kernel_on_the_bits():
    for c, x, kw, _ in _integer_tier():
        a, b = _call(x, c["num"], **kw), _call(x, c["num"], plain=True, **kw)
        for k in ("f0", "aper"):
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (c, k)
        assert np.array_equal(a["lag"], b["lag"]), c


# ---- 2. the random tier: against yin64 ----
@functools.lru_cache(maxsize=None)
def _random_tier(tier="8k"):
    wav, num, kw = R.RANDOM_TIERS[tier]()
    rows, eps = R.random_tier_margins(wav, num, kw)
    wav.setflags(write=False)
    return wav, num, kw, rows, eps


def _f0_bound(r, t, eps, sample_rate):
    """the bound (4) of the module docstring for frame t of a row's float64 result"""
    tau, dp = int(r["lag"][t]), r["dprime"][t]
    if not r["voiced"][t]:
        return 0.0
    y0, y1, y2 = dp[tau - 1], dp[tau], dp[tau + 1]
    q = y0 - 2 * y1 + y2
    e1 = eps + 4 * U
    dnum, dq = e1 * (y0 + y2) / 2, e1 * (y0 + 2 * y1 + y2)
    delta = min(max(0.5 * (y0 - y2) / q, -0.5), 0.5) if q > 0 else 0.0
    dd = min(1.0, (dnum + abs(delta) * dq) / (q - dq)) if q > dq else 1.0
    return float(r["f0"][t]) * (dd / (tau - 0.5) + 3 * U)


@pytest.mark.parametrize("tier", sorted(R.RANDOM_TIERS))
def test_random_tier_against_yin64(tier):
    """'8k': 3 rows x 61 frames at 8 kHz, fmin 60, fmax 400, window 200 (a thread's part of the j range is 13 values: the one-by-one loop).
    'model': 2 rows x 21 frames at the model's own framing, 24 kHz, window 1200, hop 300, fmin 60 (parts of 240 values: 15 register
    blocks each, so real-valued data passes through the blocked loop).  Harmonic sums with vibrato under an envelope, a noise stretch
    and a silent stretch per row.  Bounds (1) to (4) of the module docstring."""
    wav, num, kw, rows, eps = _random_tier(tier)
    L, lib = _lib()
    plan = (C.c_int * 5)()
    L.check(lib.taco_debug_f0_plan(kw["window"], R.lag_range(kw["sample_rate"], kw["fmin"], kw["fmax"])[1], kw["hop"], plan))
    assert (plan[2] >= 4 * _info()[2]) == (tier == "model")
    got = _call(wav, num, **kw)
    total = left = 0
    worst_aper = worst_f0 = 0.0
    for b, (r, need) in enumerate(rows):
        nf = len(r["f0"])
        keep = r["margin"] > need
        total, left = total + nf, left + int((~keep).sum())
        assert np.array_equal(got["lag"][b, :nf][keep], r["lag"][keep]), (b, np.nonzero(got["lag"][b, :nf] != r["lag"])[0])
        assert np.array_equal((got["f0"][b, :nf] > 0)[keep], r["voiced"][keep]), b
        assert (got["f0"][b, nf:] == 0).all() and (got["lag"][b, nf:] == 0).all()
        for t in np.nonzero(keep)[0]:
            ea, ba = abs(float(got["aper"][b, t]) - r["aper"][t]), eps * r["aper"][t] + U * r["aper"][t]      # + the final value's own storage rounding
            ef, bf = abs(float(got["f0"][b, t]) - r["f0"][t]), _f0_bound(r, t, eps, kw["sample_rate"])
            assert ea <= ba, (b, t, ea, ba)
            assert ef <= bf, (b, t, ef, bf)
            worst_aper = max(worst_aper, ea / ba)
            if bf > 0:
                worst_f0 = max(worst_f0, ef / bf)
    print("random tier %s: %d frames, %d left out (%.1f %%); worst aper error / bound %.4f, worst f0 error / bound %.4f"
          % (tier, total, left, 100.0 * left / total, worst_aper, worst_f0))
    assert left <= 0.05 * total


# ---- 3. NaN, infinities, slack, null outputs ----
def test_a_nan_gives_nan_for_exactly_the_frames_that_read_it_and_other_rows_keep_their_bits():
    wav, num, kw, rows, _ = _random_tier()
    base = _call(wav, num, **kw)
    tau_min, tau_max = R.lag_range(kw["sample_rate"], kw["fmin"], kw["fmax"])
    hop, W = kw["hop"], kw["window"]
    for (b, k, val) in ((1, 2345, np.nan), (0, 0, np.inf), (2, int(num[2]) - 1, -np.inf)):
        x = wav.copy()
        x[b, k] = val
        got = _call(x, num, **kw)
        nf = 1 + int(num[b]) // hop
        s0 = np.arange(nf) * hop - (W + tau_max) // 2
        reads = (s0 <= k) & (k <= s0 + W + tau_max)
        assert 1 <= reads.sum() < nf
        assert np.isnan(got["f0"][b, :nf][reads]).all() and np.isnan(got["aper"][b, :nf][reads]).all() and (got["lag"][b, :nf][reads] == -1).all()
        for name in ("f0", "aper"):
            assert np.array_equal(_bits(got[name][b, :nf][~reads]), _bits(base[name][b, :nf][~reads])), (b, k, name)
            others = [q for q in range(wav.shape[0]) if q != b]
            assert np.array_equal(_bits(got[name][others]), _bits(base[name][others])), (b, k, name)
        assert np.array_equal(got["lag"][b, :nf][~reads], base["lag"][b, :nf][~reads])
    slack = wav.copy()                                                                 # at and past n nothing is read
    for b in range(wav.shape[0]):
        slack[b, int(num[b]):] = np.nan
    got = _call(slack, num, **kw)
    for name in ("f0", "aper", "lag"):
        assert np.array_equal(got[name].view(np.uint32), base[name].view(np.uint32)), name


def test_null_optional_outputs():
    wav, num, kw, _, _ = _random_tier()
    base = _call(wav, num, **kw)
    for want_aper, want_lag in ((False, False), (True, False), (False, True)):
        got = _call(wav, num, want_aper=want_aper, want_lag=want_lag, **kw)
        assert np.array_equal(_bits(got["f0"]), _bits(base["f0"]))
        assert got["aper"] is None or np.array_equal(_bits(got["aper"]), _bits(base["aper"]))
        assert got["lag"] is None or np.array_equal(got["lag"], base["lag"])
    full = _call(wav, None, **kw)                                                      # NULL num_samples: full rows
    same = _call(wav, np.full(wav.shape[0], wav.shape[1]), **kw)
    assert np.array_equal(_bits(full["f0"]), _bits(same["f0"])) and np.array_equal(full["lag"], same["lag"])


# ---- 4. the Python surface: f0_track, repeat calls and graph replay ----
class _HP(object):
    """8 kHz, hop 100, frame 200, n_fft 256, 20 mel bands"""
    num_freq, sample_rate, frame_length_ms, frame_shift_ms = 129, 8000, 25.0, 12.5
    preemphasis, min_level_db, ref_level_db, power, griffin_lim_iters, num_mels = 0.97, -100, 20, 1.5, 10, 20


def test_f0_track_on_a_device_tensor_and_on_an_array():
    import torch
    from taco_amd import metrics
    wav, num, kw, _, _ = _random_tier()
    assert metrics.framing(_HP) == (kw["sample_rate"], kw["hop"], kw["window"])
    base = _call(wav, num, **kw)
    f0, aper, lag = metrics.f0_track(_up(wav), _up(num), _HP, fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"],
                                     return_aperiodicity=True, return_lag=True)
    assert f0.is_cuda and f0.dtype == torch.float32 and lag.dtype == torch.int32
    assert np.array_equal(_bits(f0.cpu().numpy()), _bits(base["f0"])) and np.array_equal(_bits(aper.cpu().numpy()), _bits(base["aper"]))
    assert np.array_equal(lag.cpu().numpy(), base["lag"])
    arr = metrics.f0_track(np.array(wav), np.array(num), _HP, fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"])
    assert arr.data_ptr() == f0.data_ptr() and np.array_equal(_bits(arr.cpu().numpy()), _bits(base["f0"]))      # the buffer set of the shape
    other = metrics.f0_track(_up(wav), _up(num), _HP, fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"], window=150).cpu().numpy()
    want = _call(wav, num, **dict(kw, window=150))["f0"]
    assert np.array_equal(_bits(other), _bits(want)) and not np.array_equal(_bits(other), _bits(base["f0"]))
    L, _ = _lib()
    with pytest.raises(L.TacoError):
        metrics.f0_track(_up(wav), _up(num), _HP, fmin=500.0, fmax=400.0)
    with pytest.raises(L.TacoError):
        metrics.f0_track(_up(wav[0]), None, _HP)


def test_second_call_and_graph_replay_give_the_same_bits():
    import torch
    from taco_amd import metrics
    wav, num, kw, _, _ = _random_tier()
    x, n = _up(wav), _up(num)
    rs = np.random.RandomState(5)
    B, F = wav.shape[0], 1 + wav.shape[1] // kw["hop"]
    fb = _up(np.where(rs.rand(B, F) < 0.3, 0.0, rs.uniform(80, 400, size=(B, F))), np.float32)
    path = _up(np.stack([np.arange(F), np.arange(F)], 1)[None].repeat(B, 0), np.int32)
    plen = _up(np.full(B, F), np.int32)

    def run():
        f0, aper, lag = metrics.f0_track(x, n, _HP, fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"], return_aperiodicity=True,
                                         return_lag=True)
        return f0, aper, lag, metrics.f0_path_stats(f0, fb, path, plen)

    first = [t.clone() for t in run()]
    outs = run()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                          # one stream, one chain of two launches
        captured = run()
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(captured, outs))           # the buffer set of the shape, not new memory
    for a, b in zip(first, captured):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 5. the path statistics ----
def _stats_call(fa, fb, path, plen):
    import torch
    L, lib = _lib()
    dfa, dfb, dp, dl = _up(fa, np.float32), _up(fb, np.float32), _up(path, np.int32), _up(plen, np.int32)
    out = torch.full((dfa.shape[0], 4), -7.0, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.taco_f0_path_stats(C.c_void_p(torch.cuda.current_stream().cuda_stream), P(dfa), dfa.shape[1], P(dfb), dfb.shape[1], P(dp), P(dl),
                                   dfa.shape[0], dp.shape[1], P(out)))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_stats(got, fa, fb, path, plen, what):
    """counts equal; the sum within: per entry c_dev = c + e_c, |e_c| <= 1200 * u / ln 2 (the rounded quotient shifts log2 by that) +
    5 u |c| (log2f to 2 ulp: 4 u of its value, and the product by 1200); the square adds 2 |c| e_c + e_c^2 + u c^2; the additions of the
    non-negative squares (a thread's strided run, then 8 tree levels) gamma(n + 8) of the sum."""
    ref = R.path_stats(np.asarray(fa, np.float32), np.asarray(fb, np.float32), path, plen)
    fa64, fb64 = np.asarray(fa, np.float32).astype(np.float64), np.asarray(fb, np.float32).astype(np.float64)
    for p in range(ref.shape[0]):
        assert got[p, 1:].tolist() == ref[p, 1:].tolist(), (what, p, got[p], ref[p])
        if np.isnan(ref[p, 0]):
            assert np.isnan(got[p, 0]), (what, p)
            continue
        n = int(min(max(int(plen[p]), 0), path.shape[1]))
        bound = 0.0
        for k in range(n):
            i, j = int(path[p, k, 0]), int(path[p, k, 1])
            if 0 <= i < fa64.shape[1] and 0 <= j < fb64.shape[1] and fa64[p, i] > 0 and fb64[p, j] > 0:
                c = abs(1200.0 * math.log2(fa64[p, i] / fb64[p, j]))
                ec = 1200.0 * U / math.log(2.0) + 5 * U * c
                bound += 2 * c * ec + ec * ec + U * c * c
        gam = (n + 8) * U
        bound += gam / (1 - gam) * ref[p, 0]
        err = abs(float(got[p, 0]) - ref[p, 0])
        print("%s pair %d: sum %.9g ref %.9g  error / bound %.4f" % (what, p, got[p, 0], ref[p, 0], err / bound if bound else 0.0))
        assert err <= bound, (what, p, err, bound)


def test_path_stats_against_the_restatement():
    import torch
    from taco_amd import metrics
    rs = np.random.RandomState(11)
    B, Fa, Fb, D = 3, 40, 50, 5
    track = lambda F: np.where(rs.rand(B, F) < 0.3, 0.0, rs.uniform(70, 420, size=(B, F))).astype(np.float32)
    fa, fb = track(Fa), track(Fb)
    # (a) a real taco_dtw_path output, ragged
    a, b = _up(rs.standard_normal((B, Fa, D)), np.float32), _up(rs.standard_normal((B, Fb, D)), np.float32)
    _, (path, plen) = metrics.dtw_distance(a, b, _up([Fa, 17, 1], np.int32), _up([33, Fb, 9], np.int32), cost="l2", return_path=True)
    path, plen = path.cpu().numpy().copy(), plen.cpu().numpy().copy()
    assert path.shape == (B, Fa + Fb - 1, 2) and (path[0, plen[0]:] == -1).all()
    _assert_stats(_stats_call(fa, fb, path, plen), fa, fb, path, plen, "dtw path")
    # the Python surface on the same path
    rmse, vuv, nv = metrics.f0_errors(_up(fa), _up(fb), _up(path), _up(plen))
    s = _stats_call(fa, fb, path, plen)
    want = R.errors_from_stats(s)
    for t, w in zip((rmse, vuv, nv), want):
        assert t.is_cuda and np.allclose(t.cpu().numpy(), w, rtol=4 * U, atol=0, equal_nan=True)
    # (b) out-of-range and -1 entries, a path_len beyond the rows and a negative one, more entries than threads
    cap = 700
    wild = rs.randint(-3, 60, size=(B, cap, 2)).astype(np.int32)
    wild[:, ::7] = -1
    wl = np.array([cap + 50, 300, -4], np.int32)
    got = _stats_call(fa, fb, wild, wl)
    _assert_stats(got, fa, fb, wild, wl, "wild path")
    assert got[2].tolist() == [0.0, 0.0, 0.0, 0.0] and 0 < got[0, 3] < cap
    # (c) a pair with no frame voiced on both sides, and a NaN in a track
    fa2, fb2 = fa.copy(), fb.copy()
    fa2[0] = 0.0
    fa2[1, int(path[1, 3, 0])] = np.nan
    got = _stats_call(fa2, fb2, path, plen)
    _assert_stats(got, fa2, fb2, path, plen, "unvoiced pair and NaN")
    assert got[0, 1] == 0 and got[0, 3] > 0 and np.isnan(got[1, 0]) and np.isfinite(got[2, 0])
    rmse, vuv, nv = metrics.f0_errors(_up(fa2), _up(fb2), _up(path), _up(plen))
    assert torch.isnan(rmse[0]) and float(vuv[0]) == float(np.float32(got[0, 2]) / np.float32(got[0, 3])) and float(nv[0]) == 0 and torch.isnan(rmse[1])


# ---- 6. prosody_distance ----
def test_prosody_distance_is_its_steps_composed_by_hand():
    import torch
    import taco_amd
    from taco_amd import metrics
    wav, num, kw, _, _ = _random_tier()
    a, na = _up(wav), _up(num)
    b, nb = _up(np.ascontiguousarray(wav[:, 400:5400])), _up(np.minimum(num - 400, 5000))       # each row against itself four frames later, cut short
    f0kw = dict(fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"])
    out = {k: v.clone() for k, v in metrics.prosody_distance(a, b, na, nb, _HP, **f0kw).items()}
    assert sorted(out) == ["f0_rmse_cents", "mcd", "voiced_frames", "vuv_error"] and all(v.is_cuda and tuple(v.shape) == (3,) for v in out.values())
    spec = taco_amd.Spectrogram(_HP, device="cuda")
    _, ma, fa_n = spec.targets(a, na)
    _, mb, fb_n = spec.targets(b, nb)
    dist, (path, plen) = metrics.dtw_distance(metrics.mel_cepstra(ma, _HP), metrics.mel_cepstra(mb, _HP), fa_n, fb_n, cost="l2", return_path=True)
    mcd = (dist * metrics.mcd_constant()).clone()
    fa = metrics.f0_track(a, na, _HP, **f0kw).clone()
    fb = metrics.f0_track(b, nb, _HP, **f0kw).clone()
    rmse, vuv, nv = metrics.f0_errors(fa, fb, path, plen)
    for k, w in (("mcd", mcd), ("f0_rmse_cents", rmse), ("vuv_error", vuv), ("voiced_frames", nv)):
        assert torch.equal(out[k].view(torch.int32), w.view(torch.int32)), k
    assert (out["mcd"] > 0).all() and (out["voiced_frames"] > 0).all()
    spec.close()
    L, _ = _lib()
    with pytest.raises(L.TacoError):                                                   # only f0_track's four settings pass through
        metrics.prosody_distance(a, b, na, nb, _HP, return_lag=True)
    # a waveform with itself: the diagonal path, every cost 0, every pair of F0 values equal
    same = metrics.prosody_distance(a, a, na, na, _HP, **f0kw)
    assert (same["mcd"] == 0).all() and (same["f0_rmse_cents"] == 0).all() and (same["vuv_error"] == 0).all() and (same["voiced_frames"] > 10).all()


def test_prosody_distance_of_a_copy_resampled_in_pitch():
    """A steady harmonic tone against itself resampled in pitch by 5/4 (yin_reference.pitch_pair): whatever the path, every pair of voiced
    frames is 1200 log2(4/5) = -386.31 cents apart up to YIN's interpolation error, so the RMSE lies within that error of 386.31.  Measured
    with yin64 on the CPU: the worst |cents - (-386.31)| over ALL pairs of voiced frames of the two tracks is 0.440 cents; allowed here is
    twice that, 0.88 cents (the device's own rounding, bound (4) of the module docstring, is four orders below)."""
    from taco_amd import metrics
    ratio = 1.25
    wa, wb = R.pitch_pair(ratio)
    kw = dict(sample_rate=8000, hop=100, window=200, fmin=60.0, fmax=400.0, threshold=0.1)
    ra, rb = R.yin64(wa, None, **kw), R.yin64(wb, None, **kw)
    fa, fb = ra["f0"][0][ra["voiced"][0]], rb["f0"][0][rb["voiced"][0]]
    want = 1200.0 * math.log2(1.0 / ratio)
    measured = float(np.abs(1200.0 * np.log2(fa[:, None] / fb[None, :]) - want).max())
    print("interpolation error measured with yin64: %.4f cents" % measured)
    assert measured <= 0.45
    out = metrics.prosody_distance(_up(wa), _up(wb), None, None, _HP, fmin=kw["fmin"], fmax=kw["fmax"], threshold=kw["threshold"])
    rmse, nv = float(out["f0_rmse_cents"][0]), float(out["voiced_frames"][0])
    print("f0_rmse_cents %.4f (1200 log2(5/4) = %.4f), voiced path entries %d, vuv_error %.4f, mcd %.3f dB"
          % (rmse, -want, nv, float(out["vuv_error"][0]), float(out["mcd"][0])))
    assert nv >= 30 and abs(rmse - abs(want)) <= 2 * 0.440
    assert float(out["mcd"][0]) > 0
