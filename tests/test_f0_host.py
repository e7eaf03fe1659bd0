"""Pitch tracking, the host side (CPU): the NumPy restatement tests/yin_reference.py on cases with known answers, yin32 against yin64 on
the integer inputs of the GPU test, the path statistics by hand, the C entry points with their prototypes and declarations, every argument
error of taco_f0_yin / taco_f0_path_stats -- all returned before the first device call, so they are reached here -- and the share of
frames the random tier of tests/test_gpu_f0.py may leave out."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import yin_reference as R
from taco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 1000


def _info():
    out = (C.c_int * 7)()
    assert _lib.load_library().taco_debug_f0_info(out, 7) == 0
    return list(out)


def _periodic(P, L, seed, half=0):
    """an integer sequence of period P; half: the weight of a component of period P / 2 added on top (the octave trap)"""
    rs = np.random.RandomState(seed)
    one = rs.randint(-8, 9, size=P).astype(np.float64)
    if half:
        h = rs.randint(-8, 9, size=P // 2).astype(np.float64)
        one = one + half * np.tile(h, 2)
    return np.tile(one, L // P + 1)[:L][None, :]


# ---- the restatement on known answers ----
@pytest.mark.parametrize("P", [7, 12, 25])
def test_a_periodic_integer_sequence_gives_its_period(P):
    """x[j] == x[j + P] for every j, so d(P) = 0 exactly and d'(P) = 0 < threshold; no smaller lag of the range has d = 0 because the
    sequence has no shorter period (checked).  Frames that lie wholly inside the row are taken: the zero padding of the ends breaks the
    period."""
    W, tau_min, tau_max, hop, L = 40, 3, 30, 10, 400
    x = _periodic(P, L, P)
    assert all((x[0, :L - k] != x[0, k:]).any() for k in range(1, P))
    fmin, fmax = R.exact_lag_args(SR, tau_min, tau_max)
    for yin in (R.yin64, R.yin32):
        r = yin(x, None, SR, hop, W, fmin, fmax, 0.1)
        inner = [t for t in range(r["frames"][0]) if t * hop - (W + tau_max) // 2 >= 0 and t * hop - (W + tau_max) // 2 + W + tau_max < L]
        assert len(inner) > 20
        for t in inner:
            assert r["lag"][0, t] == P and r["voiced"][0, t] and r["aper"][0, t] == 0
            assert SR / (P + 0.5) <= r["f0"][0, t] <= SR / (P - 0.5)


def test_silence_and_a_constant_row_are_unvoiced_with_dprime_one():
    W, tau_min, tau_max, hop, L = 32, 4, 20, 8, 200
    fmin, fmax = R.exact_lag_args(SR, tau_min, tau_max)
    x = np.zeros((2, L))
    x[1] = 5.0
    r = R.yin64(x, None, SR, hop, W, fmin, fmax, 0.1)
    assert not r["voiced"][0].any() and (r["aper"][0] == 1).all() and (r["f0"][0] == 0).all() and (r["lag"][0] == tau_min).all()
    s0 = lambda t: t * hop - (W + tau_max) // 2
    inner = [t for t in range(r["frames"][1]) if s0(t) >= 0 and s0(t) + W + tau_max < L]      # away from the zero padding the row IS constant
    assert len(inner) > 5 and not r["voiced"][1, inner].any() and (r["aper"][1, inner] == 1).all() and (r["lag"][1, inner] == tau_min).all()
    # threshold 1 is the largest allowed and d' = 1 is not below it
    assert not R.yin64(x[:1], None, SR, hop, W, fmin, fmax, 1.0)["voiced"].any()


def test_white_noise_is_unvoiced():
    W, tau_min, tau_max, hop, L = 200, 20, 134, 100, 4000
    x = np.random.RandomState(1).standard_normal((1, L))
    r = R.yin64(x, None, 8000, hop, W, 60.0, 400.0, 0.1)
    assert R.lag_range(8000, 60.0, 400.0) == (tau_min, tau_max)
    assert not r["voiced"].any() and (r["f0"] == 0).all() and (r["aper"] > 0.3).all()


def test_an_octave_trap_still_gives_the_period():
    """period P = 24 with a component of period 12 of the same strength on top: d'(12) dips to a quarter of the typical value, not below
    the threshold, and d'(24) = 0.  (A half-period component twice as strong takes d'(12) to 0.08: the definition then answers 12.)"""
    P, W, tau_min, tau_max, hop, L = 24, 60, 4, 40, 10, 500
    x = _periodic(P, L, 3, half=1)
    fmin, fmax = R.exact_lag_args(SR, tau_min, tau_max)
    row = R.yin_row64(x[0], L, SR, hop, W, fmin, fmax, 0.1)
    inner = [t for t in range(len(row["f0"])) if t * hop - (W + tau_max) // 2 >= 0 and t * hop - (W + tau_max) // 2 + W + tau_max < L]
    assert len(inner) > 20
    for t in inner:
        dp = row["dprime"][t]
        assert 0.1 <= dp[12] < 0.3 * np.median(dp[tau_min:tau_max + 1]) and dp[24] == 0          # the dip is there, and is not taken
        assert row["lag"][t] == P and row["voiced"][t]


def test_short_rows():
    """n = 0, n = 1, n < window, L < hop: one frame each (1 + n // hop), all of it or most of it padding"""
    W, tau_min, tau_max, hop = 16, 2, 10, 50
    fmin, fmax = R.exact_lag_args(SR, tau_min, tau_max)
    x = np.random.RandomState(2).randint(-8, 9, size=(3, 40)).astype(np.float64)      # L = 40 < hop
    x[1, 0] = 5.0
    for yin in (R.yin64, R.yin32):
        r = yin(x, [0, 1, 9], SR, hop, W, fmin, fmax, 0.1)
        assert R.num_columns(40, hop) == 1 and r["f0"].shape == (3, 1) and (r["frames"] == 1).all()
        assert r["lag"][0, 0] == tau_min and r["aper"][0, 0] == 1 and r["f0"][0, 0] == 0       # n = 0: silence
        assert np.isfinite(r["aper"]).all() and (r["lag"] >= tau_min).all() and (r["lag"] <= tau_max).all()
    # n = 1: the frame starts at s0 = -13 and reads x[0] at k = 13: d(tau) = 2 x0^2 for tau <= 13 (once as j = 13, once as j + tau = 13), so d' = tau / tau = 1
    one = R.yin_row64(x[1], 1, SR, hop, W, fmin, fmax, 0.1)
    assert x[1, 0] != 0 and np.allclose(one["dprime"][0][1:tau_max + 2], 1.0)
    # slack past n is never touched
    y = x.copy()
    y[2, 9:] = np.nan
    assert np.array_equal(R.yin64(y, [0, 1, 9], SR, hop, W, fmin, fmax, 0.1)["f0"], R.yin64(x, [0, 1, 9], SR, hop, W, fmin, fmax, 0.1)["f0"])
    bad = R.yin64(y, [0, 1, 10], SR, hop, W, fmin, fmax, 0.1)
    assert np.isnan(bad["f0"][2, 0]) and np.isnan(bad["aper"][2, 0]) and bad["lag"][2, 0] == -1 and np.isfinite(bad["f0"][:2]).all()


def test_yin32_equals_yin64_in_lag_and_voicing_on_the_integer_inputs():
    wave, LB, JC, FPW, NT, _, lds = _info()
    cases = R.integer_cases(wave, LB, JC, FPW, NT, lds)
    assert len(cases) > 25
    voiced = unvoiced = 0
    for c in cases:
        assert c["exact_ok"], c
        x = R.integer_rows(c["B"], c["L"], c["seed"], c["period"], c["amp"])
        fmin, fmax = R.exact_lag_args(c["sample_rate"], c["tau_min"], c["tau_max"])
        a = R.yin32(x, c["num"], c["sample_rate"], c["hop"], c["window"], fmin, fmax, c["threshold"])
        b = R.yin64(x, c["num"], c["sample_rate"], c["hop"], c["window"], fmin, fmax, c["threshold"])
        assert np.array_equal(a["lag"], b["lag"]) and np.array_equal(a["voiced"], b["voiced"]), c
        assert np.abs(a["aper"] - b["aper"]).max() <= 2.0 ** -24 * max(1.0, b["aper"].max())      # one correctly rounded division
        voiced += int(b["voiced"].sum())
        unvoiced += int((~b["voiced"]).sum())
    assert voiced > 100 and unvoiced > 100                                                        # thresholds are crossed both ways


# ---- the path statistics ----
def test_path_statistics_on_a_four_entry_path_by_hand():
    """f0_a = (100, 0, 200, 400), f0_b = (200, 0, 0); path (0,0) (1,1) (2,1) (3,2), then a -1 entry and one out of range, path_len 6.
    (0,0): both voiced, 1200 log2(100/200) = -1200 cents.  (1,1): both unvoiced: used, no error.  (2,1): one side voiced: a V/UV error.
    (3,2): one side voiced: a V/UV error.  The last two are skipped.  sum = 1200^2, both = 1, errors = 2, used = 4: rmse 1200, vuv 0.5."""
    fa, fb = np.array([[100.0, 0.0, 200.0, 400.0]]), np.array([[200.0, 0.0, 0.0]])
    path = np.array([[[0, 0], [1, 1], [2, 1], [3, 2], [-1, -1], [4, 0], [0, 0]]])
    s = R.path_stats(fa, fb, path, [6])
    assert s.tolist() == [[1200.0 ** 2, 1.0, 2.0, 4.0]]
    rmse, vuv, nv = R.errors_from_stats(s)
    assert rmse[0] == 1200.0 and vuv[0] == 0.5 and nv[0] == 1
    s7 = R.path_stats(fa, fb, path, [7])                                            # the seventh entry is (0,0) again
    assert s7.tolist() == [[2 * 1200.0 ** 2, 2.0, 2.0, 5.0]]
    assert R.path_stats(fa, fb, path, [99]).tolist() == s7.tolist() and R.path_stats(fa, fb, path, [-3])[0, 3] == 0      # clamped to the rows
    none = R.path_stats(np.zeros((1, 4)), fb, path, [4])                            # nothing voiced on both sides
    r2, v2, n2 = R.errors_from_stats(none)
    assert np.isnan(r2[0]) and v2[0] == 0.25 and n2[0] == 0
    fa_nan = fa.copy()
    fa_nan[0, 1] = np.nan
    sn = R.path_stats(fa_nan, fb, path, [6])
    assert np.isnan(sn[0, 0]) and sn[0, 1:].tolist() == [1.0, 2.0, 4.0]


# ---- the C ABI ----
def test_symbols_prototypes_and_declarations():
    lib = _lib.load_library()
    pub = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    dbg = open(os.path.join(ROOT, "include", "taco_debug.h")).read()
    for name, nargs, text in (("taco_f0_yin", 14, pub), ("taco_f0_path_stats", 10, pub), ("taco_debug_f0_yin_plain", 14, dbg),
                              ("taco_debug_f0_info", 2, dbg), ("taco_debug_f0_plan", 4, dbg)):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "taco_debug_f0" not in pub and "UNPINNED" in pub[pub.index("taco_f0_yin: the YIN"):]
    import taco_amd
    from taco_amd import metrics
    assert taco_amd.f0_track is metrics.f0_track and taco_amd.f0_errors is metrics.f0_errors and taco_amd.prosody_distance is metrics.prosody_distance
    for fn in (metrics.f0_track, metrics.f0_errors, metrics.prosody_distance):
        assert "this project's own definition, UNPINNED" in fn.__doc__.replace("This", "this")
    assert metrics.framing(taco_amd.hparams) == (24000, 300, 1200)


def test_the_kernel_widths_and_plans():
    lib = _lib.load_library()
    wave, LB, JC, FPW, NT, fmax_, lds = _info()
    assert wave == 64 and LB % 2 == 1 and NT % wave == 0 and FPW == NT // wave and lds * 4 <= 160 * 1024
    out = (C.c_int * 5)()
    assert lib.taco_debug_f0_plan(1200, 400, 300, out) == 0                           # the model's framing at fmin 60
    nblk, P, JP, fpw, used = list(out)
    assert nblk == -(-402 // LB) and P == NT // nblk and JP == -(-1200 // P) and fpw == FPW and used <= lds
    assert lib.taco_debug_f0_plan(16, 40, lds // 3 + 1, out) == 0 and 1 <= out[3] < FPW and out[4] <= lds      # a long hop: fewer frames share a span
    assert lib.taco_debug_f0_plan(1, fmax_ - 3, 1 << 30, out) == 0 and out[3] == 1 and out[4] <= lds          # the largest frame still fits
    assert lib.taco_debug_f0_plan(2, fmax_ - 3, 5, out) == _lib.TACO_ERR_ARG
    assert lib.taco_debug_f0_info(None, 7) == _lib.TACO_ERR_ARG and lib.taco_debug_f0_info((C.c_int * 7)(), -1) == _lib.TACO_ERR_ARG


def test_every_argument_error_is_returned_without_a_device():
    """The pointers are host arrays: a call that passed the checks would hand them to a kernel, so every call here must fail first."""
    lib = _lib.load_library()
    frame_max = _info()[5]
    B, L, hop, W = 2, 100, 10, 16
    F = 1 + L // hop
    wav, num = np.zeros((B, L), np.float32), np.zeros(B, np.int32)
    f0, aper, lag = np.zeros((B, F), np.float32), np.zeros((B, F), np.float32), np.zeros((B, F), np.int32)
    P = lambda x, off=0: None if x is None else C.c_void_p(x.ctypes.data + off)
    ARG, UNSUP = _lib.TACO_ERR_ARG, _lib.TACO_ERR_UNSUPPORTED

    for fn in (lib.taco_f0_yin, lib.taco_debug_f0_yin_plain):
        def call(**kw):
            v = dict(wav=P(wav), num=P(num), B=B, L=L, sr=1000, hop=hop, W=W, fmin=25.0, fmax=200.0, thr=0.1, f0=P(f0), aper=P(aper), lag=P(lag))
            v.update(kw)
            return fn(None, v["wav"], v["num"], v["B"], v["L"], v["sr"], v["hop"], v["W"], v["fmin"], v["fmax"], v["thr"], v["f0"], v["aper"], v["lag"])

        for kw in (dict(wav=None), dict(f0=None)):                                                                # null required pointer
            assert call(**kw) == ARG, kw
        for kw in (dict(B=0), dict(L=0), dict(hop=0), dict(W=0), dict(B=-1), dict(W=-5), dict(sr=0), dict(sr=-8000)):
            assert call(**kw) == ARG, kw
        for kw in (dict(fmin=0.0), dict(fmin=-1.0), dict(fmin=float("nan")), dict(fmax=25.0), dict(fmax=10.0), dict(fmax=float("nan")),
                   dict(fmax=501.0), dict(fmax=float("inf")),                                                     # tau_min = 1 and 0
                   dict(thr=0.0), dict(thr=-0.1), dict(thr=1.0001), dict(thr=float("nan"))):
            assert call(**kw) == ARG, kw
        overlaps = (dict(f0=P(wav)), dict(f0=P(wav, wav.nbytes - 4)), dict(f0=P(num, 4)), dict(aper=P(wav, 8)), dict(aper=P(num)),
                    dict(lag=P(wav, 400)), dict(lag=P(num, 4)),                                                   # output on input
                    dict(aper=P(f0)), dict(aper=P(f0, f0.nbytes - 4)), dict(lag=P(f0, 4)), dict(lag=P(aper, aper.nbytes - 4)))      # output on output
        for kw in overlaps:
            assert call(**kw) == ARG, kw
            assert b"overlap" in lib.taco_last_error()
        # a frame above the largest: window + tau_max + 2 > frame_max.  sr / fmin = 39.5 -> tau_max = 40
        fmin40 = 1000 / 39.5
        assert call(W=frame_max - 42 + 1, fmin=fmin40) == UNSUP and b"%d" % frame_max in lib.taco_last_error()
        assert call(W=10, fmin=1000.0 / (frame_max + 0.5), fmax=200.0) == UNSUP
        assert call(W=10, fmin=1e-30) == UNSUP                                                                    # a lag range beyond any int
        assert call(f0=None, W=frame_max, fmin=fmin40) == ARG                                                     # argument errors come first

    fa, fb = np.zeros((B, 7), np.float32), np.zeros((B, 9), np.float32)
    path, plen, stats = np.zeros((B, 15, 2), np.int32), np.zeros(B, np.int32), np.zeros((B, 4), np.float32)

    def scall(**kw):
        v = dict(fa=P(fa), Fa=7, fb=P(fb), Fb=9, path=P(path), plen=P(plen), B=B, cap=15, stats=P(stats))
        v.update(kw)
        return lib.taco_f0_path_stats(None, v["fa"], v["Fa"], v["fb"], v["Fb"], v["path"], v["plen"], v["B"], v["cap"], v["stats"])

    for kw in (dict(fa=None), dict(fb=None), dict(path=None), dict(plen=None), dict(stats=None), dict(Fa=0), dict(Fb=0), dict(B=0), dict(cap=0),
               dict(Fa=-1), dict(stats=P(fa)), dict(stats=P(fa, fa.nbytes - 4)), dict(stats=P(fb, 8)), dict(stats=P(path, path.nbytes - 4)),
               dict(stats=P(plen)), dict(stats=P(plen, 4))):
        assert scall(**kw) == ARG, kw
    for kw in (dict(stats=P(fa, 4)), dict(stats=P(fb, fb.nbytes - 4)), dict(stats=P(path)), dict(stats=P(plen, 4))):      # and says so
        assert scall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw


# ---- the share of frames the random tier may leave out ----


@pytest.mark.parametrize("tier", sorted(R.RANDOM_TIERS))
def test_the_random_tier_leaves_out_at_most_five_percent(tier):
    """On the inputs of the GPU test's random tiers: yin32 against yin64 alone, with the frames whose float64 margin is below the fp32 bound
    left out, agrees in lag and voicing on every kept frame, and the share left out stays within 5 % (the seeds were picked so: the 8 kHz
    tier, seed 3, leaves out 2 of 166 frames; the tier at the model's framing, seed 3, 1 of 40 -- its seeds 1 and 2 leave out 4 and 5)."""
    wav, num, kw = R.RANDOM_TIERS[tier]()
    rows, eps = R.random_tier_margins(wav, num, kw)
    a = R.yin32(wav, num, **kw)
    total = left = voiced = 0
    for b, (r, need) in enumerate(rows):
        nf = len(r["f0"])
        keep = r["margin"] > need
        total, left, voiced = total + nf, left + int((~keep).sum()), voiced + int(r["voiced"].sum())
        assert np.array_equal(a["lag"][b, :nf][keep], r["lag"][keep]) and np.array_equal(a["voiced"][b, :nf][keep], r["voiced"][keep]), b
    print("random tier %s: %d frames, %d voiced, %d left out (margin below 2 eps max d', eps = %.3g)" % (tier, total, voiced, left, eps))
    assert total >= 40 and 0.3 * total < voiced < 0.9 * total
    assert left <= 0.05 * total
