"""Host side of resampling to the model's sample rate (taco_resample_*, taco_wav_resample, audio.Resampler): everything that needs no
GPU -- the Kaiser-windowed half filter, the restatement tests/resample_reference.py against itself (the literal loop and the polyphase
bank; exact positions against resampy 0.2.0's accumulated register), the library's lengths, argument errors and filter bank.
UNPINNED on resampy and librosa: nothing here runs either."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import resample_reference as R
from taco_amd import _lib, audio

SYMBOLS = ("taco_resample_create", "taco_resample_destroy", "taco_resample_out_len", "taco_resample_computed_len", "taco_resample_phases",
           "taco_resample_taps", "taco_resample_left_taps", "taco_resample_tile", "taco_resample_bank", "taco_wav_resample")
U = 2.0 ** -53      # unit roundoff of float64


def _create(orig_sr, target_sr, half, num_table):
    lib = _lib.load_library()
    h = C.c_void_p()
    half = np.ascontiguousarray(half, np.float64)
    rc = lib.taco_resample_create(orig_sr, target_sr, half.ctypes.data_as(C.c_void_p), len(half), num_table, 0, C.byref(h))
    return rc, h


def _dot_bound(taps, A):
    """Two float64 evaluations of one sum of `taps` products in different orders, each weight carrying the two roundings of win +
    eta*delta: each is within (taps + 3) u A of the exact sum (the forward-error bound of a dot product in any order, to first
    order), so they are within twice that of each other."""
    return 2 * (taps + 3) * U * A


def test_kaiser_window_shape_peak_and_zero_crossings():
    for name, f in audio.FILTERS.items():
        half = audio.kaiser_window(**f)
        num_table = 2 ** f["precision"]
        assert half.dtype == np.float64 and len(half) == f["num_zeros"] * num_table + 1
        assert half[0] == f["rolloff"]
        # sinc(rolloff * i / num_table) changes sign at i = k * num_table / rolloff, and the Kaiser taper is positive
        change = np.flatnonzero(np.sign(half[1:]) != np.sign(half[:-1])) + 1          # first index on the new side
        want = [int(np.ceil(k * num_table / f["rolloff"])) for k in range(1, int(f["num_zeros"] * f["rolloff"]) + 1)]
        assert change.tolist() == want, name
    assert np.array_equal(audio.kaiser_window(), R.sinc_window(**R.KAISER_BEST)[0])
    assert audio.FILTERS["kaiser_best"] == R.KAISER_BEST


@pytest.mark.parametrize("flt,so,sn,L", [(R.SMALL, 3, 2, 300), (R.SMALL, 2, 3, 200), (R.SMALL, 147, 80, 1200), (R.SMALL, 80, 147, 300),
                                         (R.SMALL, 1, 1, 100), (R.KAISER_BEST, 44100, 24000, 700), (R.KAISER_BEST, 16000, 24000, 300)])
def test_literal_loop_and_bank_agree(flt, so, sn, L):
    half, nt = R.sinc_window(**flt)
    x = R.chirp_rows(L, [L], 1)[0]
    y_loop, n_loop = R.resample_loop(x, so, sn, half, nt, "exact")
    y_bank, A = R.resample_bank(x, so, sn, half, nt)
    taps = R.bank(so, sn, half, nt)[0].shape[1]
    assert len(y_loop) == len(y_bank) == R.computed_len(L, so, sn) and len(y_loop) > 0
    ratio = np.abs(y_loop - y_bank) / _dot_bound(taps, A)
    print("loop vs bank %d -> %d: largest difference over its bound %.3f" % (so, sn, ratio.max()))
    assert ratio.max() <= 1.0
    full = R.librosa_resample(x, so, sn, half, nt)
    assert len(full) == R.out_len(L, so, sn) and np.array_equal(full[:len(y_bank)], y_bank) and not full[len(y_bank):].any()


@pytest.mark.parametrize("flt,so,sn,L,drifts", [(R.SMALL, 80, 147, 600, True), (R.SMALL, 147, 80, 1200, True), (R.KAISER_BEST, 44100, 24000, 1500, True),
                                                (R.SMALL, 3, 4, 300, False), (R.SMALL, 3, 2, 300, False)])
def test_accumulated_and_exact_positions_differ_only_where_the_phase_is_zero(flt, so, sn, L, drifts):
    """resampy 0.2.0's `time_register += 1/ratio` against t*Q/P.  A condition, not a tolerance: the two take a different n only at
    outputs with (t*Q) % P == 0 -- and do so there (6 of 9 such outputs at 147 -> 80 over 1200 samples).
    Values.  Where 1/ratio is a binary fraction (3 -> 4, 3 -> 2) the register is exact and the two agree at EVERY output to the
    float64 bound of test_literal_loop_and_bank_agree.  Where it is not, they cannot agree to that bound away from r == 0 either, and
    the premise that they would was checked and found wrong: the register carries its own rounding (~1e-12 of the position after
    1000 additions), which moves eta, and the values differ by up to 1.7e3 (147 -> 80), 2.7e4 (80 -> 147) and 1.5e2 (44100 -> 24000,
    kaiser_best) times that bound at outputs with r != 0.  What does hold there, and is asserted: wherever both evaluations sit in
    the same cell of the filter table (same offsets, so every weight is win + eta*delta with the same win and delta), the values
    differ by no more than |eta - eta'| sum |delta_j| |x_j| per wing -- the exact effect of the register's rounding on a
    piecewise-linear filter -- plus that float64 bound.  At r == 0 the values differ by what include/taco_abi.h documents: ~1e-11
    when up-sampling, up to 1.8e-2 here when down-sampling."""
    half, nt = R.sinc_window(**flt)
    s = R.setup(so, sn, half, nt)
    x = R.chirp_rows(L, [L], 1)[0]
    ye, ne, ie = R.resample_loop(x, so, sn, half, nt, "exact", detail=True)
    ya, na, ia = R.resample_loop(x, so, sn, half, nt, "accumulate", detail=True)
    bk, LW = R.bank(so, sn, half, nt)
    taps = bk.shape[1]
    A = R.resample_bank(x, so, sn, half, nt)[1]
    r = (np.arange(len(ye)) * s["Q"]) % s["P"]
    assert not (ne != na)[r != 0].any()                      # the condition
    assert ((ne != na).any() and Fraction(so, sn).denominator & (Fraction(so, sn).denominator - 1)) if drifts else np.array_equal(ne, na)
    bound = _dot_bound(taps, A)
    if not drifts:
        assert (np.abs(ye - ya) <= bound).all()
        return
    xp = np.concatenate([np.zeros(taps), x, np.zeros(taps + 1)])
    worst, checked = 0.0, 0
    for t in np.flatnonzero(r != 0):
        if ie[t, 0] != ia[t, 0] or ie[t, 2] != ia[t, 2]:
            continue                                          # a knot of the table lies between the two positions
        n = int(ne[t])
        li, _ = R._wing(s, s["scale"] * (int(r[t]) / s["P"]))
        ri, _ = R._wing(s, s["scale"] - s["scale"] * (int(r[t]) / s["P"]))
        sl = (np.abs(s["delta"][li]) * np.abs(xp[taps + n - np.arange(len(li))])).sum()
        sr = (np.abs(s["delta"][ri]) * np.abs(xp[taps + n + 1 + np.arange(len(ri))])).sum()
        lim = abs(ie[t, 1] - ia[t, 1]) * sl + abs(ie[t, 3] - ia[t, 3]) * sr + bound[t]
        worst, checked = max(worst, abs(ye[t] - ya[t]) / lim), checked + 1
    print("%d -> %d: %d outputs take another n (all at r == 0, of %d such); r != 0: %d outputs in the same table cell, largest "
          "difference over its limit %.3f, over the float64 bound alone %.1f; r == 0: largest difference %.3g" % (
              so, sn, int((ne != na).sum()), int((r == 0).sum()), checked, worst, (np.abs(ye - ya) / bound)[r != 0].max(), np.abs(ye - ya)[r == 0].max()))
    assert checked > 0.9 * (r != 0).sum() and worst <= 1.0


def test_library_exports_the_resample_entry_points():
    lib = _lib.load_library()
    for name in SYMBOLS:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    assert (_lib.TACO_WAV_F32, _lib.TACO_WAV_PCM16) == (0, 1)


@pytest.mark.parametrize("so,sn", [(44100, 24000), (3, 2)])
def test_lengths_are_the_float64_expressions_of_the_reference(so, sn):
    lib = _lib.load_library()
    half, nt = R.sinc_window(**R.SMALL)
    rc, h = _create(so, sn, half, nt)
    assert rc == 0
    ratio = float(sn) / so
    for n in (0, 1, 146, 147, 148, 441, 10 ** 7 + 1):
        assert lib.taco_resample_out_len(h, n) == int(np.ceil(n * ratio)) == R.out_len(n, so, sn)
        assert lib.taco_resample_computed_len(h, n) == int(n * ratio) == R.computed_len(n, so, sn)
    assert lib.taco_resample_phases(h) == R.setup(so, sn, half, nt)["P"] and lib.taco_resample_tile(h) >= 256
    lib.taco_resample_destroy(h)


def test_argument_errors_return_before_any_device_call():
    lib = _lib.load_library()
    half, nt = R.sinc_window(**R.SMALL)
    err = lambda: lib.taco_last_error()

    def create(so=3, sn=2, hw=half, n=None, table=nt, out=True):
        h = C.c_void_p()
        hw_p = None if hw is None else np.ascontiguousarray(hw, np.float64).ctypes.data_as(C.c_void_p)
        rc = lib.taco_resample_create(so, sn, hw_p, len(half) if n is None else n, table, 0, C.byref(h) if out else None)
        if rc == 0:
            lib.taco_resample_destroy(h)
        return rc

    assert create() == 0
    assert create(so=0) == _lib.TACO_ERR_ARG and b"sample rates" in err()
    assert create(sn=-5) == _lib.TACO_ERR_ARG and b"sample rates" in err()
    assert create(table=0) == _lib.TACO_ERR_ARG and b"num_table" in err()
    assert create(n=1) == _lib.TACO_ERR_ARG and b"n_window" in err()
    assert create(hw=None) == _lib.TACO_ERR_ARG and create(out=False) == _lib.TACO_ERR_ARG
    assert create(so=100, sn=1, table=32) == _lib.TACO_ERR_ARG and b"int(scale*num_table) = 0" in err()
    big, big_table = R.sinc_window(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
    assert lib.taco_resample_create(100003, 100019, big.ctypes.data_as(C.c_void_p), len(big), big_table, 0, C.byref(C.c_void_p())) == _lib.TACO_ERR_ARG
    assert b"filter bank too large" in err()
    # every pair of the common rates fits with kaiser_best
    rates = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
    most = 0
    for so in rates:
        for sn in rates:
            rc, h = _create(so, sn, big, big_table)
            assert rc == 0, (so, sn, err())
            most = max(most, lib.taco_resample_phases(h) * lib.taco_resample_taps(h))
            lib.taco_resample_destroy(h)
    assert most <= 1 << 22

    rc, h = _create(3, 2, half, nt)
    d = C.c_void_p(4096)      # a dummy non-null address stands in for device memory: validation rejects each call before it is touched

    def run(r=h, x=d, fmt=_lib.TACO_WAV_F32, ch=1, B=2, L=300, out=d, L_out=200):
        return lib.taco_wav_resample(r, None, x, fmt, ch, None, B, L, out, L_out, None)

    assert run(r=None) == _lib.TACO_ERR_ARG and run(x=None) == _lib.TACO_ERR_ARG and run(out=None) == _lib.TACO_ERR_ARG
    assert run(B=0) == _lib.TACO_ERR_ARG and run(L=0) == _lib.TACO_ERR_ARG and run(B=65536) == _lib.TACO_ERR_ARG
    assert run(fmt=2) == _lib.TACO_ERR_ARG and b"input format" in err()
    assert run(ch=0) == _lib.TACO_ERR_ARG and b"channels" in err()
    assert run(L_out=199) == _lib.TACO_ERR_ARG and b"L_out = 199" in err()
    lib.taco_resample_destroy(h)


@pytest.mark.parametrize("flt,so,sn", [(R.SMALL, 3, 2), (R.SMALL, 2, 3), (R.SMALL, 147, 80), (R.SMALL, 1, 1), (R.KAISER_BEST, 44100, 24000)])
def test_the_library_bank_is_the_float32_of_the_restatement_bit_for_bit(flt, so, sn):
    lib = _lib.load_library()
    half, nt = R.sinc_window(**flt)
    rc, h = _create(so, sn, half, nt)
    assert rc == 0
    ref, LW = R.bank(so, sn, half, nt)
    P, taps = lib.taco_resample_phases(h), lib.taco_resample_taps(h)
    assert (P, taps) == ref.shape and lib.taco_resample_left_taps(h) == LW
    got = np.empty((P, taps), np.float32)
    assert lib.taco_resample_bank(h, got.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
    lib.taco_resample_destroy(h)
