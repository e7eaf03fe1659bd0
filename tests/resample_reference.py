"""NumPy float64 restatement of resampling to the model's sample rate (include/taco_abi.h, taco_resample_* / taco_wav_resample), the
yardstick of tests/test_resample_host.py and tests/test_gpu_resample.py.  It restates the documented algorithm of resampy.resample
(band-limited sinc interpolation with a Kaiser-windowed, linearly interpolated filter table) and librosa.core.resample's fix_length.
UNPINNED on resampy and librosa: neither is installed or imported here, nothing below was run against them.

Three pieces:
  resample_loop   the literal per-output loop over both wings, with the position of output t either accumulated as resampy 0.2.0
                  does (`time_register += 1/ratio`, a serial float64 sum) or exact (t*orig_sr/target_sr in integers: what the kernel does)
  bank / resample_bank   the polyphase evaluation with exact positions: one row of weights per phase r = (t*Q) mod P; also returns
                  A_t = sum |w_j| |x_j| per output, the scale every forward-error bound of a dot product is stated in
  librosa_resample   the wrapper: fix_length to ceil(len(x) * ratio) samples (at most one trailing zero), no rescaling"""
from math import gcd

import numpy as np

KAISER_BEST = dict(num_zeros=64, precision=9, beta=14.769656459379492, rolloff=0.9475937167399596)
SMALL = dict(num_zeros=4, precision=5, beta=6.0, rolloff=0.9)      # a small filter for the tests: 129 table entries


def sinc_window(num_zeros, precision, beta, rolloff):
    """The right half of the windowed sinc, num_zeros * 2^precision + 1 entries: rolloff * sinc(rolloff * i / num_table) * kaiser[n + i]."""
    num_table = 2 ** precision
    n = num_table * num_zeros
    return rolloff * np.sinc(rolloff * (np.arange(n + 1) / num_table)) * np.kaiser(2 * n + 1, beta)[n:], num_table


def setup(orig_sr, target_sr, half, num_table):
    ratio = float(target_sr) / orig_sr
    half = np.asarray(half, np.float64)
    win = half * ratio if ratio < 1 else half.copy()
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    g = gcd(orig_sr, target_sr)
    return dict(ratio=ratio, win=win, delta=delta, scale=scale, step=int(scale * num_table), nwin=len(win), num_table=num_table,
                P=target_sr // g, Q=orig_sr // g)


def _wing(s, frac):
    """-> (table indices of the wing's taps in order, eta)"""
    f = frac * s["num_table"]
    off = int(f)
    eta = f - off
    cnt = max(0, s["nwin"] - off) // s["step"]
    return off + s["step"] * np.arange(cnt), eta


def resample_loop(x, orig_sr, target_sr, half, num_table, positions="exact", detail=False):
    """-> (y [int(len(x) * ratio)], n [same]: the integer part of every output's position).  Taps are added one at a time in the
    reference's order: the left wing from x[n] backwards, then the right wing from x[n + 1] forwards.  detail=True: also
    [n_out, 4] = the table offset and the interpolation weight eta of the left and of the right wing."""
    assert positions in ("exact", "accumulate")
    s = setup(orig_sr, target_sr, half, num_table)
    x = np.asarray(x, np.float64)
    win, delta, scale, P, Q = s["win"], s["delta"], s["scale"], s["P"], s["Q"]
    n_out = int(len(x) * s["ratio"])
    y, ns, info = np.zeros(n_out), np.zeros(n_out, np.int64), np.zeros((n_out, 4))
    time_register, time_increment = 0.0, 1.0 / s["ratio"]
    for t in range(n_out):
        if positions == "accumulate":
            n = int(time_register)
            rem = time_register - n
        else:
            n, r = divmod(t * Q, P)
            rem = r / P
        frac = scale * rem
        idx, eta = _wing(s, frac)
        info[t, :2] = (idx[0] if len(idx) else -1), eta
        acc = 0.0
        for i in range(min(n + 1, len(idx))):
            acc += (win[idx[i]] + eta * delta[idx[i]]) * x[n - i]
        idx, eta = _wing(s, scale - frac)
        info[t, 2:] = (idx[0] if len(idx) else -1), eta
        for k in range(min(len(x) - n - 1, len(idx))):
            acc += (win[idx[k]] + eta * delta[idx[k]]) * x[n + k + 1]
        y[t], ns[t] = acc, n
        time_register += time_increment
    return (y, ns, info) if detail else (y, ns)


def bank(orig_sr, target_sr, half, num_table):
    """-> (bank float64 [P, LW + RW], LW): entry j of row r weighs x[n - (LW - 1) + j]; LW / RW are the most left / right taps any
    phase has, a phase with fewer has zeros at that end (the layout of taco_resample_bank)."""
    s = setup(orig_sr, target_sr, half, num_table)
    P, scale = s["P"], s["scale"]
    wings = []
    for r in range(P):
        frac = scale * (r / P)
        (li, le), (ri, re) = _wing(s, frac), _wing(s, scale - frac)
        wings.append((s["win"][li] + le * s["delta"][li], s["win"][ri] + re * s["delta"][ri]))
    LW, RW = max(len(a) for a, _ in wings), max(len(b) for _, b in wings)
    out = np.zeros((P, LW + RW))
    for r, (a, b) in enumerate(wings):
        out[r, LW - len(a):LW] = a[::-1]
        out[r, LW:LW + len(b)] = b
    return out, LW


def resample_bank(x, orig_sr, target_sr, half, num_table, weights=None):
    """Exact positions through the bank (`weights` = (bank, LW): e.g. the fp32-rounded bank; default the float64 one).
    -> (y [int(len(x) * ratio)], A [same]: sum over taps of |w_j| |x_j|)"""
    s = setup(orig_sr, target_sr, half, num_table)
    bk, LW = weights if weights is not None else bank(orig_sr, target_sr, half, num_table)
    bk = np.asarray(bk, np.float64)
    taps = bk.shape[1]
    x = np.asarray(x, np.float64)
    n_out = int(len(x) * s["ratio"])
    xp = np.concatenate([np.zeros(LW - 1), x, np.zeros(taps + 1)])      # xp[i] = x[i - (LW - 1)]
    y, A = np.zeros(n_out), np.zeros(n_out)
    for t0 in range(0, n_out, 1 << 16):                                  # in blocks: the gathered taps of a long recording do not fit memory
        tq = np.arange(t0, min(n_out, t0 + (1 << 16)), dtype=np.int64) * s["Q"]
        n, r = tq // s["P"], tq % s["P"]
        seg, w = xp[n[:, None] + np.arange(taps)[None, :]], bk[r]
        y[t0:t0 + len(tq)], A[t0:t0 + len(tq)] = (w * seg).sum(1), (np.abs(w) * np.abs(seg)).sum(1)
    return y, A


def out_len(n, orig_sr, target_sr):
    return int(np.ceil(n * (float(target_sr) / orig_sr)))


def computed_len(n, orig_sr, target_sr):
    return int(n * (float(target_sr) / orig_sr))


def librosa_resample(x, orig_sr, target_sr, half, num_table):
    """librosa.core.resample(x, orig_sr, target_sr, res_type='kaiser_best', fix=True, scale=False) with exact positions"""
    y = resample_bank(x, orig_sr, target_sr, half, num_table)[0]
    n = out_len(len(x), orig_sr, target_sr)
    return np.concatenate([y, np.zeros(n - len(y))])[:n]


def chirp_rows(L, lengths, seed=0):
    """[len(lengths), L] float64 at unit scale: a chirp from 0 to 0.45 cycles per sample plus noise in each row's first lengths[b]
    samples, zeros after."""
    rs = np.random.RandomState(seed)
    x = np.zeros((len(lengths), L))
    i = np.arange(L)
    for b, n in enumerate(lengths):
        x[b, :n] = (0.6 * np.sin(2 * np.pi * (0.225 / max(L, 1)) * i * i + b) + 0.3 * rs.randn(L))[:n]
    return x
