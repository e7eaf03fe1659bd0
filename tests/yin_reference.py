"""The definition of taco_f0_yin and taco_f0_path_stats (include/taco_abi.h) restated in NumPy, twice:

    yin64   float64 throughout.  It also returns each frame's decision margin: the smallest gap that would have to flip for the frame to
            choose another lag or another voicing -- |d'(tau) - threshold| over the lags the threshold search looked at,
            |d'(tau + 1) - d'(tau)| over the comparisons of the descent, and the argmin's lead over the runner-up when the frame is unvoiced.
            (A frame whose d() is 0 at every lag -- silence, a constant -- has d' = 1 set, not computed: only its threshold test can
            flip, and its margin is |1 - threshold|.)
    yin32   np.float32 with every operation rounded on its own, in the order the header states: difference, square, running sum over j
            ascending; S(tau) a running sum over tau ascending; product, then quotient; the parabola term by term.  (The kernel adds the
            square by one fmaf and sums in blocks: where every d, S and d * tau is an integer below 2^24 none of that rounds, and the
            two agree on the bits.  That is what the integer tier of tests/test_gpu_f0.py uses.)

and path_stats, the statistics of taco_f0_path_stats in float64.  This project's own definition, UNPINNED on any pitch-tracking package."""
import math

import numpy as np


def lag_range(sample_rate, fmin, fmax):
    """(tau_min, tau_max) = (floor(sr / fmax), ceil(sr / fmin)), formed in double from the fp32 values the C ABI receives"""
    return (int(math.floor(float(sample_rate) / float(np.float32(fmax)))), int(math.ceil(float(sample_rate) / float(np.float32(fmin)))))


def num_columns(L, hop):
    return 1 + L // hop


def _frame(x, n, t, hop, W, tau_max, dt):
    """x~[s0 .. s0 + W + tau_max] of frame t: x inside [0, n), 0 outside; nothing at or past n is touched"""
    s0 = t * hop - (W + tau_max) // 2
    k = np.arange(s0, s0 + W + tau_max + 1)
    seg = np.zeros(len(k), dt)
    ok = (k >= 0) & (k < n)
    seg[ok] = np.asarray(x)[k[ok]].astype(dt)
    return seg


def _dprime(seg, W, tau_max, dt):
    """(d'(0 .. tau_max + 1) of one frame in dtype dt, every operation rounded to dt; whether every d(tau) is 0: silence or a constant)"""
    NL = tau_max + 2
    j = np.arange(W)[None, :]
    tau = np.arange(NL)[:, None]
    diff = seg[j] - seg[j + tau]                       # [NL, W]
    sq = diff * diff
    d = np.cumsum(sq, axis=1, dtype=dt)[:, -1]         # a running sum over j ascending
    S = np.concatenate([np.zeros(1, dt), np.cumsum(d[1:], dtype=dt)])
    dp = np.ones(NL, dt)
    nz = S != 0
    nz[0] = False
    num = d * np.arange(NL).astype(dt)                 # the product, rounded
    dp[nz] = num[nz] / S[nz]                           # the quotient, rounded
    return dp, not d[1:].any()


def _choose(dp, tau_min, tau_max, thr):
    """(tau*, voiced, margin) by step 4; the margin in the dtype of dp, as a Python float"""
    rng = dp[tau_min:tau_max + 1]
    below = np.nonzero(rng < thr)[0]
    gaps = []
    if len(below):
        tau = tau_min + int(below[0])
        gaps.append(float(np.min(np.abs(dp[tau_min:tau + 1].astype(np.float64) - float(thr)))))
        while tau + 1 <= tau_max:
            gaps.append(abs(float(dp[tau + 1]) - float(dp[tau])))
            if not dp[tau + 1] < dp[tau]:
                break
            tau += 1
        return tau, True, min(gaps)
    k = int(np.argmin(rng))                            # the first of equal minima
    gaps.append(float(np.min(np.abs(rng.astype(np.float64) - float(thr)))))
    others = np.delete(rng, k).astype(np.float64)
    if len(others):
        gaps.append(float(np.min(others)) - float(rng[k]))
    return tau_min + k, False, min(gaps)


def _yin_row(x, n, sample_rate, hop, W, fmin, fmax, threshold, dt, want_dprime=False):
    tau_min, tau_max = lag_range(sample_rate, fmin, fmax)
    nf = 1 + n // hop
    f0, aper = np.zeros(nf, dt), np.zeros(nf, dt)
    lag, voiced, margin = np.zeros(nf, np.int32), np.zeros(nf, bool), np.full(nf, np.inf)
    dps = []
    thr = dt(np.float32(threshold))
    for t in range(nf):
        seg = _frame(x, n, t, hop, W, tau_max, dt)
        if not np.isfinite(seg).all():
            f0[t], aper[t], lag[t] = np.nan, np.nan, -1
            dps.append(None)
            continue
        dp, flat = _dprime(seg, W, tau_max, dt)
        tau, v, m = _choose(dp, tau_min, tau_max, thr)
        if flat:                                       # every d' is the constant 1, set and not computed: only the threshold test can flip
            m = abs(1.0 - float(thr))
        y0, y1, y2 = dp[tau - 1], dp[tau], dp[tau + 1]
        q = (y0 - dt(2) * y1) + y2
        delta = dt(0)
        if q > 0:
            delta = min(max((dt(0.5) * (y0 - y2)) / q, dt(-0.5)), dt(0.5))
        f0[t] = dt(sample_rate) / (dt(tau) + delta) if v else dt(0)
        aper[t], lag[t], voiced[t], margin[t] = y1, tau, v, m
        dps.append(dp)
    out = dict(f0=f0, aper=aper, lag=lag, voiced=voiced, margin=margin)
    if want_dprime:
        out["dprime"] = dps
    return out


def _batch(wav, num_samples, sample_rate, hop, window, fmin, fmax, threshold, dt):
    wav = np.asarray(wav)
    B, L = wav.shape
    F = num_columns(L, hop)
    out = dict(f0=np.zeros((B, F), dt), aper=np.zeros((B, F), dt), lag=np.zeros((B, F), np.int32), voiced=np.zeros((B, F), bool),
               margin=np.full((B, F), np.inf), frames=np.zeros(B, np.int32))
    for b in range(B):
        n = L if num_samples is None else int(min(max(int(num_samples[b]), 0), L))
        r = _yin_row(wav[b], n, sample_rate, hop, window, fmin, fmax, threshold, dt)
        nf = len(r["f0"])
        out["frames"][b] = nf
        for k in ("f0", "aper", "lag", "voiced", "margin"):
            out[k][b, :nf] = r[k]
    return out


def yin64(wav, num_samples, sample_rate, hop, window, fmin, fmax, threshold):
    """wav [B, L] -> dict of f0, aper [B, F] float64, lag [B, F] int32, voiced [B, F], margin [B, F] (inf where nothing was decided),
    frames [B]; columns past a row's own frames hold zeros"""
    return _batch(wav, num_samples, sample_rate, hop, window, fmin, fmax, threshold, np.float64)


def yin32(wav, num_samples, sample_rate, hop, window, fmin, fmax, threshold):
    """the same in np.float32, every operation rounded on its own"""
    return _batch(wav, num_samples, sample_rate, hop, window, fmin, fmax, threshold, np.float32)


def yin_row64(x, n, sample_rate, hop, window, fmin, fmax, threshold):
    """one row with its d'() per frame (a list of arrays, None for a frame that read a non-finite value)"""
    return _yin_row(x, n, sample_rate, hop, window, fmin, fmax, threshold, np.float64, want_dprime=True)


def path_stats(f0_a, f0_b, path, path_len):
    """f0_a [B, Fa], f0_b [B, Fb], path [B, cap, 2], path_len [B] -> [B, 4] float64: sum of squared cents, entries voiced on both sides,
    V/UV errors, entries used.  An entry outside the tracks is skipped; a NaN at a used entry makes the sum NaN."""
    f0_a, f0_b, path = np.asarray(f0_a, np.float64), np.asarray(f0_b, np.float64), np.asarray(path)
    B, cap = path.shape[0], path.shape[1]
    out = np.zeros((B, 4))
    for p in range(B):
        n = int(min(max(int(path_len[p]), 0), cap))
        bad = False
        for k in range(n):
            i, j = int(path[p, k, 0]), int(path[p, k, 1])
            if not (0 <= i < f0_a.shape[1] and 0 <= j < f0_b.shape[1]):
                continue
            a, b = f0_a[p, i], f0_b[p, j]
            out[p, 3] += 1
            if np.isnan(a) or np.isnan(b):
                bad = True
                continue
            if a > 0 and b > 0:
                c = 1200.0 * math.log2(a / b)
                out[p, 0] += c * c
                out[p, 1] += 1
            elif (a > 0) != (b > 0):
                out[p, 2] += 1
        if bad:
            out[p, 0] = np.nan
    return out


def errors_from_stats(stats):
    """(rmse_cents, vuv_error, voiced_frames) as metrics.f0_errors forms them: sqrt(sum / count), NaN where the count is 0; errors / used"""
    stats = np.asarray(stats, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.sqrt(stats[:, 0] / stats[:, 1]), stats[:, 2] / stats[:, 3], stats[:, 1]


# ---- the inputs the host test and the GPU test share ----
def exact_lag_args(sample_rate, tau_min, tau_max):
    """(fmin, fmax) that give exactly these lags: sr / fmin = tau_max - 1/2 and sr / fmax = tau_min + 1/2, far from a rounding edge"""
    fmin, fmax = sample_rate / (tau_max - 0.5), sample_rate / (tau_min + 0.5)
    assert lag_range(sample_rate, fmin, fmax) == (tau_min, tau_max)
    return fmin, fmax


def integer_rows(B, L, seed, period=None, amp=8):
    """B rows of integer samples in [-amp, amp]: row 0 a periodic sequence, row 1 the same kind plus integer noise of amplitude 1 to 3
    (clipped back into range), row 2 pure noise, then the three kinds again"""
    rs = np.random.RandomState(seed)
    x = np.zeros((B, L), np.float32)
    for b in range(B):
        P = period if period is not None else int(rs.randint(5, 30))
        base = np.tile(rs.randint(-amp, amp + 1, size=P), L // P + 1)[:L]
        if b % 3 == 0:
            row = base
        elif b % 3 == 1:
            a = int(rs.randint(1, 4))
            row = np.clip(base + rs.randint(-a, a + 1, size=L), -amp, amp)
        else:
            row = rs.randint(-amp, amp + 1, size=L)
        x[b] = row
    return x


def integer_cases(wave, LB, JC, FPW, NT, lds_floats):
    """The shapes of the integer tier from k_yin's own widths (taco_debug_f0_info): dicts of sample_rate, tau_min, tau_max, window, hop,
    L, num (None or a list per row), B, seed, threshold, amp (samples lie in [-amp, amp]).  Every case keeps d, S and d * tau integers up
    to 2^24: (2 amp)^2 * window * (tau_max + 1) <= 2^24 -- `exact_ok`, checked by the caller."""
    cases = []
    widths = sorted({w + s for w in (wave, LB, JC) for s in (-1, 0, 1)})
    seed = 0
    for W in widths:                                    # window at every width +-1, tau_max + 2 at a mid value
        seed += 1
        cases.append(dict(window=W, tau_min=3, tau_max=40, hop=7, L=160, B=1, num=None, seed=seed, threshold=0.2))
    for NL in widths:                                   # tau_max + 2 at every width +-1
        seed += 1
        cases.append(dict(window=50, tau_min=2, tau_max=NL - 2, hop=11, L=200, B=1, num=None, seed=seed, threshold=0.25))
    hop = 20
    for nfr in (FPW - 1, FPW, FPW + 1, 2 * FPW, 2 * FPW + 1):      # frame counts at the frames-per-workgroup span +-1
        seed += 1
        cases.append(dict(window=64, tau_min=4, tau_max=62, hop=hop, L=hop * (nfr - 1) + 3, B=1, num=None, seed=seed, threshold=0.15))
    # ragged rows: n at hop multiples +-1, below the window, and 0, 1, 2; B = 3, NaN slack is added by the caller
    L = 6 * hop + 5
    for nums in ([0, 1, 2], [hop - 1, hop, hop + 1], [3 * hop - 1, 3 * hop, 3 * hop + 1], [40, L, 6 * hop], [63, 5 * hop + 1, 7]):
        seed += 1
        cases.append(dict(window=64, tau_min=4, tau_max=62, hop=hop, L=L, B=3, num=nums, seed=seed, threshold=0.2))
    seed += 1                                           # the largest shape of the tier: window 256, tau_max 255
    cases.append(dict(window=256, tau_min=5, tau_max=255, hop=97, L=700, B=3, num=[700, 650, 389], seed=seed, threshold=0.3))
    seed += 1                                           # more lag blocks than threads (further rounds of the lag loop); window 16 keeps it exact
    cases.append(dict(window=16, tau_min=7, tau_max=LB * NT + 40, hop=900, L=3000, B=1, num=None, seed=seed, threshold=0.2, period=23))
    seed += 1                                           # a hop so long that FPW frames' span does not fit the LDS: fewer frames per workgroup
    cases.append(dict(window=16, tau_min=3, tau_max=40, hop=lds_floats // 3 + 1, L=2 * (lds_floats // 3 + 1) + 9, B=1, num=None, seed=seed,
                      threshold=0.2, period=9))
    # The register-blocked loop runs over a thread's PART of the j range, JP = ceil(window / P) values with P = NT // lag blocks (1 from
    # NT // 2 + 1 blocks on): what decides between full blocks of JC and the one-by-one tail is JP, not the window.  The cases above have
    # JP of 1 or 2 (the tail alone) but for the two large ones (whole blocks, no tail); these sit on either side of JC per part.
    many = LB * (NT // 2 + 1) - 2                       # tau_max with NT // 2 + 1 lag blocks: P = 1, JP = window
    for W in (JC - 1, JC, JC + 1, 2 * JC - 1, 2 * JC + 1):      # the tail alone, one block, a block and a tail of 1, of JC - 1, two and 1
        seed += 1
        cases.append(dict(window=W, tau_min=7, tau_max=many, hop=700, L=1500, B=1, num=None, seed=seed, threshold=0.2, period=23))
    P = NT // 12                                        # 12 lag blocks: P = 21 parts
    for W in (P * (JC + 4), P * (JC + 4) - 10):         # JP = JC + 4: a block and a tail of 4 in every part; then the last part cut to a tail
        seed += 1
        cases.append(dict(window=W, tau_min=7, tau_max=LB * 12 - 2, hop=150, L=700, B=3, num=[700, 451, 150], seed=seed, threshold=0.2, amp=4))
    seed += 1                                           # 64 lag blocks: 4 parts of 2 JC + 4, the last one 2 JC + 1
    cases.append(dict(window=4 * (2 * JC + 4) - 3, tau_min=7, tau_max=LB * 64 - 2, hop=200, L=900, B=1, num=None, seed=seed, threshold=0.2,
                      amp=4, period=29))
    seed += 1                                           # the model's lag count (tau_max 400: 45 blocks, 5 parts) at parts of 2 JC + 6, the last 2 JC + 4
    cases.append(dict(window=5 * (2 * JC + 6) - 2, tau_min=48, tau_max=400, hop=300, L=1300, B=2, num=[1300, 901], seed=seed, threshold=0.2,
                      amp=4, period=77))
    for c in cases:
        c.setdefault("period", None)
        c.setdefault("amp", 8)
        c["sample_rate"] = 1000
        # ((2 amp)^2 per term) * W terms * the largest tau (d * tau) or the number of lags (S)
        c["exact_ok"] = (2 * c["amp"]) ** 2 * c["window"] * (c["tau_max"] + 1) <= 2 ** 24
    return cases


def random_tier(seed=3):
    """3 rows x 61 frames at 8 kHz: harmonic sums with vibrato under an envelope, with a noise stretch and a silent stretch in each
    row; ragged lengths.  Returns (wav [3, 6000] float32, num_samples, kwargs of the call)."""
    rs = np.random.RandomState(seed)
    sr, L = 8000, 6000
    t = np.arange(L) / sr
    x = np.zeros((3, L))
    for b, f in enumerate((110.0, 173.0, 261.0)):
        ph = 2 * np.pi * np.cumsum(f * (1 + 0.03 * np.sin(2 * np.pi * 5.5 * t + b))) / sr
        amp = rs.uniform(0.3, 1.0, size=4)
        tone = sum(a * np.sin((k + 1) * ph + rs.uniform(0, 6.28)) for k, a in enumerate(amp))
        env = 0.4 + 0.6 * np.sin(np.pi * t / t[-1]) ** 2
        x[b] = env * tone * 0.2 + 0.003 * rs.standard_normal(L)
        a0 = 900 + 700 * b
        x[b, a0:a0 + 900] = 0.1 * rs.standard_normal(900)      # a noise stretch
        x[b, a0 + 1800:a0 + 2600] = 0.0                        # a silent stretch
    return x.astype(np.float32), np.array([6000, 5550, 4803], np.int32), dict(sample_rate=sr, hop=100, window=200, fmin=60.0, fmax=400.0,
                                                                               threshold=0.1)


def random_tier_model(seed=3):
    """2 rows x 21 frames at the model's own framing (24 kHz, hop 300, frame 1200, fmin 60: 402 lags, so a thread's part of the j range
    is 240 values = 15 register blocks): the same kind of signal as random_tier.  Returns (wav [2, 6000] float32, num_samples, kwargs)."""
    rs = np.random.RandomState(seed)
    sr, L = 24000, 6000
    t = np.arange(L) / sr
    x = np.zeros((2, L))
    for b, f in enumerate((131.0, 277.0)):
        ph = 2 * np.pi * np.cumsum(f * (1 + 0.03 * np.sin(2 * np.pi * 5.5 * t + b))) / sr
        amp = rs.uniform(0.3, 1.0, size=4)
        tone = sum(a * np.sin((k + 1) * ph + rs.uniform(0, 6.28)) for k, a in enumerate(amp))
        env = 0.4 + 0.6 * np.sin(np.pi * t / t[-1]) ** 2
        x[b] = env * tone * 0.2 + 0.003 * rs.standard_normal(L)
        a0 = 2400 + 900 * b
        x[b, a0:a0 + 900] = 0.1 * rs.standard_normal(900)      # a noise stretch
        x[b, a0 + 1500:a0 + 2400] = 0.0                        # a silent stretch
    return x.astype(np.float32), np.array([6000, 5403], np.int32), dict(sample_rate=sr, hop=300, window=1200, fmin=60.0, fmax=500.0,
                                                                        threshold=0.1)


RANDOM_TIERS = {"8k": random_tier, "model": random_tier_model}


def dprime_error_bound(window, n_lags):
    """Relative error of the device's d'(tau) against float64, u = 2^-24.  d(tau) is a sum of W non-negative terms, each a rounded
    difference squared (2 u) and then carried through at most W additions, one rounding each (a thread's run of j, then the parts): d_dev =
    d (1 + t1), |t1| <= gamma(W + 2).  S(tau) adds non-negative d(k): a term passes through at most C additions inside its lane, 6 levels
    of the wave scan and C more of the running sum, C = ceil(n_lags / 64): S_dev = S (1 + t2), |t2| <= gamma(W + 2 + 2 C + 6).  The product
    d * tau and the quotient add one rounding each.  Together (2 W + 2 C + 12) u to first order; gamma(k) = k u / (1 - k u) covers the rest."""
    k = 2 * window + 2 * -(-n_lags // 64) + 12
    u = 2.0 ** -24
    return k * u / (1 - k * u)


def random_tier_margins(wav, num, kw):
    """per row (the float64 result with d'() per frame, the bound a frame's margin has to clear): a decision compares d'(tau) with the
    threshold or with another d'; the device's d' is off by at most eps * d' (dprime_error_bound), so a gap above
    2 * eps * max d' of the frame cannot flip"""
    tau_min, tau_max = lag_range(kw["sample_rate"], kw["fmin"], kw["fmax"])
    eps = dprime_error_bound(kw["window"], tau_max + 2)
    rows = []
    for b in range(wav.shape[0]):
        r = yin_row64(wav[b], int(num[b]), kw["sample_rate"], kw["hop"], kw["window"], kw["fmin"], kw["fmax"], kw["threshold"])
        need = np.array([2 * eps * dp[tau_min - 1:tau_max + 2].max() for dp in r["dprime"]])
        rows.append((r, need))
    return rows, eps


def pitch_pair(ratio, sample_rate=8000, L=4000, f=140.0):
    """(a, b) float32 [1, L]: a steady harmonic tone of fundamental f under a slow envelope, and the same waveform resampled in pitch by
    `ratio` -- b(t) = a's tone at ratio * t, formed from the closed form, so nothing is interpolated -- under the same envelope"""
    t = np.arange(L) / sample_rate
    env = 0.5 + 0.5 * np.sin(np.pi * t / t[-1]) ** 2
    tone = lambda tt: sum(a * np.sin(2 * np.pi * (k + 1) * f * tt + p) for k, (a, p) in enumerate(((1.0, 0.3), (0.6, 1.1), (0.35, 2.0), (0.2, 0.7))))
    return (0.2 * env * tone(t)).astype(np.float32)[None, :], (0.2 * env * tone(ratio * t)).astype(np.float32)[None, :]
