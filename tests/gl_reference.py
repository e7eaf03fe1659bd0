"""NumPy restatement of the stages of the librosa-flavour Griffin-Lim path, one at a time: test infrastructure only, nothing in the
product imports it.  tests/test_gpu_gl_stages.py holds the kernels to it through the taco_debug_gl_* hooks; tests/test_gl_stages_host.py
holds it to oracle/audio_oracle.py and shows that every MUTATION below is seen on the inputs the GPU tests use (the generators at the
end of this file are shared by both).

Every stage has a float64 form, and the stages whose kernels can be reproduced to the bit have a float32 form in the kernel's order of
operations (csrc/taco_audio.h):
  window sum     per position the covering frames from the last one down, then 1.0f / s, or 1 where s <= tiny
  overlap-add    the same order, then one multiplication by that reciprocal
  reflect pad    np.pad(mode="reflect") of the row's own L = hop * (frames - 1) samples
  pre-emphasis   out[n] = x[n] + a * out[n-1] as a plain loop (scipy.signal.lfilter([1], [1, -a], x)), and the kernel's scan over
                 1024 chunks of C = ceil(L / 1024) samples: a serial pass per chunk, the carries c[k+1] = ends[k] + a^C c[k], then
                 out[i] += a^(i - i0 + 1) c[k] with the factor formed by repeated multiplication
  PCM16          one correctly rounded division, one multiplication, truncation, clamp
A float32 form with a multiplication feeding an addition is bit-exact only where both are exact (the compiler may fuse them): the a = 0
and a = 1 tiers of the scan.

A mutation is a named mistake; a function that takes `mutation` computes the mistaken result when given its name."""
import numpy as np

import audio_oracle as A

U = 2.0 ** -24                                   # unit roundoff of float32
TINY = np.float32(1.17549435e-38)                # np.finfo(np.float32).tiny, librosa's threshold
PI2 = 6.283185307179586476925286766559

MUTATIONS = {
    "carry_from_wrong_chunk": "pre-emphasis: chunk k adds the carry of chunk k - 1",
    "power_c_minus_1": "pre-emphasis: a^(C-1) for a^C in the carry recurrence",
    "factor_starts_at_1": "pre-emphasis: the factor f starts at 1 instead of a",
    "reflect_one_off": "reflect padding one position off on each side (np.pad mode symmetric)",
    "wss_missing_last_frame": "window sum without the last frame it visits (the earliest one that covers the position)",
    "short_row_full_table": "a row with fewer than T frames divided by the window-sum table of T frames",
    "tiny_returns_0": "the tiny branch returns 0 instead of 1",
    "hermitian_2_at_dc_nyquist": "inverse matrix: weight 2 on the DC and Nyquist bins",
}
STAGE_MUTATIONS = {
    "preemphasis": ("carry_from_wrong_chunk", "power_c_minus_1", "factor_starts_at_1"),
    "overlap_add": ("reflect_one_off", "wss_missing_last_frame", "short_row_full_table", "tiny_returns_0"),
    "inverse_dft": ("hermitian_2_at_dc_nyquist",),
}

# name -> hparams, all at 1600 Hz: (n_fft, win, hop) = (128, 80, 20), (80, 80, 20), (128, 80, 30), (128, 80, 80), (2048, 1200, 300)
HANDLES = {
    "small": A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5),
    "win_is_nfft": A.AudioHParams(num_freq=41, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5),
    "hop30": A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=18.75),
    "hop_is_win": A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=50),
    "reference": A.AudioHParams(num_freq=1025, sample_rate=1600, frame_length_ms=750, frame_shift_ms=187.5),
}


class Geometry(object):
    """The integers of a handle (gl_create, gl_rows, gl_slot of csrc/taco_audio.h); tf: the flavour of taco_gl_create_tf"""

    def __init__(self, hp, tf=False):
        self.hp, self.tf = hp, tf
        self.n_fft, self.hop, self.win = hp.stft_parameters()
        self.F = hp.num_freq
        self.half = self.n_fft // 2
        self.lpad = 0 if tf else (self.n_fft - self.win) // 2
        self.fmin = 1 if tf else self.half // self.hop + 2
        self.tail = 2 * self.n_fft + self.win

    def rows(self, T):
        return T + -(-self.n_fft // self.hop)

    def slot(self, T):
        return self.rows(T) * self.hop

    def frames(self, f, T):
        return min(max(int(f), self.fmin), T)

    def samples(self, f):
        return self.hop * (f - 1) + (self.win if self.tf else 0)

    def info(self, T):
        """What taco_debug_gl_info reports"""
        return [self.rows(T), self.slot(T), self.half, self.lpad, self.tail, self.hop * (T - 1) + self.n_fft, self.fmin, self.samples(T)]


# ---- windows and the two DFT matrices, as gl_create builds them before its cast ----
def window64(win):
    return 0.5 - 0.5 * np.cos(PI2 * np.arange(win) / win)


def w2_32(geo):
    """The squared window the kernels read: float32 of the float64 square, win values (the padded table is zero outside them)"""
    w = window64(geo.win)
    return (w * w).astype(np.float32)


def dft_matrices(geo, mutation=None):
    """(forward [win, 2F], inverse [2F, win]) in float64: X_k = sum_n f[n] w[n] e^{-2 pi i k (n + lpad) / N} and its transpose with the
    irfft weights -- 1/N on DC and Nyquist, 2/N elsewhere, no imaginary part on DC and Nyquist -- with the angle reduced exactly"""
    N, F, W = geo.n_fft, geo.F, geo.win
    w = window64(W)
    k, n = np.arange(F)[:, None], np.arange(W)[None, :]
    ang = PI2 * ((k * (n + geo.lpad)) % N) / N
    c, s = np.cos(ang), np.sin(ang)
    fwd = np.concatenate([(w * c).T, (-w * s).T], axis=1)
    edge = ((k == 0) | (k == N // 2))
    ck = np.where(edge & (mutation != "hermitian_2_at_dc_nyquist"), 1.0, 2.0)
    inv = np.concatenate([ck / N * c * w, np.where(edge, 0.0, -ck / N * s * w)], axis=0)
    return fwd, inv


# ---- magnitude and initial phase ----
def magnitudes64(spec, hp):
    """gl_magnitude_of: (10^((clip(x,0,1) * -min_db + min_db + ref_db) / 20))^power"""
    return A.db_to_amp(A.denormalize(np.asarray(spec, np.float64), hp) + hp.ref_level_db) ** hp.power


def init_phase64(S, u):
    """[S cos 2 pi u | S sin 2 pi u] along the last axis"""
    S, u = np.asarray(S, np.float64), np.asarray(u, np.float64)
    return np.concatenate([S * np.cos(2 * np.pi * u), S * np.sin(2 * np.pi * u)], axis=-1)


# ---- window sum, overlap-add, reflect padding ----
def _covering_sum(rows, geo, f, dtype, skip_earliest=False):
    """acc[p] = sum over the frames t < f that cover padded position p of rows[t][p - t*hop - lpad], visited from the last frame down;
    rows [>= f, win], or one row of win values used for every frame"""
    Lp = geo.hop * (f - 1) + geo.n_fft
    acc = np.zeros(Lp, dtype)
    one = np.ndim(rows) == 1
    for t in range(f - 1, -1, -1):
        lo = t * geo.hop + geo.lpad
        seg = np.array(rows if one else rows[t], dtype)
        if skip_earliest:                          # the earliest frame that covers p is the last one the loop visits
            p = lo + np.arange(geo.win)
            seg[np.maximum(0, (p - geo.lpad - geo.win) // geo.hop + 1) == t] = 0
        acc[lo:lo + geo.win] += seg
    return acc


def wss_inv32(geo, f, mutation=None):
    """k_gl_wss for f frames: (1.0f / s where s > tiny else 1, the mask of the tiny branch), in padded coordinates"""
    s = _covering_sum(w2_32(geo), geo, f, np.float32, mutation == "wss_missing_last_frame")
    small = ~(s > TINY)
    with np.errstate(divide="ignore"):
        inv = np.where(small, np.float32(0.0 if mutation == "tiny_returns_0" else 1.0), np.float32(1.0) / s).astype(np.float32)
    return inv, small


def overlap_add32(Y, geo, T, frames, mutation=None):
    """k_gl_overlap_add on one utterance in float32, the kernel's order: Y [>= frames, win] -> (its slot of the padded rows [slot]: the
    row's own L samples from `half` on, their reflections on both sides, zeros after; the mask of its samples that took the tiny branch)"""
    f = geo.frames(frames, T)
    L = geo.hop * (f - 1)
    acc = _covering_sum(np.asarray(Y, np.float32), geo, f, np.float32)
    if f < T and mutation == "short_row_full_table":
        inv, small = wss_inv32(geo, T, mutation)
        inv, small = inv[:acc.size], small[:acc.size]
    else:
        inv, small = wss_inv32(geo, f, mutation)      # the row's own frames: what the kernel sums alongside, and the table at f = T
    y = (acc * inv)[geo.half:geo.half + L]
    out = np.zeros(geo.slot(T), np.float32)
    out[:L + geo.n_fft] = np.pad(y, geo.half, mode="symmetric" if mutation == "reflect_one_off" else "reflect")
    return out, small[geo.half:geo.half + L]


def overlap_add64(Y, geo, frames, w2=None):
    """istft's overlap-add and normalisation in float64 on f = frames frames: (y [L], bound [L]).  w2: the squared window, by default the
    float32 values the kernel reads (the same operands); window64(win)**2 gives oracle/audio_oracle.py's istft.
    bound: what float32 may differ by -- with n the most frames that cover a sample, at most n - 1 additions in each of the two sums, one
    division and one multiplication: 2n * 2^-24 * sum|Y| / s (first order, 1 % added for the rest)."""
    f = int(frames)
    w2 = w2_32(geo).astype(np.float64) if w2 is None else w2
    Y = np.asarray(Y, np.float64)
    acc, mag, s = _covering_sum(Y, geo, f, np.float64), _covering_sum(np.abs(Y), geo, f, np.float64), _covering_sum(w2, geo, f, np.float64)
    nz = s > float(TINY)
    inv = np.where(nz, 1.0 / np.where(nz, s, 1.0), 1.0)
    n = -(-geo.win // geo.hop)
    sl = slice(geo.half, geo.half + geo.hop * (f - 1))
    return (acc * inv)[sl], (1.01 * 2 * n * U * mag * inv)[sl]


def overlap_add_tf64(Y, geo, T, frames):
    """k_gl_overlap_add_tf: the plain sum from the start of the slot, zeros after hop*(f-1) + win; (slot [slot], sum|Y| [slot])"""
    f = min(max(int(frames), 1), T)
    Y = np.asarray(Y, np.float64)
    out, mag = np.zeros(geo.slot(T)), np.zeros(geo.slot(T))
    for t in range(f - 1, -1, -1):
        out[t * geo.hop:t * geo.hop + geo.win] += Y[t]
        mag[t * geo.hop:t * geo.hop + geo.win] += np.abs(Y[t])
    return out, mag


# ---- inverse pre-emphasis ----
def inv_preemphasis64(x, a):
    """scipy.signal.lfilter([1], [1, -a], x) as a plain loop in float64"""
    x = np.asarray(x, np.float64)
    out = np.empty_like(x)
    acc, a = 0.0, float(a)
    for i in range(x.size):
        acc = x[i] + a * acc
        out[i] = acc
    return out


def chunked_scan(x, a, L, Lb, dtype=np.float32, mutation=None):
    """k_inv_preemphasis on one row in `dtype` arithmetic: x [>= Lb] -> out [L], the first Lb samples filtered, zeros after.  1024 threads
    of C = ceil(L / 1024) samples each (C comes from the rectangle's L, not from the row's Lb)."""
    C = -(-L // 1024)
    a = dtype(a)
    xp = np.zeros(1024 * C, dtype)
    xp[:Lb] = np.asarray(x[:Lb], dtype)
    X = xp.reshape(1024, C)
    live = (np.arange(1024 * C) < Lb).reshape(1024, C)
    acc, loc = np.zeros(1024, dtype), np.zeros((1024, C), dtype)
    for j in range(C):
        acc = np.where(live[:, j], X[:, j] + a * acc, acc)
        loc[:, j] = acc
    aC = dtype(np.float64(a) ** (C - 1 if mutation == "power_c_minus_1" else C))          # powf
    carry, c = np.zeros(1024, dtype), dtype(0)
    for k in range(1024):
        carry[k] = c
        c = dtype(acc[k] + aC * c)
    if mutation == "carry_from_wrong_chunk":
        carry = np.concatenate([carry[:1], carry[:-1]])
    f = dtype(1) if mutation == "factor_starts_at_1" else a
    out = loc.copy()
    for j in range(C):
        out[:, j] = loc[:, j] + f * carry
        f = dtype(f * a)
    out = np.where(live, out, dtype(0)).reshape(-1)[:L]
    return out


def preemphasis_bound_units(a, L):
    """The float32 scan against the float64 loop, |error| <= units * 2^-24 * max|y| (y the exact output, u = 2^-24, Y = max|y|), in four parts.
    With C = ceil(L/1024), A = a^C, G = (1 - A) / (1 - a) = 1 + a + ... + a^(C-1):
      serial      inside a chunk l_n = fl(x_n + a l_(n-1)) is two roundings (one when fused) of a value that is a difference of two
                  outputs, |l| <= (1 + a) Y <= 2Y: err_n = a err_(n-1) + d_n, |d_n| <= 2u * 2Y, so |err| <= 4 G u Y
      carries     c_(k+1) = fl(ends_k + fl(A) c_k), the exact carries being outputs (|c| <= Y): the error obeys
                  e_(k+1) = A e_k + err(ends_k) + (fl(A) - A) c_k + two roundings, with powf held to 2 ulp (|fl(A) - A| <= 4uA; HIP documents 1 ulp):
                  |e| <= (4 G + 4 A + 2) u Y / (1 - A) = (4 / (1 - a) + (4 A + 2) / (1 - A)) u Y
      factor      f_j, the j-th factor, is a^j with j - 1 roundings: |f_j - a^j| <= 1.01 (j - 1) a^j u, times |c| <= Y: at most
                  1.01 * max_j (j - 1) a^j u Y over j = 1 .. C
      last line   out = fl(l + fl(f c)): the carry's error times f <= a, and two roundings of values below Y: 2 u Y
    The sum, 1 % added for the second-order terms."""
    a = float(a)
    C = -(-L // 1024)
    if a == 0.0:
        return 0.0
    A_ = a ** C
    G = (1 - A_) / (1 - a)
    j = np.arange(1, C + 1)
    carries = 4 / (1 - a) + (4 * A_ + 2) / (1 - A_)
    return 1.01 * (4 * G + a * carries + 1.01 * float(((j - 1) * a ** j).max()) + 2)


# ---- PCM16 ----
def pcm16_f32(x, n):
    """k_wav_to_pcm16 on one row in float32: scale = 32767.0f / max(0.01f, max|x[:n]|) (one correctly rounded division), then per sample
    one multiplication, truncation and the clamp to +-32767; zeros from n on"""
    x = np.asarray(x, np.float32)
    peak = np.abs(x[:n]).max() if n else np.float32(0)
    scale = np.float32(32767.0) / np.maximum(np.float32(0.01), np.float32(peak))
    out = np.zeros(x.size, np.int16)
    out[:n] = np.clip(np.trunc(x[:n] * scale), np.float32(-32767), np.float32(32767)).astype(np.int16)
    return out


# ---- the whole path at zero iterations, composed from the stages ----
def inv_spectrogram64(spec_FT, hp, init_uniform):
    """audio_oracle.inv_spectrogram(iters=0) from the stages above: magnitudes, initial phase, the inverse matrix, overlap-add with the
    float64 window, the loop.  spec_FT, init_uniform [num_freq, T]."""
    geo = Geometry(hp)
    X = init_phase64(magnitudes64(spec_FT.T, hp), init_uniform.T)            # [T, 2F]
    Y = X @ dft_matrices(geo)[1]                                             # [T, win]
    y, _ = overlap_add64(Y, geo, Y.shape[0], w2=window64(geo.win) ** 2)
    return inv_preemphasis64(y, hp.preemphasis)


# ---- the inputs of the GPU tests (shared with the mutation table of tests/test_gl_stages_host.py) ----
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# (handle, T): L = hop*(T-1) on both sides of the 256-thread block of k_gl_overlap_add and at two blocks (hop 20: 240, 260, 500, 520), and one
# shape per other handle
OVERLAP_ADD_CASES = [("small", 13), ("small", 14), ("small", 26), ("small", 27), ("win_is_nfft", 14), ("hop30", 14), ("hop_is_win", 5), ("reference", 7)]


def overlap_add_case(name, T, integers=True, tf=False):
    """(geo, frames [B], Y [B, Tr, win] float32): rows [T, T-1, fmin+1, fmin] and two whose counts lie outside [fmin, T]; every row of Y,
    those past a row's frames and the slot's tail rows included, holds data the kernel must not read.  integers: values in [-8, 8], so
    that every sum is exact."""
    geo = Geometry(HANDLES[name], tf)
    rs = np.random.RandomState(T * 7 + len(name))
    frames = np.array([T, T - 1, geo.fmin + 1, geo.fmin, geo.fmin - 2, T + 5], np.int32)
    shape = (frames.size, geo.rows(T), geo.win)
    Y = rs.randint(-8, 9, shape).astype(np.float32) if integers else rs.randn(*shape).astype(np.float32)
    return geo, _frozen(frames), _frozen(Y)


PREEMPHASIS_LENGTHS = [1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 3073, 153300]


def preemphasis_case(L, integers):
    """(fmin, frames [B], x [B, L] float32) for the hook at hop = 1 (T = L + 1): a full row, one that ends in the middle of a chunk, one that
    ends on a chunk boundary and one clamped to fmin (fmin - 1 samples); at 153 300 the first two only.  integers: values in [-8, 8],
    whose prefix sums stay below 2^24."""
    C = -(-L // 1024)
    T = L + 1
    fmin = min(4, T)
    mid = max(1, L // 2)
    if C > 1 and mid % C == 0:
        mid += 1
    edge = max(1, (L // C) // 3) * C
    frames = [T, mid + 1] if L > 100000 else [T, mid + 1, edge + 1, 0]
    rs = np.random.RandomState(L)
    x = rs.randint(-8, 9, (len(frames), L)).astype(np.float32) if integers else rs.randn(len(frames), L).astype(np.float32)
    return fmin, _frozen(np.array(frames, np.int32)), _frozen(x)


def prologue_case(name):
    """(geo, B, T, frames, spec [B, T, F], u [B, T, F]): spec in [-0.1, 1.1) with exact 0, 1 and values outside planted; a short row and one
    below fmin"""
    geo = Geometry(HANDLES[name])
    B, T = (3, 13) if name == "small" else (2, 6)
    rs = np.random.RandomState(len(name))
    spec = (rs.rand(B, T, geo.F) * 1.2 - 0.1).astype(np.float32)
    spec[0, 0, :6] = [0.0, 1.0, -3.0, 2.5, -0.0, 1.0000001]
    u = rs.rand(B, T, geo.F).astype(np.float32)
    frames = np.array([T, T - 3, 2][:B], np.int32)
    return geo, B, T, _frozen(frames), _frozen(spec), _frozen(u)


def dft_inverse_case(name):
    """X [M, 2F] float32 for the inverse product, M = B * Tr: random rows, a zero row, and unit rows at DC, Nyquist, their imaginary twins and
    one bin between -- a unit row reads one row of the matrix alone"""
    geo = Geometry(HANDLES[name])
    B, T = (3, 13) if name == "small" else (2, 24)
    M, F = B * geo.rows(T), geo.F
    X = np.random.RandomState(M).randn(M, 2 * F).astype(np.float32)
    X[5] = 0.0
    units = [0, F - 1, F, 2 * F - 1, F // 3, F + F // 3]
    for i, k in enumerate(units):
        X[7 + i] = 0.0
        X[7 + i, k] = 1.0
    return geo, _frozen(X), 5, {7 + i: k for i, k in enumerate(units)}
