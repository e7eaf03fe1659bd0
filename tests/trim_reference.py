"""Float64 restatement of `librosa.effects.trim` as the reference calls it (synthesizer.py:266-269: frame_length=5120, hop_length=256,
top_db=50, then `audio_out[:index[-1]]`), test infrastructure only: nothing in the product imports it.

UNPINNED on librosa.  The reference pins librosa==0.5.1; librosa is not a dependency of this project and is not available to its
tests, so this file restates the documented algorithm and could NOT be checked against librosa's source or output.  What it
restates, for `trim(y, top_db, ref=np.max, frame_length, hop_length)`:

  1. mse = rmse(y=y, n_fft=frame_length, hop_length=hop_length) ** 2.
     energy="spectral" (librosa 0.5.x, the pin): rmse goes through S = |stft(y, n_fft=frame_length, hop_length)| -- periodic Hann
       window of frame_length, center=True i.e. np.pad(y, frame_length // 2, mode="reflect"), 1 + n // hop_length frames -- and
       mse[t] = mean over the frame_length/2 + 1 one-sided bins of S[:, t] ** 2.  Not the time-domain mean square: DC and Nyquist
       count at full weight in the one-sided mean.
     energy="time" (librosa >= 0.6): mse[t] = mean of the squares of the same reflect-padded frame, no window.
  2. db = 10 log10(max(1e-10, mse)) - 10 log10(max(1e-10, max_t mse))   (logamplitude, ref_power=np.max, top_db=None);
     non_silent = db > -top_db.
  3. index = [first * hop_length, min(n, (last + 1) * hop_length)] over the non-silent frames, [0, 0] when there is none.

Written the LONG way on purpose -- np.pad, explicit frames, np.fft.rfft of the windowed frames, np.mean(|S|^2) -- so that it checks
the shortcut the kernel takes (`parseval_mse`, three windowed sums per frame and no transform).  A row of fewer than two samples
has nothing to reflect: it gets index [0, n] and no frames (include/taco_abi.h)."""
import numpy as np

ENERGIES = ("spectral", "time")


def hann_periodic(N):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)


def frames_of(y, frame_length, hop_length):
    """[1 + n // hop, frame_length]: the frames of the reflect-padded row (np.pad reflects as often as a short row needs)."""
    y = np.asarray(y, np.float64)
    n = len(y)
    yp = np.pad(y, frame_length // 2, mode="reflect")
    nf = 1 + n // hop_length
    return np.stack([yp[t * hop_length:t * hop_length + frame_length] for t in range(nf)])


def frame_mse(y, frame_length, hop_length, energy="spectral", drop_dc_nyquist=False):
    fr = frames_of(y, frame_length, hop_length)
    if energy == "time":
        return np.mean(fr ** 2, axis=1)
    assert energy == "spectral", energy
    S = np.abs(np.fft.rfft(fr * hann_periodic(frame_length)[None, :], axis=1))          # [nf, frame_length/2 + 1]
    if drop_dc_nyquist:          # a control only: what a formula that forgets the two unpaired bins would compute (N sum xw^2 / 2 / bins)
        S2 = S ** 2
        return (S2.sum(1) - 0.5 * S2[:, 0] - 0.5 * S2[:, -1]) / S.shape[1]
    return np.mean(S ** 2, axis=1)


def parseval_mse(y, frame_length, hop_length):
    """The kernel's form of the spectral energy: (N sum xw^2 + (sum xw)^2 + (sum (-1)^i xw)^2) / 2 / (N/2 + 1)."""
    N = frame_length
    xw = frames_of(y, N, hop_length) * hann_periodic(N)[None, :]
    alt = np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
    return (N * (xw ** 2).sum(1) + xw.sum(1) ** 2 + (xw * alt[None, :]).sum(1) ** 2) / 2.0 / (N // 2 + 1)


def trim(y, top_db=60, frame_length=2048, hop_length=512, energy="spectral", drop_dc_nyquist=False):
    """-> (index [2] int64, db [1 + n // hop] float64, margin: the smallest |db + top_db| over the frames, inf for no frames)."""
    y = np.asarray(y, np.float64)
    n = len(y)
    if n < 2:
        return np.array([0, n], np.int64), np.zeros(0), float("inf")
    mse = frame_mse(y, frame_length, hop_length, energy, drop_dc_nyquist)
    db = 10.0 * np.log10(np.maximum(1e-10, mse)) - 10.0 * np.log10(np.maximum(1e-10, mse.max()))
    nz = np.flatnonzero(db > -top_db)
    index = np.array([nz[0] * hop_length, min(n, (nz[-1] + 1) * hop_length)] if len(nz) else [0, 0], np.int64)
    return index, db, float(np.abs(db + top_db).min())


def burst_rows(L, lengths, bursts, seed, noise=1e-4, level=0.3, dc_row=None, dc=0.05):
    """The test signal: per row noise * randn over its own length with a louder burst level * randn on [lo, hi) of it (fractions of
    the row's length).  Row dc_row is built so that the DC and Nyquist terms of the one-sided sum decide its index: the offset dc
    sits on the middle half of its burst only (it raises the loudest frames, hence the reference level, by the DC term and leaves
    the frames at the edges alone), and the burst fades by 60 dB, linearly in dB, from the middle half out to its edges, so a
    change of the reference level moves the frame at which the threshold is crossed.  What lies past a row's length is left at
    zero.  float32 [B, L]."""
    rs = np.random.RandomState(seed)
    x = np.zeros((len(lengths), L), np.float32)
    for b, (n, (lo, hi)) in enumerate(zip(lengths, bursts)):
        row = noise * rs.randn(n)
        a, e = int(round(lo * n)), int(round(hi * n))
        burst = level * rs.randn(e - a)
        if b == dc_row:
            q = (e - a) // 4
            fade = np.concatenate([np.linspace(-60.0, 0.0, q, endpoint=False), np.zeros(e - a - 2 * q), np.linspace(0.0, -60.0, q + 1)[1:]])
            burst = burst * 10.0 ** (fade / 20.0)
            burst[q:e - a - q] += dc
        row[a:e] = burst
        x[b, :n] = row
    return x
