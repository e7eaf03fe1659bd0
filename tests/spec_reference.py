"""Float64 restatement of the reference's waveform -> training-target functions (audio/__init__.py:48-51,64-67,142-147,155-156,161-162),
test infrastructure only: nothing in the product imports it.

  preemphasis      scipy.signal.lfilter([1, -k], [1], x), the call the reference itself makes
  stft             oracle/audio_oracle.py (librosa's documented convention; UNPINNED on librosa, see that file's header)
  amp_to_db        20 log10(max(1e-5, x));  normalize  clip((S - min_level_db) / -min_level_db, 0, 1)
  spectrogram      normalize(amp_to_db(|stft(preemphasis(y))|) - ref_level_db)           [num_freq, T]
  melspectrogram   normalize(amp_to_db(mel . |stft(preemphasis(y))|))                    [num_mels, T]   (no ref_level_db)
  mel_filters      librosa.filters.mel with its defaults, written DIFFERENTLY from the product's audio.mel_basis: one filter at a time,
                   scalar mel-scale conversions, the triangle as an explicit piecewise formula on the bin frequencies k * sr / n_fft.
                   UNPINNED on librosa as well; the two formulations check each other (tests/test_spec_host.py).
The librosa-free pieces are pinned on the reference's own recorded outputs (tests/golden/audio_vectors.npz: preemphasis, amp_to_db,
normalize)."""
import math

import numpy as np
import scipy.signal

import audio_oracle as A


def preemphasis(x, hp):
    return scipy.signal.lfilter([1, -hp.preemphasis], [1], x)


def amp_to_db(x):
    return 20 * np.log10(np.maximum(1e-5, x))


def normalize(S, hp):
    return np.clip((S - hp.min_level_db) / -hp.min_level_db, 0, 1)


def hz_to_mel(f):
    if f < 1000.0:
        return 3.0 * f / 200.0
    return 15.0 + 27.0 * math.log(f / 1000.0) / math.log(6.4)


def mel_to_hz(m):
    if m < 15.0:
        return 200.0 * m / 3.0
    return 1000.0 * math.exp(math.log(6.4) * (m - 15.0) / 27.0)


def mel_filters(sample_rate, n_fft, n_mels):
    top = hz_to_mel(sample_rate / 2.0)
    edges = [mel_to_hz(top * i / (n_mels + 1)) for i in range(n_mels + 2)]
    out = np.zeros((n_mels, n_fft // 2 + 1))
    for m in range(n_mels):
        left, centre, right = edges[m], edges[m + 1], edges[m + 2]
        for k in range(n_fft // 2 + 1):
            f = k * (sample_rate / 2.0) / (n_fft // 2)
            if left < f <= centre:
                out[m, k] = (f - left) / (centre - left)
            elif centre < f < right:
                out[m, k] = (right - f) / (right - centre)
        out[m] *= 2.0 / (right - left)
    return out


def magnitudes(y, hp):
    return np.abs(A.stft(preemphasis(np.asarray(y, np.float64), hp), hp))


def spectrogram(y, hp, D=None):
    D = magnitudes(y, hp) if D is None else D
    return normalize(amp_to_db(D) - hp.ref_level_db, hp)


def melspectrogram(y, hp, num_mels, D=None):
    D = magnitudes(y, hp) if D is None else D
    n_fft = hp.stft_parameters()[0]
    return normalize(amp_to_db(mel_filters(hp.sample_rate, n_fft, num_mels) @ D), hp)


def db_to_amp(x):
    return np.power(10.0, x * 0.05)


def linear_amplitude(S, hp):
    """Inverse of spectrogram's normalisation: the amplitude a normalised linear value stands for (floor and clip included)."""
    return db_to_amp(np.clip(S, 0, 1) * -hp.min_level_db + hp.min_level_db + hp.ref_level_db)


def mel_amplitude(S, hp):
    return db_to_amp(np.clip(S, 0, 1) * -hp.min_level_db + hp.min_level_db)


def test_signal(n, sample_rate, seed):
    """The accuracy tests' signal: a sine at sample_rate/110 Hz of amplitude 0.3 plus 0.1 N(0,1) noise; the first fifth scaled by 1e-4."""
    rs = np.random.RandomState(seed)
    t = np.arange(n)
    y = 0.3 * np.sin(2 * np.pi * t / 110.0) + 0.1 * rs.randn(n)
    y[:n // 5] *= 1e-4
    return y.astype(np.float32)
