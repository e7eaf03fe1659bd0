"""NumPy float64 restatements of the reference's two other vocoders, the yardsticks of tests/test_gpu_vocoder.py: test infrastructure
only, nothing in the product imports it.

inv_spectrogram_tensorflow (audio/__init__.py:59-61,87-96,109-116): tf.contrib.signal.stft / inverse_stft of TF 1.x restated from their
documented algorithm -- UNPINNED on TensorFlow, which is not installed here.  Written on explicitly framed and zero-padded arrays with
np.fft.rfft / irfft, not with the DFT matrices the kernels multiply by:
  stft(y, pad_end=False)  frame t = y[t*hop : t*hop + win] for t = 0 .. (len - win) // hop, times the periodic Hann window of win,
                          zero-padded at the END to n_fft, rfft
  inverse_stft(X)         irfft(X, n_fft)[:win] times the same window, overlap-added at stride hop; no division by the window
                          sum-square, no padding removed: hop*(T - 1) + win samples
inv_melspectrogram (audio/__init__.py:70-72,136-140) composes oracle/audio_oracle.py's griffin_lim / inv_preemphasis (librosa semantics,
UNPINNED on librosa as that file says)."""
import numpy as np

import audio_oracle as A


def hann(win):
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(win) / win)


def tf_stft(y, hp):
    """y [len] -> [T, n_fft/2 + 1] complex, T = 1 + (len - win) // hop (0 frames when len < win)"""
    n_fft, hop, win = hp.stft_parameters()
    y = np.asarray(y, np.float64)
    T = 1 + (len(y) - win) // hop if len(y) >= win else 0
    frames = np.zeros((T, n_fft))
    w = hann(win)
    for t in range(T):
        frames[t, :win] = y[t * hop:t * hop + win] * w
    return np.fft.rfft(frames, axis=1)


def tf_istft(X, hp):
    """X [T, n_fft/2 + 1] complex -> [hop*(T-1) + win]"""
    n_fft, hop, win = hp.stft_parameters()
    T = X.shape[0]
    w = hann(win)
    y = np.zeros(hop * (T - 1) + win)
    for t in range(T):
        y[t * hop:t * hop + win] += np.fft.irfft(X[t], n_fft)[:win] * w
    return y


def tf_magnitudes(spec_TF, hp):
    return A.db_to_amp(A.denormalize(np.asarray(spec_TF, np.float64), hp) + hp.ref_level_db) ** hp.power


def inv_spectrogram_tensorflow(spec_TF, hp, iters=None, return_min_est=False):
    """spec_TF [T, num_freq] (the model's layout, as the reference's graph takes linear_outputs) -> [hop*(T-1) + win].  With
    return_min_est also the smallest |est| met in any iteration (inf with none): how far every bin stayed from the 1e-8 branch."""
    S = tf_magnitudes(spec_TF, hp)
    y = tf_istft(S.astype(np.complex128), hp)
    lo = np.inf
    for _ in range(hp.griffin_lim_iters if iters is None else iters):
        est = tf_stft(y, hp)
        mag = np.abs(est)
        lo = min(lo, float(mag.min()))
        y = tf_istft(S * (est / np.maximum(1e-8, mag)), hp)
    return (y, lo) if return_min_est else y


def mel_amplitudes(mel_TM, hp):
    """_db_to_amp(_denormalize(mel)): no ref_level_db (melspectrogram never subtracts it)"""
    return A.db_to_amp(A.denormalize(np.asarray(mel_TM, np.float64), hp))


def mel_to_linear(mel_TM, inv_FM, hp):
    """mel_TM [T, num_mels], inv_FM [num_freq, num_mels] -> [T, num_freq] = max(1e-10, inv . amp) per frame"""
    return np.maximum(1e-10, mel_amplitudes(mel_TM, hp) @ np.asarray(inv_FM, np.float64).T)


def inv_melspectrogram(mel_TM, inv_FM, hp, init_uniform_TF, iters=None):
    """audio/__init__.py:70-72: mel_TM [T, num_mels], init_uniform_TF [T, num_freq] -> [hop*(T-1)]"""
    S = mel_to_linear(mel_TM, inv_FM, hp).T
    return A.inv_preemphasis(A.griffin_lim(S ** hp.power, hp, np.asarray(init_uniform_TF).T, iters), hp)
