"""NumPy float64 restatement of the Fast Griffin-Lim loop (Perraudin, Balazs, Sondergaard 2013) in both flavours, and of the spectral
convergence the device reports: test infrastructure only, nothing in the product imports it.

With momentum a and c = a / (1 + a):
    y = istft(X0); t_prev = 0
    repeat iters times:  t = stft(y);  z = t - c * t_prev (first iteration: z = t);  t_prev = t;  y = istft(project(z))
    project(z) = S * exp(i angle(z))          librosa flavour and mel (np.angle(0) = 0)
               = S * z / max(1e-8, |z|)       TensorFlow flavour
This is librosa.griffinlim's loop (0.7 and later) with the reference's own normalisations in place of z / (|z| + 1e-16).  It composes
oracle/audio_oracle.py's stft / istft / inv_preemphasis and tests/vocoder_reference.py's tf_stft / tf_istft, and at momentum 0 its
expressions are theirs, so that it returns their bits (tests/test_fast_gl_host.py)."""
import numpy as np

import audio_oracle as A
import vocoder_reference as V


CONSISTENT = A.AudioHParams(num_freq=129, sample_rate=3200, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=60)   # n_fft 256, hop 40, win 160


def consistent_case(seed, T=60):
    """The input of test_gpu_audio.test_full_iterations_reach_the_same_spectral_consistency: (spec [F, T] normalised, the magnitudes it
    stands for [F, T], initial phases [F, T]) of a two-tone signal's own STFT magnitudes; `seed` draws the phases"""
    ahp = CONSISTENT
    t = np.arange(40 * (T - 1)) / 3200.0
    y0 = np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 555 * t * (1 + 0.2 * t))
    mag = np.abs(A.stft(y0, ahp))
    S = mag ** (1 / ahp.power)
    spec = np.clip((20 * np.log10(np.maximum(1e-5, S)) - ahp.ref_level_db - ahp.min_level_db) / -ahp.min_level_db, 0, 1)
    return spec, magnitudes(spec, ahp), np.random.RandomState(seed).rand(129, T)


def _c(momentum):
    return float(momentum) / (1.0 + float(momentum))


def griffin_lim(S, hp, init_uniform, iters=None, momentum=0.0, return_min_z=False):
    """audio_oracle.griffin_lim with momentum.  S [F, T] magnitudes, init_uniform [F, T] in [0, 1).  With return_min_z also the smallest
    |z| met in any iteration (inf with none)."""
    c = _c(momentum)
    angles = np.exp(2j * np.pi * init_uniform)
    Sc = np.abs(S).astype(np.complex128)
    y = A.istft(Sc * angles, hp)
    t_prev, lo = None, np.inf
    for _ in range(hp.griffin_lim_iters if iters is None else iters):
        t = A.stft(y, hp)
        z = t if (t_prev is None or c == 0.0) else t - c * t_prev
        t_prev = t
        lo = min(lo, float(np.abs(z).min()))
        angles = np.exp(1j * np.angle(z))
        y = A.istft(Sc * angles, hp)
    return (y, lo) if return_min_z else y


def inv_spectrogram(spec_FT, hp, init_uniform, iters=None, momentum=0.0):
    """audio_oracle.inv_spectrogram with momentum: spec_FT [num_freq, T] normalised -> [hop*(T-1)]"""
    S = A.db_to_amp(A.denormalize(spec_FT, hp) + hp.ref_level_db)
    return A.inv_preemphasis(griffin_lim(S ** hp.power, hp, init_uniform, iters, momentum), hp)


def inv_melspectrogram(mel_TM, inv_FM, hp, init_uniform_TF, iters=None, momentum=0.0, return_min_z=False):
    """vocoder_reference.inv_melspectrogram with momentum"""
    S = V.mel_to_linear(mel_TM, inv_FM, hp).T
    y, lo = griffin_lim(S ** hp.power, hp, np.asarray(init_uniform_TF).T, iters, momentum, return_min_z=True)
    y = A.inv_preemphasis(y, hp)
    return (y, lo) if return_min_z else y


def inv_spectrogram_tensorflow(spec_TF, hp, iters=None, momentum=0.0, return_min_z=False):
    """vocoder_reference.inv_spectrogram_tensorflow with momentum: spec_TF [T, num_freq] -> [hop*(T-1) + win]"""
    c = _c(momentum)
    S = V.tf_magnitudes(spec_TF, hp)
    y = V.tf_istft(S.astype(np.complex128), hp)
    t_prev, lo = None, np.inf
    for _ in range(hp.griffin_lim_iters if iters is None else iters):
        est = V.tf_stft(y, hp)
        z = est if (t_prev is None or c == 0.0) else est - c * t_prev
        t_prev = est
        mag = np.abs(z)
        lo = min(lo, float(mag.min()))
        y = V.tf_istft(S * (z / np.maximum(1e-8, mag)), hp)
    return (y, lo) if return_min_z else y


def magnitudes(spec_FT, hp):
    """The target of inv_spectrogram: (10^((clip(x,0,1) * -min_db + min_db + ref_db) / 20))^power, [num_freq, T]"""
    return A.db_to_amp(A.denormalize(np.asarray(spec_FT, np.float64), hp) + hp.ref_level_db) ** hp.power


def analysed_magnitudes(y_after_inverse_preemphasis, hp):
    """|stft(p)| [num_freq, T], p the pre-emphasis of the vocoder's output: it undoes the inverse pre-emphasis the vocoder ended with"""
    w = np.asarray(y_after_inverse_preemphasis, np.float64)
    p = np.append(w[0], w[1:] - hp.preemphasis * w[:-1])
    return np.abs(A.stft(p, hp))


def spectral_convergence(y_after_inverse_preemphasis, S, hp):
    """|| |stft(p)| - S || / || S ||, S [num_freq, T] the magnitudes the waveform was synthesised from; 0 for a silent target"""
    S = np.asarray(S, np.float64)
    den = np.linalg.norm(S)
    return float(np.linalg.norm(analysed_magnitudes(y_after_inverse_preemphasis, hp) - S) / den) if den > 0 else 0.0
