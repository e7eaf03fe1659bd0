"""Host side of the two other vocoders (inv_spectrogram_tensorflow, inv_melspectrogram): the float64 restatement
tests/vocoder_reference.py against identities and known answers, the pseudo-inverse of the mel filter bank, and the argument and state
errors of the new entry points, which come before their first device call.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import audio_oracle as A
import vocoder_reference as V
from taco_amd import _lib, audio


class _HP(A.AudioHParams):
    def __init__(self, a, num_mels):
        self.__dict__.update(a.__dict__)
        self.num_mels = num_mels


REF = _HP(A.AudioHParams(), 80)                                                                                   # n_fft 2048, hop 300, win 1200
SMALL = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5), 12)          # n_fft 128, hop 20, win 80


@pytest.mark.parametrize("T", [1, 2, 5, 37])
def test_frame_count_and_length_identities(T):
    n_fft, hop, win = SMALL.stft_parameters()
    rs = np.random.RandomState(T)
    X = rs.randn(T, 65) + 1j * rs.randn(T, 65)
    y = V.tf_istft(X, SMALL)
    assert y.shape == (hop * (T - 1) + win,)
    assert V.tf_stft(y, SMALL).shape == (T, 65)
    assert V.tf_stft(np.zeros(win - 1), SMALL).shape == (0, 65)
    assert V.tf_stft(np.zeros(win + hop - 1), SMALL).shape == (1, 65) and V.tf_stft(np.zeros(win + hop), SMALL).shape == (2, 65)
    assert V.inv_spectrogram_tensorflow(rs.rand(T, 65), SMALL, iters=2).shape == (hop * (T - 1) + win,)


def test_stft_is_the_left_aligned_window():
    """X_k = sum_n y[n] w[n] e^{-2 pi i k n / N}, n < W: written out as the sum, against the framed rfft"""
    n_fft, hop, win = SMALL.stft_parameters()
    y = np.random.RandomState(0).randn(win)
    n, k = np.arange(win), np.arange(65)
    direct = (y * V.hann(win))[None, :] @ np.exp(-2j * np.pi * np.outer(n, k) / n_fft)
    assert np.abs(V.tf_stft(y, SMALL) - direct).max() < 1e-12


def test_one_frame_of_a_constant_spectrum():
    """X_k = c for every k: irfft is c at n = 0 and 0 elsewhere, and the Hann window is 0 at n = 0 -- the frame is all zeros; with
    X_k = c * e^{-2 pi i k / N} the impulse moves to n = 1 and the one non-zero sample is c * w[1]."""
    n_fft, hop, win = SMALL.stft_parameters()
    c = 0.75
    y = V.tf_istft(np.full((1, 65), c, np.complex128), SMALL)
    assert y.shape == (win,) and np.abs(y).max() < 1e-15
    y = V.tf_istft(c * np.exp(-2j * np.pi * np.arange(65) / n_fft)[None, :], SMALL)
    want = np.zeros(win); want[1] = c * V.hann(win)[1]
    assert np.abs(y - want).max() < 1e-15


def test_zero_magnitudes_and_zero_estimates_give_zeros():
    n_fft, hop, win = SMALL.stft_parameters()
    hp = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, min_level_db=-100, ref_level_db=20, power=1.5), 12)
    # S = 0 cannot come out of the dB law, so it is put in directly: every iterate is zero, and est = 0 goes through est / 1e-8 = 0
    S = np.zeros((4, 65))
    y = V.tf_istft(S.astype(np.complex128), hp)
    est = V.tf_stft(y, hp)
    assert not y.any() and not est.any()
    X = np.ones((4, 65)) * (est / np.maximum(1e-8, np.abs(est)))          # S = 1 on a zero estimate: 0, not S
    assert not X.any() and not V.tf_istft(X, hp).any()
    # the librosa rule differs there: exp(i * angle(0)) = 1 keeps S
    assert np.all(np.exp(1j * np.angle(est)) == 1)


@pytest.mark.parametrize("hp", [SMALL, REF], ids=["65x12", "1025x80"])
def test_inv_mel_basis_is_a_right_inverse(hp):
    b, inv = audio.mel_basis(hp), audio.inv_mel_basis(hp)
    assert inv.dtype == np.float64 and inv.shape == (hp.num_freq, hp.num_mels)
    assert np.linalg.matrix_rank(b) == hp.num_mels
    d = float(np.abs(b @ inv - np.eye(hp.num_mels)).max())
    print("mel_basis . inv_mel_basis - I: max abs %.3g; largest |inv| %.3g" % (d, np.abs(inv).max()))
    assert d < 1e-9


def test_mel_to_linear_restatement_floor_and_scale():
    inv = audio.inv_mel_basis(SMALL)
    lin = V.mel_to_linear(np.zeros((2, 12)), inv, SMALL)                    # normalised 0 = min_level_db: amplitude 1e-5 in every filter
    assert lin.shape == (2, 65) and lin.min() >= 1e-10
    assert np.abs(lin - np.maximum(1e-10, 1e-5 * inv.sum(1))[None, :]).max() < 1e-18
    assert np.all(V.mel_amplitudes(np.array([[1.5, 1.0]]), SMALL) == 1.0)   # clip to 1 -> 0 dB, and no ref_level_db added


def _host_handle(lib, hp, tf):
    h = C.c_void_p()
    chp = audio.c_audio_hparams(hp)
    assert lib.taco_debug_gl_create_host(C.byref(chp), int(tf), C.byref(h)) == 0
    return h


def test_symbols_and_host_arithmetic():
    lib = _lib.load_library()
    for name in ("taco_gl_create_tf", "taco_gl_tf_num_samples", "taco_gl_tf_workspace_bytes", "taco_gl_inv_spectrogram_tf",
                 "taco_gl_set_inv_mel_basis", "taco_gl_mel_to_linear", "taco_gl_inv_melspectrogram_rows"):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
    h = _host_handle(lib, SMALL, True)
    assert lib.taco_gl_tf_num_samples(h, 37) == 20 * 36 + 80 and lib.taco_gl_tf_num_samples(h, 1) == 80
    assert lib.taco_gl_tf_num_samples(h, 0) == 0 and lib.taco_gl_tf_num_samples(None, 5) == 0
    assert lib.taco_gl_tf_workspace_bytes(h, 3, 37) > 0 and lib.taco_gl_tf_workspace_bytes(h, 0, 37) == 0
    assert lib.taco_gl_tf_workspace_bytes(h, 3, 37) == lib.taco_gl_rows_workspace_bytes(h, 3, 37)      # the same slot layout
    lib.taco_gl_destroy(h)


def test_argument_and_state_errors_need_no_device():
    lib = _lib.load_library()
    err = lambda: lib.taco_last_error()
    tf, lr = _host_handle(lib, SMALL, True), _host_handle(lib, SMALL, False)
    buf = (C.c_float * 16)()
    d = C.cast(buf, C.c_void_p)          # never dereferenced: every call below returns before its first device call
    big = 1 << 30

    def run_tf(g=tf, spec=d, B=3, T=37, wav=d, ws=d):
        return lib.taco_gl_inv_spectrogram_tf(g, None, spec, None, B, T, 1, wav, None, ws, big)

    assert run_tf(g=None) == _lib.TACO_ERR_ARG and run_tf(spec=None) == _lib.TACO_ERR_ARG
    assert run_tf(wav=None) == _lib.TACO_ERR_ARG and run_tf(ws=None) == _lib.TACO_ERR_ARG
    assert run_tf(B=0) == _lib.TACO_ERR_ARG and run_tf(T=0) == _lib.TACO_ERR_ARG and run_tf(B=65536) == _lib.TACO_ERR_ARG
    assert run_tf(g=lr) == _lib.TACO_ERR_STATE and b"taco_gl_create_tf" in err()

    def run_rows(fn, g=lr, x=d, wav=d, ws=d, B=3, T=37):
        return fn(g, None, x, None, None, 0, B, T, 1, wav, None, ws, big)

    for fn in (lib.taco_gl_inv_spectrogram_rows, lib.taco_gl_inv_melspectrogram_rows):
        assert run_rows(fn, g=None) == _lib.TACO_ERR_ARG and run_rows(fn, x=None) == _lib.TACO_ERR_ARG
        assert run_rows(fn, wav=None) == _lib.TACO_ERR_ARG and run_rows(fn, ws=None) == _lib.TACO_ERR_ARG
        assert run_rows(fn, B=0) == _lib.TACO_ERR_ARG and run_rows(fn, T=1) == _lib.TACO_ERR_ARG
        assert run_rows(fn, g=tf) == _lib.TACO_ERR_STATE and b"taco_gl_create_tf" in err()       # a librosa entry point on a TF handle
    assert lib.taco_gl_inv_spectrogram(tf, None, d, None, 0, 3, 37, 1, d, d, big) == _lib.TACO_ERR_STATE
    assert lib.taco_spec_targets(tf, None, d, None, 2, 1000, d, None, None, d, big) == _lib.TACO_ERR_STATE
    # the mel vocoder and the op-level product without an inverse basis
    assert run_rows(lib.taco_gl_inv_melspectrogram_rows) == _lib.TACO_ERR_STATE and b"taco_gl_set_inv_mel_basis" in err()
    for g in (lr, tf):
        assert lib.taco_gl_mel_to_linear(g, None, d, 2, 5, d) == _lib.TACO_ERR_STATE and b"taco_gl_set_inv_mel_basis" in err()
    assert lib.taco_gl_mel_to_linear(None, None, d, 2, 5, d) == _lib.TACO_ERR_ARG
    assert lib.taco_gl_mel_to_linear(lr, None, None, 2, 5, d) == _lib.TACO_ERR_ARG and lib.taco_gl_mel_to_linear(lr, None, d, 2, 5, None) == _lib.TACO_ERR_ARG
    assert lib.taco_gl_mel_to_linear(lr, None, d, 0, 5, d) == _lib.TACO_ERR_ARG and lib.taco_gl_mel_to_linear(lr, None, d, 2, 0, d) == _lib.TACO_ERR_ARG
    assert lib.taco_gl_set_inv_mel_basis(None, d, 12) == _lib.TACO_ERR_ARG and lib.taco_gl_set_inv_mel_basis(lr, None, 12) == _lib.TACO_ERR_ARG
    assert lib.taco_gl_set_inv_mel_basis(lr, d, 0) == _lib.TACO_ERR_ARG
    assert lib.taco_gl_set_inv_mel_basis(lr, d, 4096) == _lib.TACO_ERR_UNSUPPORTED and b"LDS" in err()
    h = C.c_void_p()
    chp = audio.c_audio_hparams(SMALL)
    assert lib.taco_gl_create_tf(None, 0, C.byref(h)) == _lib.TACO_ERR_ARG and lib.taco_gl_create_tf(C.byref(chp), 0, None) == _lib.TACO_ERR_ARG
    lib.taco_gl_destroy(tf); lib.taco_gl_destroy(lr)


def test_python_surface_rejects_unknown_names_before_the_device():
    with pytest.raises(_lib.TacoError) as e:
        audio.GriffinLim(SMALL, device="cuda:0", flavor="tf2")
    assert e.value.code == _lib.TACO_ERR_ARG
