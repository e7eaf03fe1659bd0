"""Host side of the waveform -> training-target path: the mel filter bank (audio.mel_basis vs the independently written
tests/spec_reference.py), the frame count, and the float64 helper itself against the reference's own recorded outputs
(tests/golden/audio_vectors.npz).  No GPU."""
import os

import numpy as np
import pytest

import audio_oracle as A
import spec_reference as R
from taco_amd import audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _HP(A.AudioHParams):
    def __init__(self, a, num_mels):
        self.__dict__.update(a.__dict__)
        self.num_mels = num_mels


REF = _HP(A.AudioHParams(), 80)                                                                                   # 24000 Hz, n_fft 2048
SMALL = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5), 12)          # n_fft 128, hop 20, win 80


@pytest.mark.parametrize("hp", [REF, SMALL], ids=["24000-2048-80", "1600-128-12"])
def test_mel_basis_equals_the_per_filter_formulation(hp):
    n_fft = (hp.num_freq - 1) * 2
    a, b = audio.mel_basis(hp), R.mel_filters(hp.sample_rate, n_fft, hp.num_mels)
    assert a.dtype == np.float64 and a.shape == (hp.num_mels, hp.num_freq) == b.shape
    d = float(np.abs(a - b).max())
    print("mel basis (%d, %d, %d): max abs difference %.3g (largest weight %.3g)" % (hp.sample_rate, n_fft, hp.num_mels, d, b.max()))
    assert d < 1e-12


def test_slaney_scale_known_points():
    assert float(audio.hz_to_mel(1000.0)) == pytest.approx(15.0, abs=1e-12)
    assert float(audio.mel_to_hz(15.0)) == pytest.approx(1000.0, abs=1e-9)
    assert R.hz_to_mel(1000.0) == pytest.approx(15.0, abs=1e-12) and R.mel_to_hz(15.0) == pytest.approx(1000.0, abs=1e-9)
    assert float(audio.hz_to_mel(6400.0)) == pytest.approx(42.0, abs=1e-12)        # 27 mels per factor 6.4
    f = np.array([0.0, 100.0, 999.0, 1000.0, 1001.0, 5000.0, 12000.0])
    assert np.allclose(audio.mel_to_hz(audio.hz_to_mel(f)), f, rtol=1e-13, atol=1e-10)


def test_filter_bands_at_the_reference_parameters():
    w = audio.mel_basis(REF)
    nz = w != 0
    widths = nz.sum(1)
    assert (widths > 0).all()
    for m in range(w.shape[0]):                                  # a triangle: its non-zeros are one run of bins
        k = np.flatnonzero(nz[m])
        assert k[-1] - k[0] + 1 == len(k)
    print("band widths %d .. %d bins, %d non-zeros" % (widths.min(), widths.max(), nz.sum()))
    assert widths.min() == 7 and widths.max() == 85 and nz.sum() == 2000
    assert (audio.mel_basis(SMALL) != 0).sum(1).min() > 0


def test_slaney_area_normalisation():
    w = audio.mel_basis(REF)
    area = w.sum(1) * REF.sample_rate / 2048
    print("filter areas %.4f .. %.4f" % (area.min(), area.max()))
    assert np.all(np.abs(area - 1) < 0.02)


@pytest.mark.parametrize("hp", [REF, SMALL], ids=["hop300", "hop20"])
def test_num_frames(hp):
    hop = hp.stft_parameters()[1]
    for n in (hop - 1, hop, hop + 1, 7 * hop - 1, 7 * hop, 7 * hop + 1, 0):
        assert audio.num_frames(hp, n) == 1 + n // hop
    n_fft = (hp.num_freq - 1) * 2
    for n in (n_fft // 2 + 1, 5 * hop, 5 * hop + 7, 11 * hop - 1):
        if n > n_fft // 2:
            assert audio.num_frames(hp, n) == A.stft(np.zeros(n), hp).shape[1]


def test_helper_reproduces_the_reference_vectors():
    g = np.load(os.path.join(ROOT, "tests", "golden", "audio_vectors.npz"))
    hpv = dict(zip([str(k) for k in g["hparams_keys"]], g["hparams_values"]))
    hp = A.AudioHParams(**{k: hpv[k] for k in ("preemphasis", "min_level_db", "ref_level_db") if k in hpv})
    d = float(np.abs(R.preemphasis(g["wave"], hp) - g["preemphasis"]).max())
    print("preemphasis: max abs difference %.3g" % d)
    assert d == 0.0
    db = R.amp_to_db(g["mag"])
    d_db = float(np.abs(db - g["amp_to_db"]).max())
    d_n = float(np.abs(R.normalize(db - hp.ref_level_db, hp) - g["normalize"]).max())
    print("amp_to_db: max abs difference %.3g; normalize: %.3g" % (d_db, d_n))
    assert d_db < 1e-12 and d_n < 1e-14
