"""Spectrogram -> waveform on the GPU vs oracle/audio_oracle.py (float64 restatement of
audio/__init__.py + librosa's stft/istft)."""
import numpy as np
import pytest

import audio_oracle as A

pytestmark = pytest.mark.gpu


class _HP(object):
    def __init__(self, a):
        self.__dict__.update(a.__dict__)


def _cmp(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_small_stft_parameters_match_oracle(iters):
    import torch, taco_amd
    ahp = A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3)   # n_fft 128, hop 20, win 80
    rs = np.random.RandomState(iters)
    B, T = 3, 37
    spec = rs.rand(B, T, 65) * 1.2 - 0.1                      # exercises the clip to [0,1]
    u = rs.rand(B, T, 65)
    gl = taco_amd.GriffinLim(_HP(ahp))
    wav = gl.inv_spectrogram(spec, init_uniform=u, iters=iters).cpu().numpy()
    assert wav.shape == (B, 20 * (T - 1))
    for b in range(B):
        ref = A.inv_spectrogram(spec[b].T, ahp, u[b].T, iters=iters)
        assert _cmp(wav[b], ref) < 2e-4, (b, _cmp(wav[b], ref))
    gl.close()


def test_reference_stft_parameters_one_iteration():
    """n_fft 2048, hop 300, win 1200 (24 kHz, 50 ms / 12.5 ms), 1025 bins."""
    import torch, taco_amd
    ahp = A.AudioHParams()
    rs = np.random.RandomState(5)
    B, T = 2, 24
    spec = rs.rand(B, T, 1025)
    u = rs.rand(B, T, 1025)
    gl = taco_amd.GriffinLim(_HP(ahp))
    wav = gl.inv_spectrogram(spec, init_uniform=u, iters=1).cpu().numpy()
    assert wav.shape == (B, 300 * (T - 1))
    for b in range(B):
        ref = A.inv_spectrogram(spec[b].T, ahp, u[b].T, iters=1)
        assert _cmp(wav[b], ref) < 5e-4
    gl.close()


def test_full_iterations_reach_the_same_spectral_consistency():
    """60 iterations amplify rounding differences sample by sample; what must agree is the quality of the result:
    the magnitude of the STFT of the produced waveform vs the requested magnitudes (spectral convergence)."""
    import torch, taco_amd
    ahp = A.AudioHParams(num_freq=129, sample_rate=3200, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=60)  # n_fft 256, hop 40, win 160
    rs = np.random.RandomState(9)
    T = 60
    t = np.arange(40 * (T - 1)) / 3200.0
    y0 = np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 555 * t * (1 + 0.2 * t))
    mag = np.abs(A.stft(y0, ahp))                                            # [F, T] a consistent spectrogram
    # encode it the way the model's output would be: normalised dB of mag^(1/power) ...
    S = mag ** (1 / ahp.power)
    spec = np.clip((20 * np.log10(np.maximum(1e-5, S)) - ahp.ref_level_db - ahp.min_level_db) / -ahp.min_level_db, 0, 1)
    target = A.db_to_amp(A.denormalize(spec, ahp) + ahp.ref_level_db) ** ahp.power
    u = rs.rand(129, T)
    gl = taco_amd.GriffinLim(_HP(ahp))
    wav = gl.inv_spectrogram(spec.T[None], init_uniform=u.T[None]).cpu().numpy()[0]
    ref = A.inv_spectrogram(spec, ahp, u)
    def sc(w):                                                               # undo the final inverse pre-emphasis first
        y = np.append(w[0], w[1:] - ahp.preemphasis * w[:-1])
        return np.linalg.norm(np.abs(A.stft(y, ahp)) - target) / np.linalg.norm(target)
    assert sc(ref) < 0.25
    assert abs(sc(wav) - sc(ref)) < 0.03, (sc(wav), sc(ref))
    gl.close()


def test_hash_initial_phases_and_errors():
    import torch, taco_amd
    ahp = A.AudioHParams(num_freq=65, sample_rate=1600)
    gl = taco_amd.GriffinLim(_HP(ahp))
    spec = np.random.RandomState(1).rand(2, 30, 65)
    a = gl.inv_spectrogram(spec, seed=7, iters=2).cpu().numpy()
    b = gl.inv_spectrogram(spec, seed=7, iters=2).cpu().numpy()
    c = gl.inv_spectrogram(spec, seed=8, iters=2).cpu().numpy()
    assert np.array_equal(a, b) and not np.array_equal(a, c) and np.isfinite(a).all()
    with pytest.raises(taco_amd._lib.TacoError):
        gl.inv_spectrogram(spec[:, :3], iters=1)               # too short for reflect padding
    with pytest.raises(Exception):
        gl.inv_spectrogram(spec[:, :, :10])
    gl.close()


def test_synthesizer_vocode_surface(tmp_path):
    import taco_amd
    import taco_oracle as O
    from util import tiny_hp, to_product_hp
    ohp = tiny_hp(num_freq=65, max_iters=20)
    hp = to_product_hp(ohp)
    hp.add_hparam("sample_rate", 1600); hp.add_hparam("griffin_lim_iters", 3)
    w = O.init_weights(ohp, 1, 31)
    taco_amd.save_hparams(str(tmp_path), hp)
    taco_amd.weights.save_weights(str(tmp_path / "model.ckpt-1.safetensors"), w)
    ids, L = O.synthetic_inputs(2, 9, 41)
    s = taco_amd.Synthesizer().load(str(tmp_path), num_speakers=1)
    lin, al = s.synthesize(tokens=ids, vocode=True)
    assert len(s.wavs) == 2 and all(w.ndim == 1 and np.isfinite(w).all() and len(w) > 0 for w in s.wavs)
    assert len(s.wavs[0]) == 20 * max(int(s.spec_end_idx[0]) - 1, 1)
    s.close()


# ---- the one marshalling layer of audio.py, through every public method that takes device data ----
_LIN, _MEL, _WAV = ("linear", (2, 8, 65)), ("mel", (2, 8, 12)), ("wav", (2, 140))
_METHODS = [      # handle, method, (its main argument, a good shape), its [B] vector
    ("gl", "inv_spectrogram", _LIN, None), ("gl", "inv_spectrogram_rows", _LIN, "frames"), ("tf", "inv_spectrogram_tensorflow", _LIN, "frames"),
    ("gl", "mel_to_linear", _MEL, None), ("gl", "inv_melspectrogram", _MEL, "frames"), ("gl", "pcm16", _WAV, "num_samples"),
    ("gl", "trim", _WAV, "num_samples"), ("gl", "split", _WAV, "num_samples"), ("gl", "remove_breath", _WAV, "num_samples"),
    ("sp", "targets", _WAV, "num_samples"), ("rs", "resample", _WAV, "num_samples")]
_BAD = [(h, m, a, v, kind) for h, m, a, v in _METHODS for kind in ("rank", "last", "vector", "init_uniform")
        if (kind != "last" or len(a[1]) == 3 or m == "resample") and (kind != "vector" or v)
        and (kind != "init_uniform" or m in ("inv_spectrogram", "inv_spectrogram_rows", "inv_melspectrogram"))]


@pytest.fixture(scope="module")
def handles():
    import taco_amd
    hp = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=2))
    hp.num_mels = 12
    h = {"gl": taco_amd.GriffinLim(hp), "tf": taco_amd.GriffinLim(hp, flavor="tensorflow"), "sp": taco_amd.Spectrogram(hp),
         "rs": taco_amd.audio.Resampler(3, 2)}
    h["gl"].set_inv_mel_basis()
    assert h["gl"].inv_mels == 12 and h["tf"].inv_mels == 0 and h["gl"].min_frames() == 5
    yield h
    for x in h.values():
        x.close()


@pytest.mark.parametrize("handle,method,arg,vector,kind", _BAD, ids=["%s-%s" % (m, k) for _, m, _, _, k in _BAD])
def test_every_method_refuses_a_bad_shape_by_the_arguments_name(handles, handle, method, arg, vector, kind):
    """A wrong rank, a wrong last dimension (where the method fixes one; for resample: a row that is no whole number of channels), a
    [B + 1] length vector and a narrower init_uniform each raise a plain Exception -- not TacoError: the library is never called --
    whose message names the argument."""
    import taco_amd
    name, shape = arg
    x, kw, blamed = np.zeros(shape, np.float32), {}, name
    if kind == "rank":
        x = x[0]
    elif kind == "last" and method == "resample":
        x, kw = x[:, :7], {"channels": 2}
    elif kind == "last":
        x = np.zeros(shape[:2] + (shape[2] + 1,), np.float32)
    elif kind == "vector":
        kw, blamed = {vector: [5] * (shape[0] + 1)}, vector
    else:
        kw, blamed = {"init_uniform": np.zeros((2, 8, 64), np.float32)}, "init_uniform"
    if method == "inv_spectrogram_rows":
        kw.setdefault("frames", None)
    with pytest.raises(Exception) as e:
        getattr(handles[handle], method)(x, **kw)
    print("%s %s: %s" % (method, kind, e.value))
    assert not isinstance(e.value, taco_amd._lib.TacoError) and blamed in str(e.value), (type(e.value), str(e.value))


@pytest.mark.parametrize("method", ["trim", "split", "remove_breath"])
def test_an_unknown_energy_is_an_argument_error(handles, method):
    import taco_amd
    with pytest.raises(taco_amd._lib.TacoError) as e:
        getattr(handles["gl"], method)(np.zeros((2, 140), np.float32), energy="loud")
    assert e.value.code == taco_amd._lib.TACO_ERR_ARG and "energy" in str(e.value)
