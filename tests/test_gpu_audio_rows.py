"""Griffin-Lim per utterance length (taco_gl_inv_spectrogram_rows), the PCM16 kernel behind it and Synthesizer.synthesize_audio vs
oracle/audio_oracle.py run on the TRIMMED spectrogram -- what the reference computes (synthesizer.py:242-264:
`wav = wav[:spec_end_idx]; inv_spectrogram(wav.T)`; audio/__init__.py:22-25 for the scaling)."""
import numpy as np
import pytest

import audio_oracle as A
import gl_reference as G

pytestmark = pytest.mark.gpu


class _HP(object):
    def __init__(self, a):
        self.__dict__.update(a.__dict__)


def _cmp(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


def _small():
    return A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3)   # n_fft 128, hop 20, win 80


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_rows_match_oracle_on_the_trimmed_spectrogram(iters):
    """Parameters, seeds and bar (2e-4) of test_gpu_audio.test_small_stft_parameters_match_oracle, one more row, unequal lengths.
    The control shows the bar separates the two methods: the oracle on the zero-padded rectangle, sliced, is more than 1e-2 away
    from the oracle on the trimmed spectrogram on every short row."""
    import torch, taco_amd
    ahp = _small()
    rs = np.random.RandomState(iters)
    B, T = 4, 37
    frames = [37, 23, 8, 5]
    spec = rs.rand(B, T, 65) * 1.2 - 0.1
    u = rs.rand(B, T, 65)
    gl = taco_amd.GriffinLim(_HP(ahp))
    assert gl.min_frames() == 5
    wav, ns = gl.inv_spectrogram_rows(spec, torch.tensor(frames, dtype=torch.int32, device="cuda"), init_uniform=u, iters=iters)
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert wav.shape == (B, 20 * (T - 1)) and ns.dtype == np.int32
    assert ns.tolist() == [20 * (f - 1) for f in frames]
    for b, f in enumerate(frames):
        n = 20 * (f - 1)
        ref = A.inv_spectrogram(spec[b, :f].T, ahp, u[b, :f].T, iters=iters)
        assert ref.shape == (n,)
        e = _cmp(wav[b, :n], ref)
        print("iters %d row %d frames %d: rel max-abs err %.3g" % (iters, b, f, e))
        assert e < 2e-4, (b, f, e)
        assert np.all(wav[b, n:] == 0.0)
        if f < T:                                                # control, CPU only: the padded-rectangle method misses the bar
            padded = spec[b].copy()
            padded[f:] = 0.0
            old = A.inv_spectrogram(padded.T, ahp, u[b].T, iters=iters)[:n]
            d = _cmp(old, ref)
            print("iters %d row %d frames %d: padded-and-sliced oracle vs trimmed oracle %.3g" % (iters, b, f, d))
            assert d > 1e-2, (b, f, d)
    gl.close()


def test_rows_reference_stft_parameters_one_iteration():
    """n_fft 2048, hop 300, win 1200, 1025 bins; the bar of test_gpu_audio.test_reference_stft_parameters_one_iteration."""
    import torch, taco_amd
    ahp = A.AudioHParams()
    rs = np.random.RandomState(5)
    B, T = 2, 24
    frames = [24, 11]
    spec = rs.rand(B, T, 1025)
    u = rs.rand(B, T, 1025)
    gl = taco_amd.GriffinLim(_HP(ahp))
    assert gl.min_frames() == 5
    wav, ns = gl.inv_spectrogram_rows(spec, frames, init_uniform=u, iters=1)         # host frames: uploaded by the binding
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert wav.shape == (B, 300 * (T - 1)) and ns.tolist() == [300 * (f - 1) for f in frames]
    for b, f in enumerate(frames):
        n = 300 * (f - 1)
        ref = A.inv_spectrogram(spec[b, :f].T, ahp, u[b, :f].T, iters=1)
        e = _cmp(wav[b, :n], ref)
        print("row %d frames %d: rel max-abs err %.3g" % (b, f, e))
        assert e < 5e-4, (b, f, e)
        assert np.all(wav[b, n:] == 0.0)
    gl.close()


def test_full_length_rows_are_the_old_entry_point():
    import torch, taco_amd
    ahp = _small()
    rs = np.random.RandomState(3)
    B, T = 3, 30
    spec = rs.rand(B, T, 65) * 1.2 - 0.1
    u = rs.rand(B, T, 65)
    gl = taco_amd.GriffinLim(_HP(ahp))
    for kw in (dict(init_uniform=u), dict(seed=11)):
        old = gl.inv_spectrogram(spec, iters=3, **kw).cpu().numpy()
        for frames in ([T] * B, None):
            wav, ns = gl.inv_spectrogram_rows(spec, frames, iters=3, **kw)
            assert np.array_equal(wav.cpu().numpy(), old), (sorted(kw), frames)
            assert ns.cpu().numpy().tolist() == [20 * (T - 1)] * B
    assert np.isfinite(old).all() and np.abs(old).max() > 0
    gl.close()


def test_the_batch_entry_point_is_the_rows_entry_point_without_frames():
    """inv_spectrogram is inv_spectrogram_rows(x, None, ...)[0]: the same bits, and a full-length frames vector reports hop*(T-1)."""
    import torch, taco_amd
    rs = np.random.RandomState(8)
    B, T = 2, 8
    spec, u = rs.rand(B, T, 65) * 1.2 - 0.1, rs.rand(B, T, 65)
    gl = taco_amd.GriffinLim(_HP(_small()))
    assert gl.min_frames() == 5
    old = gl.inv_spectrogram(spec, u, iters=2).cpu().numpy()
    assert old.shape == (B, 140) and np.isfinite(old).all() and np.abs(old).max() > 0
    assert np.array_equal(gl.inv_spectrogram_rows(spec, None, u, iters=2)[0].cpu().numpy().view(np.uint32), old.view(np.uint32))
    wav, ns = gl.inv_spectrogram_rows(spec, [8, 8], u, iters=2)
    assert ns.cpu().numpy().tolist() == [140, 140] and np.array_equal(wav.cpu().numpy().view(np.uint32), old.view(np.uint32))
    gl.close()


def test_frames_are_clamped_and_short_batches_refused():
    import torch, taco_amd
    ahp = _small()
    gl = taco_amd.GriffinLim(_HP(ahp))
    T = 30
    spec = np.random.RandomState(1).rand(4, T, 65)
    wav, ns = gl.inv_spectrogram_rows(spec, [-3, 0, 3, T + 9], seed=7, iters=2)
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert ns.tolist() == [20 * 4, 20 * 4, 20 * 4, 20 * (T - 1)]
    assert np.isfinite(wav).all()
    for b in range(4):
        assert np.abs(wav[b, :ns[b]]).max() > 0 and np.all(wav[b, ns[b]:] == 0.0)
    with pytest.raises(taco_amd._lib.TacoError):
        gl.inv_spectrogram_rows(spec[:, :gl.min_frames() - 1], [4] * 4, iters=1)
    with pytest.raises(taco_amd._lib.TacoError):
        gl.inv_spectrogram_rows(spec[:, :3], None, iters=1)
    gl.close()


def test_pcm16_is_save_audios_arithmetic():
    """pcm = trunc(x * 32767 / max(0.01, max|x[:n]|)) (audio/__init__.py:23-24) against NumPy float64 on the device's own float32
    waveform.  Two fp32 roundings (the scale, the product) move a full-scale value by at most 0.004 of a step, so a sample may land on
    the other side of an integer -- off by one -- only when it lies that close to one: at most 0.8 % of samples; the bar is 1 %.
    A row reaches full scale (32767, or 32766 after the roundings) when its peak is at least the 0.01 floor of the scale; the
    all-zero row stays zero and the row with peak 0.004 reaches 0.4 of full scale, as save_audio would write them.
    Against the float32 restatement of the same arithmetic the samples are equal, all of them."""
    import torch, taco_amd
    ahp = _small()
    rs = np.random.RandomState(2)
    B, T = 3, 37
    frames = [37, 20, 6]
    gl = taco_amd.GriffinLim(_HP(ahp))
    wav, ns = gl.inv_spectrogram_rows(rs.rand(B, T, 65), frames, seed=4, iters=2)
    L = wav.shape[1]
    quiet = wav[1:2] * (0.004 / wav[1, :int(ns[1])].abs().max())            # peak below 0.01: the floor of the scale applies
    wav = torch.cat([wav, torch.zeros_like(wav[:1]), quiet], 0)
    ns = torch.cat([ns, torch.tensor([L, int(ns[1])], dtype=torch.int32, device=ns.device)])
    pcm = gl.pcm16(wav, ns)
    assert pcm.dtype == torch.int16 and tuple(pcm.shape) == (5, L)
    wav32 = wav.cpu().numpy()
    pcm, x, n = pcm.cpu().numpy().astype(np.int64), wav32.astype(np.float64), ns.cpu().numpy()
    for b in range(5):
        peak = np.abs(x[b, :n[b]]).max()
        ref = np.trunc(x[b, :n[b]] * 32767 / max(0.01, peak)).astype(np.int64)
        d = np.abs(pcm[b, :n[b]] - ref)
        print("row %d: n %d peak %.4g max |diff| %d share differing %.4f peak pcm %d" % (b, n[b], peak, d.max(), (d > 0).mean(), np.abs(pcm[b]).max()))
        assert d.max() <= 1 and (d > 0).mean() <= 0.01, (b, d.max(), (d > 0).mean())
        assert np.all(pcm[b, n[b]:] == 0)
        # and to the sample against the same arithmetic in float32 (tests/gl_reference.py): the kernel is one correctly rounded division
        # (the scale), one multiplication, a truncation and the clamp, each of which NumPy's float32 reproduces
        same = G.pcm16_f32(wav32[b], int(n[b])).astype(np.int64)
        print("row %d: samples differing from the float32 restatement %d of %d" % (b, int((pcm[b] != same).sum()), same.size))
        assert np.array_equal(pcm[b], same), (b, np.flatnonzero(pcm[b] != same)[:8])
        if peak >= 0.01:
            assert np.abs(pcm[b]).max() in (32767, 32766), b
    assert np.all(pcm[3] == 0)
    assert 0 < np.abs(pcm[4]).max() < 32766 * 0.5                            # the quiet row is not normalised up to full scale
    full = gl.pcm16(wav[:1]).cpu().numpy()                                  # num_samples None: the whole row
    assert np.array_equal(full, pcm[:1].astype(np.int16))
    gl.close()


def test_synthesize_audio_surface(tmp_path):
    import torch, taco_amd
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
    wavs = s.synthesize_audio(tokens=ids, pcm=False, seed=3)
    end = np.asarray(s.spec_end_idx)
    lin, al = s.synthesize(tokens=ids)
    assert np.array_equal(end, s.spec_end_idx)
    gl = taco_amd.GriffinLim(hp)
    T = lin.shape[1]
    clamped = np.clip(end, gl.min_frames(), T)
    hand, ns = gl.inv_spectrogram_rows(lin, end, seed=3)
    hand, ns = hand.cpu().numpy(), ns.cpu().numpy()
    assert len(wavs) == 2
    for b in range(2):
        n = 20 * (int(clamped[b]) - 1)
        assert wavs[b].dtype == np.float32 and wavs[b].shape == (n,) and ns[b] == n
        assert np.isfinite(wavs[b]).all() and np.abs(wavs[b]).max() > 0
        e = _cmp(wavs[b], hand[b, :n])
        print("row %d: spec_end_idx %d -> %d samples, vs the rows call by hand %.3g" % (b, end[b], n, e))
        assert e < 2e-4, (b, e)
    pcms = s.synthesize_audio(tokens=ids, seed=3)
    assert [p.dtype for p in pcms] == [np.int16] * 2 and [len(p) for p in pcms] == [len(x) for x in wavs]
    for p, x in zip(pcms, wavs):
        ref = np.trunc(x.astype(np.float64) * 32767 / max(0.01, np.abs(x).max()))
        assert np.abs(p - ref).max() <= 1
    untrimmed = s.synthesize_audio(tokens=ids, attention_trim=False, pcm=False, seed=3)
    assert s.spec_end_idx is None and [len(x) for x in untrimmed] == [20 * (T - 1)] * 2
    gl.close()
    s.close()
