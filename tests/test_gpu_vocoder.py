"""The reference's two other vocoders on the GPU -- inv_spectrogram_tensorflow (GriffinLim(flavor="tensorflow")) and
inv_melspectrogram -- against tests/vocoder_reference.py, float64 restatements on framed arrays with np.fft.  Both are UNPINNED on
TensorFlow / librosa (include/taco_abi.h).  The device takes float32 spectrograms; the restatements get the same float32 values.

Measured on an MI355X (every test prints its figures; DESIGN.md §3.8 quotes them):
  TF flavour, 0 / 1 / 4 iterations (bar 2e-4)     error over the reference's peak at most 3.5e-6 / 7.3e-6 / 2.9e-5
  mel -> linear                                   largest |gpu - ref| over the derived bound 0.297 (65 x 12) and 0.0752 (1025 x 80)
  mel vocoder, 0 / 1 / 4 iterations (bar 2e-4)    6.9e-6 / 6.0e-6 / 1.2e-5"""
import functools

import numpy as np
import pytest

import audio_oracle as A
import vocoder_reference as V

pytestmark = pytest.mark.gpu


class _HP(A.AudioHParams):
    def __init__(self, a, num_mels):
        self.__dict__.update(a.__dict__)
        self.num_mels = num_mels


SMALL = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3), 12)   # n_fft 128, hop 20, win 80
REF = _HP(A.AudioHParams(), 80)                                                                                                 # n_fft 2048, hop 300, win 1200
B, T = 3, 37


def _cmp(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _spec(seed, F=65, b=B, t=T):
    s = (np.random.RandomState(seed).rand(b, t, F) * 1.2 - 0.1).astype(np.float32)      # exercises the clip to [0,1]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _tf_ref(seed, iters, row, frames=T):
    """(waveform, smallest |est| of any iteration) of row `row` of _spec(seed) cut to `frames` frames"""
    return V.inv_spectrogram_tensorflow(_spec(seed)[row, :frames], SMALL, iters=iters, return_min_est=True)


@pytest.fixture(scope="module")
def gl_tf():
    import taco_amd
    g = taco_amd.GriffinLim(SMALL, flavor="tensorflow")
    yield g
    g.close()


@pytest.fixture(scope="module")
def gl_mel():
    import taco_amd
    g = taco_amd.GriffinLim(SMALL)
    g.set_inv_mel_basis()
    yield g
    g.close()


# ---- 1. the TF flavour against the restatement ----
@pytest.mark.parametrize("iters", [0, 1, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tf_flavour_matches_the_restatement(gl_tf, seed, iters):
    refs = [_tf_ref(seed, iters, b) for b in range(B)]
    lo = min(r[1] for r in refs)
    assert lo > 1e-4, lo                                       # no bin of the restatement is within rounding of the 1e-8 branch
    wav, ns = gl_tf.inv_spectrogram_tensorflow(_spec(seed), iters=iters)
    wav = wav.cpu().numpy()
    assert wav.shape == (B, 20 * (T - 1) + 80) and ns.cpu().numpy().tolist() == [20 * (T - 1) + 80] * B
    errs = [_cmp(wav[b], refs[b][0]) for b in range(B)]
    print("tf flavour seed %d iters %d: error over peak %.3g (bar 2e-4), smallest |est| %.3g" % (seed, iters, max(errs), lo))
    assert max(errs) < 2e-4, errs


# ---- 2. the reference's STFT parameters, once ----
def test_tf_flavour_at_the_reference_stft_parameters():
    import taco_amd
    spec = (np.random.RandomState(5).rand(2, 8, 1025) * 1.2 - 0.1).astype(np.float32)
    g = taco_amd.GriffinLim(REF, flavor="tensorflow")
    wav, ns = g.inv_spectrogram_tensorflow(spec, iters=1)
    wav = wav.cpu().numpy()
    assert wav.shape == (2, 300 * 7 + 1200) and ns.cpu().numpy().tolist() == [300 * 7 + 1200] * 2
    for b in range(2):
        ref, lo = V.inv_spectrogram_tensorflow(spec[b], REF, iters=1, return_min_est=True)
        e = _cmp(wav[b], ref)
        print("tf flavour, 1025 bins, row %d: error over peak %.3g (bar 5e-4), smallest |est| %.3g" % (b, e, lo))
        assert lo > 1e-4 and e < 5e-4, (e, lo)
    g.close()


# ---- 3. frames: each row is the vocoding of its own truncated spectrogram ----
def test_tf_flavour_frames_are_the_truncated_spectrogram(gl_tf):
    frames = [37, 9, 1]
    wav, ns = gl_tf.inv_spectrogram_tensorflow(_spec(1), frames=np.array(frames, np.int32), iters=2)
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert wav.shape == (B, 20 * (T - 1) + 80)
    assert ns.tolist() == [20 * (f - 1) + 80 for f in frames]
    for b, f in enumerate(frames):
        ref, lo = _tf_ref(1, 2, b, f)
        n = 20 * (f - 1) + 80
        assert len(ref) == n and lo > 1e-4
        e = _cmp(wav[b, :n], ref)
        print("tf flavour, %d of %d frames: error over peak %.3g (bar 2e-4)" % (f, T, e))
        assert e < 2e-4
        assert not wav[b, n:].any()                           # exact zeros past the row's own samples
    # clamped to [1, T] on the device
    w2, n2 = gl_tf.inv_spectrogram_tensorflow(_spec(1), frames=np.array([99, 9, -4], np.int32), iters=2)
    assert np.array_equal(w2.cpu().numpy(), wav) and np.array_equal(n2.cpu().numpy(), ns)


# ---- 4. determinism and capture ----
def test_tf_flavour_is_deterministic_capturable_and_leaves_the_librosa_flavour_alone(gl_tf):
    import torch, taco_amd
    lib_gl = taco_amd.GriffinLim(SMALL)
    u = np.random.RandomState(7).rand(B, T, 65).astype(np.float32)
    before = lib_gl.inv_spectrogram(_spec(0), init_uniform=u, iters=2).clone()
    x = torch.from_numpy(_spec(2).copy()).cuda()
    fr = torch.tensor([37, 20, 3], dtype=torch.int32, device="cuda")
    a, na = gl_tf.inv_spectrogram_tensorflow(x, fr, iters=3)
    b, nb = gl_tf.inv_spectrogram_tensorflow(x, fr, iters=3)
    assert torch.equal(a, b) and torch.equal(na, nb) and bool(torch.isfinite(a).all())
    a, na = a.clone(), na.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):            # the workspace has its size from the calls above: nothing is allocated by the library
            c, nc = gl_tf.inv_spectrogram_tensorflow(x, fr, iters=3)
    torch.cuda.current_stream().wait_stream(side)
    c.zero_(); nc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, a) and torch.equal(nc, na)
    after = lib_gl.inv_spectrogram(_spec(0), init_uniform=u, iters=2)
    assert torch.equal(before, after)
    with pytest.raises(taco_amd._lib.TacoError) as e:
        gl_tf.inv_spectrogram(_spec(0), iters=1)               # a librosa entry point on a TF handle
    assert e.value.code == taco_amd._lib.TACO_ERR_STATE
    with pytest.raises(taco_amd._lib.TacoError) as e:
        lib_gl.inv_spectrogram_tensorflow(_spec(0), iters=1)
    assert e.value.code == taco_amd._lib.TACO_ERR_STATE
    lib_gl.close()


# ---- 5. mel -> linear under the fp32 dot-product bound ----
@pytest.mark.parametrize("hp", [SMALL, REF], ids=["65x12", "1025x80"])
def test_mel_to_linear_within_the_dot_product_bound(hp):
    """|gpu - ref| <= (num_mels + 3) * 2^-24 * sum_m |inv[f, m]| * amp[m] + 1e-30 per element: num_mels fmaf roundings, one rounding
    each for the fp32 inverse basis and the amplitude (formed in double on the device and rounded once), one to spare; max(1e-10, .)
    is 1-Lipschitz when both sides take the same floor -- float32 cannot hold 1e-10, so the restatement is floored at the float32
    nearest to it (1.3e-18 away, which alone would pass the bound of a bin whose inverse-basis row is ~1e-14 of rounding, as the DC
    bin's is).  A bin whose row of the inverse basis is all zero (Nyquist) has bound 0: the floor exactly."""
    import taco_amd
    from taco_amd import audio
    M, F = hp.num_mels, hp.num_freq
    inv = audio.inv_mel_basis(hp)
    mel = (np.random.RandomState(11).rand(2, 25, M) * 1.2 - 0.1).astype(np.float32)
    g = taco_amd.GriffinLim(hp)
    with pytest.raises(taco_amd._lib.TacoError) as e:
        g.mel_to_linear(mel)
    assert e.value.code == taco_amd._lib.TACO_ERR_STATE
    g.set_inv_mel_basis(inv)
    out = g.mel_to_linear(mel).cpu().numpy().reshape(50, F)
    g.close()
    rows = mel.reshape(50, M)
    floor = float(np.float32(1e-10))
    assert abs(floor - 1e-10) <= 2.0 ** -24 * 1e-10
    ref = np.maximum(floor, V.mel_amplitudes(rows, hp) @ inv.T)
    assert np.abs(ref - V.mel_to_linear(rows, inv, hp)).max() <= abs(floor - 1e-10)        # the restatement, but for the floor's last bits
    mass = V.mel_amplitudes(rows, hp) @ np.abs(inv).T                       # sum_m |inv[f, m]| amp[m], [50, F]
    bound = (M + 3) * 2.0 ** -24 * mass + 1e-30
    dead = np.abs(inv.astype(np.float32)).sum(1) == 0                         # the fp32 basis the device holds
    live = ~dead
    err = np.abs(out.astype(np.float64) - ref)
    ratio = float((err[:, live] / bound[:, live]).max())
    clamped = float((ref == floor).mean())
    print("mel_to_linear (%d bins, %d mels): largest error over the bound %.3g; %.1f %% of the sums clamp at 1e-10; %d bins with an all-zero row"
          % (F, M, ratio, 100 * clamped, int(dead.sum())))
    assert np.all(out[:, dead] == np.float32(1e-10))
    assert ratio <= 1.0, ratio
    assert out.min() >= np.float32(1e-10)


# ---- 6. the mel vocoder against the restatement ----
@functools.lru_cache(maxsize=None)
def _mel_case():
    rs = np.random.RandomState(21)
    mel = (rs.rand(B, T, 12) * 1.2 - 0.1).astype(np.float32)
    u = rs.rand(B, T, 65).astype(np.float32)
    return mel, u


@pytest.mark.parametrize("iters", [0, 1, 4])
def test_mel_vocoder_matches_the_restatement(gl_mel, iters):
    from taco_amd import audio
    mel, u = _mel_case()
    inv = audio.inv_mel_basis(SMALL)
    wav, ns = gl_mel.inv_melspectrogram(mel, init_uniform=u, iters=iters)
    wav = wav.cpu().numpy()
    assert wav.shape == (B, 20 * (T - 1)) and ns.cpu().numpy().tolist() == [20 * (T - 1)] * B
    errs = [_cmp(wav[b], V.inv_melspectrogram(mel[b], inv, SMALL, u[b], iters=iters)) for b in range(B)]
    print("mel vocoder iters %d: error over peak %.3g (bar 2e-4)" % (iters, max(errs)))
    assert max(errs) < 2e-4, errs


def test_mel_vocoder_frames_are_the_truncated_input(gl_mel):
    from taco_amd import audio
    mel, u = _mel_case()
    inv = audio.inv_mel_basis(SMALL)
    frames = [37, 20, 9]
    wav, ns = gl_mel.inv_melspectrogram(mel, frames=np.array(frames, np.int32), init_uniform=u, iters=1)
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert ns.tolist() == [20 * (f - 1) for f in frames]
    for b, f in enumerate(frames):
        n = 20 * (f - 1)
        e = _cmp(wav[b, :n], V.inv_melspectrogram(mel[b, :f], inv, SMALL, u[b, :f], iters=1))
        print("mel vocoder, %d of %d frames: error over peak %.3g (bar 2e-4)" % (f, T, e))
        assert e < 2e-4
        assert not wav[b, n:].any()


# ---- 7. Synthesizer.synthesize_audio(vocoder=...) ----
def test_synthesizer_vocoder_argument(tmp_path):
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

    def same(a, b):
        return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))

    def expect(gl, wav, ns):
        pcm, n = gl.pcm16(wav, ns).cpu().numpy(), ns.cpu().numpy()
        return [p[:k] for p, k in zip(pcm, n)]

    got = s.synthesize_audio(tokens=ids, vocoder="tensorflow")
    frames = torch.from_numpy(np.asarray(s.spec_end_idx, np.int32)).cuda()
    gl = taco_amd.GriffinLim(s.hparams, flavor="tensorflow")
    assert same(got, expect(gl, *gl.inv_spectrogram_tensorflow(s.model.linear_outputs, frames)))
    assert all(a.dtype == np.int16 and len(a) == 20 * (min(max(int(f), 1), 60) - 1) + 80 for a, f in zip(got, s.spec_end_idx))
    gl.close()

    got = s.synthesize_audio(tokens=ids, vocoder="mel", seed=3)
    gl = taco_amd.GriffinLim(s.hparams)
    gl.set_inv_mel_basis()
    mel = s.model.mel_outputs.reshape(2, -1, s.hparams.num_mels)
    assert mel.shape[1] == s.model.linear_outputs.shape[1]
    assert same(got, expect(gl, *gl.inv_melspectrogram(mel, frames, seed=3)))
    gl.close()

    assert same(s.synthesize_audio(tokens=ids, seed=5), s.synthesize_audio(tokens=ids, seed=5, vocoder="griffin_lim"))
    f32 = s.synthesize_audio(tokens=ids, vocoder="tensorflow", pcm=False, librosa_trim=True)
    assert all(a.dtype == np.float32 for a in f32) and s.trim_index is not None and [len(a) for a in f32] == s.trim_index[:, 1].tolist()
    with pytest.raises(taco_amd._lib.TacoError) as e:
        s.synthesize_audio(tokens=ids, vocoder="wavenet")
    assert e.value.code == taco_amd._lib.TACO_ERR_ARG
    s.close()
