"""Waveform -> linear and mel training targets on the GPU (taco_spec_targets: k_spec_prepare, the windowed-DFT product of the
Griffin-Lim loop, k_spec_targets) against the float64 restatement tests/spec_reference.py, run per row on that row's own samples.

Error is measured per frame in the amplitude domain -- (a) every bin, |amp_dev - amp_ref| <= TOL_AMP x the frame's peak reference
amplitude -- and (b) in the normalised domain on the bins that carry at least 1e-2 of the frame's peak, |S_dev - S_ref| <= TOL_DB
(a dB bar on EVERY bin cannot be met by any fp32 transform: it blows up on bins far below the peak).

Bars = 4 x the worst value measured on an MI355X over the small and the reference case, the product at the three-product split-bf16
level (the margin covers other seeds and the fp32 log10); the tests print every figure (profiles/r08_spec_targets_tests.txt):
  (a) worst 6.54e-6 (linear, small parameters, the 161-sample row; reference parameters 4.63e-6; mel 3.77e-6 / 4.88e-6)
  (b) worst 2.99e-5 (linear, same row; reference parameters 2.68e-5; mel 1.67e-6 / 2.33e-5)
  epilogue alone on the reference's recorded magnitudes (test 3): 8.15e-8
TOL_DB is 1.2e-4, under the 1e-3 above which the product would move to the six-product level.  For comparison a plain fp32 DFT on the
CPU lands at 8e-7 (a) and 1e-6 (b).
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import audio_oracle as A
import spec_reference as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_AMP = 4 * 6.54e-6       # (a), x the frame's peak amplitude
TOL_DB = 4 * 2.99e-5        # (b), normalised units (1 = 100 dB); the issue's condition is <= 1e-3
TOL_EPILOGUE = 4 * 8.15e-8  # test 3, normalised units
FILL = 1.0e3                # what the input rows hold past their own samples: must never reach a kept frame


class _HP(object):
    def __init__(self, a, num_mels):
        self.__dict__.update(a.__dict__)
        self.num_mels = num_mels


SMALL = dict(name="small", ahp=A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5), num_mels=12,
             num_samples=[727, 460, 161, 65], frames=[37, 24, 9, 4])                     # n_fft 128, hop 20, win 80
REFERENCE = dict(name="reference", ahp=A.AudioHParams(), num_mels=80, num_samples=[7011, 3300], frames=[24, 12])   # n_fft 2048, hop 300, win 1200
CASES = {"small": SMALL, "reference": REFERENCE}


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """(wav [B, Lmax] with FILL past each row's samples, [(linear [T_b, F], mel [T_b, M]) per row]) -- computed once, read-only."""
    c = CASES[name]
    ns = c["num_samples"]
    wav = np.full((len(ns), max(ns)), FILL, np.float32)
    rows = []
    for b, n in enumerate(ns):
        y = R.test_signal(n, c["ahp"].sample_rate, 100 + b)
        wav[b, :n] = y
        D = R.magnitudes(y, c["ahp"])
        lin, mel = R.spectrogram(None, c["ahp"], D).T, R.melspectrogram(None, c["ahp"], c["num_mels"], D).T
        lin.setflags(write=False); mel.setflags(write=False)
        rows.append((lin, mel))
    wav.setflags(write=False)
    return wav, rows


def _errors(dev, ref, to_amp):
    """worst (a) and (b) of one row: dev, ref [T, bins] normalised"""
    ad, ar = to_amp(dev.astype(np.float64)), to_amp(ref)
    peak = ar.max(axis=1, keepdims=True)
    ea = float((np.abs(ad - ar) / peak).max())
    q = ar >= 1e-2 * peak
    eb = float(np.abs(dev - ref)[q].max())
    return ea, eb, float(q.mean())


def _run_case(name):
    import torch, taco_amd
    c = CASES[name]
    ahp = c["ahp"]
    wav, rows = _oracle(name)
    for which, i in (("linear", 0), ("mel", 1)):          # precondition: the floor and the clip do not hide the errors
        allv = np.concatenate([r[i].ravel() for r in rows])
        inside = float(((allv > 0) & (allv < 1)).mean())
        print("%s: %.1f %% of the oracle's %s bins strictly inside (0, 1)" % (name, 100 * inside, which))
        assert inside >= 0.8
    sp = taco_amd.Spectrogram(_HP(ahp, c["num_mels"]))
    lin, mel, nf = sp.targets(wav, torch.tensor(c["num_samples"], dtype=torch.int32, device="cuda"))
    lin, mel, nf = lin.cpu().numpy(), mel.cpu().numpy(), nf.cpu().numpy()
    sp.close()
    Tmax = 1 + wav.shape[1] // ahp.stft_parameters()[1]
    assert lin.shape == (len(rows), Tmax, ahp.num_freq) and mel.shape == (len(rows), Tmax, c["num_mels"]) and lin.dtype == mel.dtype == np.float32
    assert nf.dtype == np.int32 and nf.tolist() == c["frames"]
    worst = {}
    for b, (rl, rm) in enumerate(rows):
        T = c["frames"][b]
        assert rl.shape[0] == T == rm.shape[0]
        assert np.all(lin[b, T:] == 0.0) and np.all(mel[b, T:] == 0.0)
        for which, dev, ref, inv in (("linear", lin[b, :T], rl, lambda s: R.linear_amplitude(s, ahp)), ("mel", mel[b, :T], rm, lambda s: R.mel_amplitude(s, ahp))):
            ea, eb, frac = _errors(dev, ref, inv)
            print("%s row %d (%d samples, %d frames) %s: (a) amplitude err / frame peak %.3g   (b) normalised err %.3g on %.1f %% of bins" % (
                name, b, c["num_samples"][b], T, which, ea, eb, 100 * frac))
            worst[which] = (max(worst.get(which, (0, 0))[0], ea), max(worst.get(which, (0, 0))[1], eb))
    for which, (ea, eb) in worst.items():
        print("%s %s worst: (a) %.3g (bar %.3g)   (b) %.3g (bar %.3g)" % (name, which, ea, TOL_AMP, eb, TOL_DB))
    for which, (ea, eb) in worst.items():
        assert ea <= TOL_AMP, (which, ea)
        assert eb <= TOL_DB, (which, eb)


def test_tolerances_meet_the_condition():
    assert TOL_DB <= 1e-3        # 0.1 dB of the 100 dB range: above that the analysis product moves to the six-product level


def test_small_parameters_ragged_batch():
    """n_fft 128, hop 20, win 80, 12 mels; 727 samples (no multiple of hop), 460 (a multiple: the 1 + n // hop boundary), 161, 65 (the shortest legal)."""
    _run_case("small")


def test_reference_parameters():
    """1025 bins (an odd column count), n_fft 2048, hop 300, win 1200, 80 mels with bands up to 85 bins; 24 and 12 frames."""
    _run_case("reference")


def test_epilogue_alone_on_the_reference_vectors():
    """k_spec_targets through the debug hook on the reference's OWN recorded numbers: est = (golden mag.T, 0) -> golden normalize.T.
    Where the golden file holds exactly 0 or 1 (the floor 0, 1e-6, 1e-5 and the clip 1e3 of the first row among them) the device must too."""
    import ctypes as C
    import torch, taco_amd
    g = np.load(os.path.join(ROOT, "tests", "golden", "audio_vectors.npz"))
    mag, want = g["mag"].T, g["normalize"].T                     # [5, 1025]
    assert mag[:, 0].tolist() == [0.0, 1e-6, 1e-5, 1.0, 1e3]
    hpv = dict(zip([str(k) for k in g["hparams_keys"]], g["hparams_values"]))
    ahp = A.AudioHParams(**{k: hpv[k] for k in ("min_level_db", "ref_level_db") if k in hpv})
    sp = taco_amd.Spectrogram(_HP(ahp, 80))
    Rn, F = mag.shape
    est = torch.zeros((Rn, 2 * F), dtype=torch.float32, device="cuda")
    est[:, :F] = torch.from_numpy(mag.astype(np.float32)).cuda()
    lin = torch.empty((Rn, F), dtype=torch.float32, device="cuda")
    mel = torch.empty((Rn, 80), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    taco_amd._lib.check(sp._lib.taco_debug_spec_epilogue(sp._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(est), Rn, p(lin), p(mel)))
    got, gmel = lin.cpu().numpy(), mel.cpu().numpy()
    sp.close()
    e = float(np.abs(got - want).max())
    print("epilogue alone vs the reference's recorded normalize: max abs err %.3g (bar %.3g); %d entries at exactly 0, %d at exactly 1" % (
        e, TOL_EPILOGUE, int((want == 0).sum()), int((want == 1).sum())))
    assert (want == 0).any() and (want == 1).any()
    assert np.all(got[want == 0] == 0.0) and np.all(got[want == 1] == 1.0)
    assert e <= TOL_EPILOGUE
    mref = R.normalize(R.amp_to_db(taco_amd.audio.mel_basis(_HP(ahp, 80)) @ g["mag"]), ahp).T
    em = float(np.abs(gmel - mref).max())
    print("epilogue alone, mel rows vs float64: max abs err %.3g" % em)
    assert em <= TOL_DB


def test_control_ref_level_db_on_the_mel_side_misses_the_bar():
    """CPU arithmetic: the most likely slip -- subtracting ref_level_db on the mel side too, as the linear side does -- misses bar (b)
    of the small case by more than 100 x."""
    c = SMALL
    ahp = c["ahp"]
    wav, rows = _oracle("small")
    for b, n in enumerate(c["num_samples"]):
        D = R.magnitudes(wav[b, :n], ahp)
        n_fft = ahp.stft_parameters()[0]
        slip = R.normalize(R.amp_to_db(R.mel_filters(ahp.sample_rate, n_fft, c["num_mels"]) @ D) - ahp.ref_level_db, ahp).T
        _, eb, _ = _errors(slip.astype(np.float32), rows[b][1], lambda s: R.mel_amplitude(s, ahp))
        print("row %d: mel with ref_level_db subtracted misses (b) by %.3g = %.0f x the bar" % (b, eb, eb / TOL_DB))
        assert eb > 100 * TOL_DB


# ---- surface ----
def _small_sp(**kw):
    import taco_amd
    return taco_amd.Spectrogram(_HP(SMALL["ahp"], SMALL["num_mels"]), **kw)


def test_single_waveform_functions_equal_row_zero_of_targets():
    import torch
    wav, _ = _oracle("small")
    sp = _small_sp()
    lin, mel, nf = sp.targets(wav[:1])                          # num_samples None: all Lmax
    assert nf.tolist() == [37]
    s, m = sp.spectrogram(wav[0]), sp.melspectrogram(wav[0])
    assert tuple(s.shape) == (65, 37) and tuple(m.shape) == (12, 37)
    assert torch.equal(s, lin[0].t()) and torch.equal(m, mel[0].t())
    full = sp.targets(wav[:1], torch.tensor([727], dtype=torch.int32, device="cuda"))
    assert torch.equal(full[0], lin) and torch.equal(full[1], mel)
    sp.close()


def test_mel_is_optional_and_needs_a_basis():
    import torch, taco_amd
    wav, _ = _oracle("small")
    sp = _small_sp(basis=None)
    assert sp.num_mels == 0
    lin, mel, nf = sp.targets(wav, SMALL["num_samples"], mel=False)       # d_mel NULL works without a basis
    assert mel is None and nf.tolist() == SMALL["frames"]
    with pytest.raises(taco_amd._lib.TacoError):
        sp.targets(wav, SMALL["num_samples"])
    sp.set_mel_basis(taco_amd.audio.mel_basis(_HP(SMALL["ahp"], 12)))
    assert sp.num_mels == 12
    lin2, mel2, _ = sp.targets(wav, SMALL["num_samples"])
    assert torch.equal(lin, lin2) and tuple(mel2.shape) == (4, 37, 12)
    dense = np.abs(np.random.RandomState(0).randn(5, 65)) + 0.1           # a dense basis: full bands; calling again replaces the basis
    sp.set_mel_basis(dense)
    _, mel3, _ = sp.targets(wav[:1])
    D = R.magnitudes(wav[0], SMALL["ahp"])
    ref = R.normalize(R.amp_to_db(dense.astype(np.float32).astype(np.float64) @ D), SMALL["ahp"]).T
    assert tuple(mel3.shape) == (1, 37, 5) and float(np.abs(mel3[0].cpu().numpy() - ref).max()) <= TOL_DB
    sp.close()


def test_too_short_is_refused_and_short_rows_are_clamped():
    import torch, taco_amd
    wav, _ = _oracle("small")
    sp = _small_sp()
    with pytest.raises(taco_amd._lib.TacoError):
        sp.targets(wav[:, :64])                                  # Lmax <= n_fft/2
    a = sp.targets(wav[3:4], torch.tensor([3], dtype=torch.int32, device="cuda"))
    b = sp.targets(wav[3:4], torch.tensor([65], dtype=torch.int32, device="cuda"))
    assert a[2].tolist() == [4] == b[2].tolist()                 # 3 is clamped to n_fft/2 + 1 = 65 samples
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    sp.close()


@pytest.mark.parametrize("name", ["small", "reference"])
def test_two_calls_return_identical_bits(name):
    import torch, taco_amd
    c = CASES[name]
    wav, _ = _oracle(name)
    sp = taco_amd.Spectrogram(_HP(c["ahp"], c["num_mels"]))
    x = sp.targets(wav, c["num_samples"])
    y = sp.targets(wav, c["num_samples"])
    assert all(torch.equal(p, q) for p, q in zip(x, y))
    sp.close()


def test_process_and_generate_data(tmp_path):
    import taco_amd
    wav, rows = _oracle("small")
    ns = SMALL["num_samples"]
    sp = _small_sp()
    out = sp.process([wav[b, :n] for b, n in enumerate(ns)])
    for b, r in enumerate(out):
        assert r["linear"].shape == (SMALL["frames"][b], 65) and r["mel"].shape == (SMALL["frames"][b], 12)
        assert r["linear"].dtype == r["mel"].dtype == np.float32
    spec = importlib.util.spec_from_file_location("generate_data", os.path.join(ROOT, "tools", "generate_data.py"))
    gd = importlib.util.module_from_spec(spec); spec.loader.exec_module(gd)
    npy = str(tmp_path / "utt2.npy")
    np.save(npy, wav[2, :ns[2]])
    tokens = [np.arange(3 + b, dtype=np.int32) for b in range(3)]
    paths = gd.generate([wav[0, :ns[0]], wav[1, :ns[1]], npy], tokens, [1.0, 0.5, 2.0], str(tmp_path / "data"), batch=2, spectrogram=sp)
    sp.close()
    assert [os.path.basename(p) for p in paths] == ["000000.npz", "000001.npz", "utt2.npz"]
    with pytest.raises(Exception, match="not unique"):
        gd.generate([npy, npy], tokens[:2], 1.0, str(tmp_path / "dup"), spectrogram=sp)
    assert sorted(np.load(paths[0]).files) == ["linear", "loss_coeff", "mel", "tokens"]       # generate_data.py:156-161
    src = taco_amd.feeder.NpzSource(paths, 0, np.random.RandomState(0), training=False)
    ex = src()                                                   # the cursor starts at the third path
    assert not src.skipped
    vals = list(ex)
    assert np.array_equal(vals[0], tokens[2]) and float(vals[1]) == 2.0
    # (the same row in another batch may run on another GEMM tile: equal to the bar, not to the bit)
    assert vals[2].shape == out[2]["mel"].shape and np.abs(vals[2] - out[2]["mel"]).max() <= TOL_DB
    assert vals[3].shape == out[2]["linear"].shape and vals[3].dtype == np.float32
