"""Silence trimming on the device (taco_wav_trim, GriffinLim.trim, Synthesizer.synthesize_audio(librosa_trim=True)) against the float64
restatement tests/trim_reference.py of `librosa.effects.trim` as synthesizer.py:266-269 calls it.  UNPINNED on librosa (see the
restatement's header): what is held here is the kernels against that restatement, not against librosa.

The index is compared for EQUALITY, on every row.  That is meaningful because every input is built so that no frame of the
restatement lies within MARGIN = 0.05 dB of the threshold (asserted on the CPU before the device is asked), and the device's dB
values are held to DB_BAR.  Measured on an MI355X over every case of this file: largest |dB difference| 1.31e-5 dB (printed per row
with -s); DB_BAR is ten times that, rounded up, which is far below the 0.01 dB (a fifth of MARGIN) the comparison needs."""
import functools

import numpy as np
import pytest

import trim_reference as R

pytestmark = pytest.mark.gpu

MARGIN = 0.05            # dB: no frame of the restatement may be this close to -top_db
DB_BAR = 2e-4            # dB: ten times the measured 1.31e-5, rounded up; the condition is <= 0.01 (a fifth of MARGIN)
assert DB_BAR <= MARGIN / 5

LENGTHS = [700, 451, 64, 33, 9, 1]                 # frame 64: single reflection, repeated reflection (n < 32), the degenerate row
BURSTS = [(0.3, 0.7), (0.5, 1.0), (0.4, 1.0), (0.2, 0.6), (0.3, 0.8), (0.0, 1.0)]      # row 1's burst runs to its last sample
# (frame_length, hop_length) -> (top_db, seed, dc): seeds and offsets chosen on the CPU from the restatement's margins alone
SMALL = {(64, 8): (40.0, 0, 0.6), (80, 20): (40.0, 1, 0.3)}


class _HP(object):
    sample_rate, num_freq, frame_length_ms, frame_shift_ms = 1600, 65, 50, 12.5


@pytest.fixture(scope="module")
def gl():
    import taco_amd
    g = taco_amd.GriffinLim(_HP())
    yield g
    g.close()


@functools.lru_cache(maxsize=None)
def _small_case(N, hop, ragged):
    """(wav [6, 700] float32, lengths or None, top_db, {energy: [(index, db, margin) per row]}): computed once, shared, not modified."""
    top_db, seed, dc = SMALL[(N, hop)]
    lengths = LENGTHS if ragged else [700] * 6
    bursts = BURSTS if ragged else [(0.3, 0.7), (0.0, 0.5), (0.5, 1.0), (0.2, 0.6), (0.1, 0.9), (0.4, 0.8)]
    x = R.burst_rows(700, lengths, bursts, seed, dc_row=0, dc=dc)
    ref = {e: [R.trim(x[b, :n], top_db, N, hop, e) for b, n in enumerate(lengths)] for e in R.ENERGIES}
    x.setflags(write=False)
    return x, (lengths if ragged else None), top_db, ref


@functools.lru_cache(maxsize=None)
def _reference_case():
    lengths = [40000, 1500]
    x = R.burst_rows(40000, lengths, [(0.25, 0.65), (0.3, 0.7)], seed=0, dc_row=0, dc=0.3)
    ref = {e: [R.trim(x[b, :n], 50.0, 5120, 256, e) for b, n in enumerate(lengths)] for e in R.ENERGIES}
    x.setflags(write=False)
    return x, lengths, 50.0, ref


def _check_margins(ref, what):
    for e, rows in ref.items():
        for b, (index, db, margin) in enumerate(rows):
            print("%s %s row %d: restatement index %s, margin %.3f dB" % (what, e, b, index.tolist(), margin))
            assert margin >= MARGIN, (what, e, b, margin)


def _run_and_compare(gl, x, lengths, top_db, N, hop, energy, rows, what):
    """NaN past every row's count, one device call, index equality and the dB bar; returns the largest dB difference."""
    import torch
    B, L = x.shape
    xn = np.array(x, np.float32, copy=True)
    ns = None
    if lengths is not None:
        for b, n in enumerate(lengths):
            xn[b, n:] = np.nan                                # nothing at or past n_b may be read
        ns = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    index, db = gl.trim(torch.from_numpy(xn).cuda(), ns, top_db=top_db, frame_length=N, hop_length=hop, energy=energy, return_db=True)
    assert index.dtype == torch.int32 and tuple(index.shape) == (B, 2) and tuple(db.shape) == (B, 1 + L // hop)
    index, db = index.cpu().numpy(), db.cpu().numpy()
    assert np.isfinite(db).all()
    worst = 0.0
    for b, (ri, rdb, margin) in enumerate(rows):
        nf = len(rdb)
        d = float(np.abs(db[b, :nf] - rdb).max()) if nf else 0.0
        worst = max(worst, d)
        print("%s %s row %d: device index %s restatement %s, max |dB difference| %.3g over %d frames" % (what, energy, b, index[b].tolist(), ri.tolist(), d, nf))
        assert index[b].tolist() == ri.tolist(), (what, energy, b, index[b].tolist(), ri.tolist())
        assert np.all(db[b, nf:] == 0.0)
        assert d <= DB_BAR, (what, energy, b, d)
    return worst


@pytest.mark.parametrize("ragged", [True, False], ids=["lengths", "num_samples_null"])
@pytest.mark.parametrize("energy", R.ENERGIES)
@pytest.mark.parametrize("N,hop", sorted(SMALL))
def test_small_parameters_index_equals_the_restatement(gl, N, hop, energy, ragged):
    """frame 64 / hop 8 and frame 80 / hop 20 (four waves share a tile of 16 frames: the hop does not divide it evenly), B = 6, L = 700;
    lengths [700, 451, 64, 33, 9, 1] or none."""
    x, lengths, top_db, ref = _small_case(N, hop, ragged)
    _check_margins(ref, "%d/%d" % (N, hop))
    _run_and_compare(gl, x, lengths, top_db, N, hop, energy, ref[energy], "%d/%d" % (N, hop))
    if ragged:
        assert ref[energy][1][0][1] == 451                   # the burst that runs to the last sample: end == n, the min(n, ...) branch
        assert [r[0].tolist() for r in ref[energy][2:]] == [[0, 64], [0, 33], [0, 9], [0, 1]]
    assert 0 < ref[energy][0][0][0] and ref[energy][0][0][1] < 700      # leading and trailing silence are both cut on row 0


@pytest.mark.parametrize("energy", R.ENERGIES)
def test_reference_parameters(gl, energy):
    """5120 / 256 / 50 dB as synthesizer.py:267-268 calls it, B = 2, lengths [40000, 1500] (the short row is reflected twice)."""
    x, lengths, top_db, ref = _reference_case()
    _check_margins(ref, "5120/256")
    _run_and_compare(gl, x, lengths, top_db, 5120, 256, energy, ref[energy], "5120/256")
    assert ref["spectral"][0][0].tolist() != ref["time"][0][0].tolist()


@pytest.mark.parametrize("which", ["64/8", "5120/256"])
def test_control_the_dc_and_nyquist_terms_decide_the_index(which):
    """CPU only: on the row with the offset, the restatement without the two unpaired bins (N sum xw^2 / 2 alone) returns another
    index -- so index equality on that row tells the full form from the truncated one."""
    if which == "64/8":
        x, lengths, top_db, ref = _small_case(64, 8, True)
        N, hop = 64, 8
    else:
        x, lengths, top_db, ref = _reference_case()
        N, hop = 5120, 256
    full = ref["spectral"][0][0].tolist()
    cut = R.trim(x[0, :lengths[0]], top_db, N, hop, "spectral", drop_dc_nyquist=True)[0].tolist()
    print("%s row 0: full form %s, without the DC and Nyquist terms %s" % (which, full, cut))
    assert full != cut


def test_all_zero_row_and_burst_to_the_last_sample(gl):
    import torch
    x = np.array(_small_case(64, 8, True)[0], copy=True)
    x[2] = 0.0                                               # all zero over n = 300: every frame clamps to 1e-10, db = 0 > -top_db
    x[3] = 0.0
    x[3, 500:655] = 0.3 * np.random.RandomState(5).randn(155)      # exact zeros, then a burst up to the last of its 655 samples
    lengths = [700, 451, 300, 655]
    ns = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    for energy in R.ENERGIES:
        index, db = gl.trim(torch.from_numpy(x[:4]).cuda(), ns, top_db=40, frame_length=64, hop_length=8, energy=energy, return_db=True)
        index, db = index.cpu().numpy(), db.cpu().numpy()
        ref = [R.trim(x[b, :n], 40, 64, 8, energy) for b, n in enumerate(lengths)]
        assert min(r[2] for r in ref) >= MARGIN
        assert [r[0].tolist() for r in ref] == index.tolist()
        assert index[2].tolist() == [0, 300] and np.all(db[2] == 0.0)
        assert index[3][1] == 655 and index[3][0] > 0 and index[1][1] == 451


def test_two_calls_give_the_same_bits(gl):
    import torch
    x, lengths, top_db, ref = _reference_case()
    xs, ls, *_ = _small_case(80, 20, True)
    for wav, ns, kw in ((x, lengths, dict(top_db=50, frame_length=5120, hop_length=256)), (xs, ls, dict(top_db=40, frame_length=80, hop_length=20))):
        w = torch.from_numpy(np.array(wav)).cuda()
        n = torch.tensor(ns, dtype=torch.int32, device="cuda")
        for energy in R.ENERGIES:
            a = gl.trim(w, n, energy=energy, return_db=True, **kw)
            a = [t.clone() for t in a]
            gl.pcm16(w, n)                                    # something else on the stream in between
            b = gl.trim(w, n, energy=energy, return_db=True, **kw)
            assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_capture_and_replay_of_trim_and_pcm16(gl):
    import torch
    x, lengths, top_db, ref = _reference_case()
    w = torch.from_numpy(np.array(x)).cuda()
    n = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    kw = dict(top_db=50, frame_length=5120, hop_length=256)

    def chain():
        index = gl.trim(w, n, **kw)
        return index, gl.pcm16(w, index[:, 1].contiguous())
    e_index, e_pcm = [t.clone() for t in chain()]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()                                              # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        c_index, c_pcm = chain()
    c_index.zero_(); c_pcm.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(c_index, e_index) and torch.equal(c_pcm, e_pcm)
    assert e_index.cpu().numpy().tolist() == [r[0].tolist() for r in ref["spectral"]]
    assert int((e_pcm[0, int(e_index[0, 1]):] != 0).sum()) == 0 and int(e_pcm[0].abs().max()) >= 32766


def test_synthesize_audio_librosa_trim(tmp_path):
    """The small model of tests/test_gpu_audio_rows.py with a hop of 40 samples and 402 frames, so that a row (16 040 samples) is longer
    than the 5120-sample frame of the reference's trim call.  The model's linear output is mapped into [0.6, 0.8] and its last third
    scaled by 0.02 (a hundred dB quieter after the 1.5 power), so there is a tail to cut."""
    import torch, taco_amd
    import taco_oracle as O
    from util import tiny_hp, to_product_hp
    from taco_amd.hparams import EOS_ID
    ohp = tiny_hp(num_freq=65, max_iters=134)
    hp = to_product_hp(ohp)
    hp.add_hparam("sample_rate", 1600); hp.add_hparam("griffin_lim_iters", 3); hp.add_hparam("frame_shift_ms", 25.0)
    w = O.init_weights(ohp, 1, 31)
    taco_amd.save_hparams(str(tmp_path), hp)
    taco_amd.weights.save_weights(str(tmp_path / "model.ckpt-1.safetensors"), w)
    ids, L = O.synthetic_inputs(2, 9, 41)
    s = taco_amd.Synthesizer().load(str(tmp_path), num_speakers=1)
    run = s.model.run

    def run_with_a_quiet_tail(**kw):
        lin, al = run(**kw)
        lin = lin.clamp(0.0, 1.0) * 0.2 + 0.6
        cut = (2 * lin.shape[1]) // 3
        lin[:, cut:] *= 0.02
        return lin, al
    s.model.run = run_with_a_quiet_tail
    kw = dict(tokens=ids, seed=3, attention_trim=False)
    plain = s.synthesize_audio(pcm=False, librosa_trim=False, **kw)          # the untrimmed float rows
    assert s.trim_index is None
    n = len(plain[0])
    assert n >= 3 * 5120 and all(len(p) == n for p in plain)                # the quiet third is longer than the trim's frame
    ref = [R.trim(p, 50, 5120, 256, "spectral") for p in plain]
    for b, (index, db, margin) in enumerate(ref):
        print("row %d: %d samples, restatement index %s, margin %.3f dB" % (b, n, index.tolist(), margin))
        assert margin >= MARGIN, (b, margin)
        assert 0 < index[1] < n                                              # there is a tail, and it is cut
    trimmed = s.synthesize_audio(pcm=False, librosa_trim=True, **kw)
    assert s.trim_index.dtype == np.int32 and s.trim_index.tolist() == [r[0].tolist() for r in ref]
    for b in range(2):
        end = int(ref[b][0][1])
        assert trimmed[b].dtype == np.float32 and np.array_equal(trimmed[b], plain[b][:end])
    pcms = s.synthesize_audio(librosa_trim=True, **kw)
    assert s.trim_index.tolist() == [r[0].tolist() for r in ref]
    for b in range(2):
        x = plain[b][:int(ref[b][0][1])].astype(np.float64)
        want = np.trunc(x * 32767 / max(0.01, np.abs(x).max())).astype(np.int64)       # save_audio's scaling of the trimmed prefix
        d = np.abs(pcms[b].astype(np.int64) - want)
        assert pcms[b].dtype == np.int16 and pcms[b].shape == want.shape
        assert d.max() <= 1 and (d > 0).mean() <= 0.01, (b, d.max(), (d > 0).mean())
        assert np.abs(pcms[b]).max() in (32767, 32766)
    # the flag off is the call as it was: the same bits as composing the steps by hand, and as leaving the keyword out
    off = s.synthesize_audio(librosa_trim=False, **kw)
    assert s.trim_index is None
    default = s.synthesize_audio(**kw)
    gl = s._griffin_lim()
    lin, _ = run_with_a_quiet_tail(inputs=ids.astype(np.int32), input_lengths=np.argmax(ids == EOS_ID, 1).astype(np.int32), speaker_id=None,
                                   manual_alignments=None, is_manual_attention=False)
    hw, hn = gl.inv_spectrogram_rows(lin, None, seed=3)
    hand = gl.pcm16(hw, hn).cpu().numpy()
    for b in range(2):
        assert np.array_equal(off[b], default[b]) and np.array_equal(off[b], hand[b, :n]) and len(off[b]) == n
    # Synthesizer.synthesize(vocode=True, librosa_trim=True): each entry of wavs is cut to its end; without vocode the flag does nothing
    s.synthesize(tokens=ids, vocode=True, attention_trim=False)
    full = [np.array(x) for x in s.wavs]
    assert s.trim_index is None
    s.synthesize(tokens=ids, vocode=True, attention_trim=False, librosa_trim=True)
    ref2 = [R.trim(x, 50, 5120, 256, "spectral") for x in full]
    assert min(r[2] for r in ref2) >= MARGIN, [r[2] for r in ref2]
    assert s.trim_index.tolist() == [r[0].tolist() for r in ref2]
    for b in range(2):
        assert np.array_equal(s.wavs[b], full[b][:int(s.trim_index[b, 1])]) and len(s.wavs[b]) < len(full[b])
    s.synthesize(tokens=ids, attention_trim=False, librosa_trim=True)
    assert s.wavs is None and s.trim_index is None
    s.close()
