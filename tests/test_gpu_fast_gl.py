"""Fast Griffin-Lim on the GPU (taco_gl_set_momentum: k_gl_project_fast in the loop of all three vocoders) and the device's own report of
spectral convergence (taco_gl_convergence: k_gl_convergence_partial / _final) against the float64 restatement tests/fast_gl_reference.py.
The device takes float32 inputs; the restatement gets the same float32 values.

Shapes are the smallest that cross the boundaries: num_freq 65 at 1600 Hz (n_fft 128, hop 20, win 80), B = 3, T = 37 -- rows x bins =
8580 is no multiple of the 256-thread workgroup, min_frames is 5, 37 frames are five tiles of the convergence kernel and the last is
partial.  num_freq 66 is the one even bin count: the only shape at which k_gl_project_fast takes its 8-byte path.

Bars.  Parity of the librosa flavour: 2e-4 of the reference's peak, the bar tests/test_gpu_audio.py holds the plain loop to on these
inputs; a float32 emulation of the restatement puts the fast loop at no more than 2.5 x the plain loop's rounding up to 5 iterations, so
were the plain loop measured above 8e-5 the fast loop would be held to 2.5 x that measurement instead.  Measured on an MI355X at 1 / 2 /
3 / 5 iterations (every case prints both; profiles/r20_fast_gl_tests.txt): plain loop 5.8e-6 / 5.5e-6 / 9.1e-6 / 7.5e-6, momentum 0.99
5.8e-6 / 5.6e-6 / 8.4e-6 / 2.1e-5 -- the plain loop is far below 8e-5, so the bar is 2e-4.  Ragged rows, mel and TensorFlow flavours:
2e-4, the bars of tests/test_gpu_audio_rows.py and tests/test_gpu_vocoder.py (measured: at most 1.1e-5).  Convergence: derived, see
_sc_bound (measured: at most 1.1e-7 against bounds of 3.4e-5 and up)."""
import ctypes as C
import functools

import numpy as np
import pytest

import audio_oracle as A
import fast_gl_reference as FG
import vocoder_reference as V

pytestmark = pytest.mark.gpu


class _HP(A.AudioHParams):
    def __init__(self, a, num_mels=12):
        self.__dict__.update(a.__dict__)
        self.num_mels = num_mels


SMALL = _HP(A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3))      # n_fft 128, hop 20, win 80
EVEN = _HP(A.AudioHParams(num_freq=66, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3))       # n_fft 130, hop 20, win 80
CONSISTENT = _HP(FG.CONSISTENT)
B, T, F, HOP = 3, 37, 65, 20
RAGGED = (37, 5, 20)
M = 0.99
BAR = 2e-4
ETA = 4 * 6.54e-6       # tests/test_gpu_spec.py TOL_AMP: the analysis product's element-wise bar, x the frame's peak amplitude


def _cmp(a, b):
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _inputs(seed, freq=F, b=B, t=T):
    rs = np.random.RandomState(seed)
    spec = (rs.rand(b, t, freq) * 1.2 - 0.1).astype(np.float32)      # exercises the clip to [0,1]
    u = rs.rand(b, t, freq).astype(np.float32)
    spec.setflags(write=False); u.setflags(write=False)
    return spec, u


@functools.lru_cache(maxsize=None)
def _ref(seed, row, frames, iters, momentum):
    spec, u = _inputs(seed)
    return FG.inv_spectrogram(spec[row, :frames].T, SMALL, u[row, :frames].T, iters=iters, momentum=momentum)


@pytest.fixture(scope="module")
def gl():
    import taco_amd
    g = taco_amd.GriffinLim(SMALL)
    g.set_inv_mel_basis()
    yield g
    g.close()


@pytest.fixture(scope="module")
def dev(gl):
    """Device outputs shared by the parity and the convergence cases: seed 5, momentum 0.99 -- 5 iterations on the full rectangle, 3 on RAGGED"""
    spec, u = _inputs(5)
    full = gl.inv_spectrogram(spec, init_uniform=u, iters=5, momentum=M)
    rag, ns = gl.inv_spectrogram_rows(spec, np.array(RAGGED, np.int32), init_uniform=u, iters=3, momentum=M)
    gl.set_momentum(0)
    return {"full": full.clone(), "ragged": rag.clone(), "ns": ns.cpu().numpy()}


# ---- 1. parity, librosa flavour ----
@pytest.mark.parametrize("iters", [1, 2, 3, 5])
def test_fast_loop_matches_the_restatement(gl, dev, iters):
    """1: no previous estimate; 2: first use of it; 3: the two estimate buffers have swapped back; 5: beyond"""
    spec, u = _inputs(5)
    plain = gl.inv_spectrogram(spec, init_uniform=u, iters=iters, momentum=0).cpu().numpy()
    fast = dev["full"].cpu().numpy() if iters == 5 else gl.inv_spectrogram(spec, init_uniform=u, iters=iters, momentum=M).cpu().numpy()
    gl.set_momentum(0)
    assert fast.shape == (B, HOP * (T - 1)) and np.isfinite(fast).all()
    if iters == 1:
        assert np.array_equal(fast, plain)
    else:
        assert not np.array_equal(fast, plain)
    ep = max(_cmp(plain[b], _ref(5, b, T, iters, 0.0)) for b in range(B))
    ef = max(_cmp(fast[b], _ref(5, b, T, iters, M)) for b in range(B))
    bar = BAR if ep <= 8e-5 else 2.5 * ep
    print("iters %d: error over peak, plain loop %.3g, momentum 0.99 %.3g (bar %.3g)" % (iters, ep, ef, bar))
    assert ep < BAR, ep
    assert ef < bar, (ef, ep)


def test_even_bin_count_takes_the_paired_path():
    """num_freq 66: every offset of the estimate matrix is even and k_gl_project_fast reads and writes 8-byte words"""
    import taco_amd
    spec, u = _inputs(6, 66, 2, 12)
    g = taco_amd.GriffinLim(EVEN)
    plain = g.inv_spectrogram(spec, init_uniform=u, iters=3).cpu().numpy()
    fast = g.inv_spectrogram(spec, init_uniform=u, iters=3, momentum=M).cpu().numpy()
    g.close()
    for b in range(2):
        ep = _cmp(plain[b], FG.inv_spectrogram(spec[b].T, EVEN, u[b].T, iters=3))
        ef = _cmp(fast[b], FG.inv_spectrogram(spec[b].T, EVEN, u[b].T, iters=3, momentum=M))
        print("66 bins row %d: error over peak, plain loop %.3g, momentum 0.99 %.3g (bar %.3g)" % (b, ep, ef, BAR))
        assert ep < BAR and ef < (BAR if ep <= 8e-5 else 2.5 * ep), (ep, ef)


@pytest.mark.parametrize("flavor,hp", [("librosa", SMALL), ("librosa", EVEN), ("tensorflow", SMALL), ("tensorflow", EVEN)],
                         ids=["librosa-65", "librosa-66", "tensorflow-65", "tensorflow-66"])
def test_projection_kernel_alone_and_its_zero_rows(flavor, hp):
    """k_gl_project_fast through taco_debug_gl_project against the same arithmetic in float64 on the same float32 operands.  Bound per
    element, with e = 2^-24: the two components of z carry at most two roundings each, |dz| <= 2e(|est| + c|prev|) summed over both;
    a direction z / |z| moves by at most 2|dz| / |z|; the squares, their sum, the root, the quotient and the product add 6e.
    And the rule of the slack: where S = 0 the output is an exact zero although est and prev hold NaN and infinities there."""
    import torch, taco_amd
    from taco_amd import _lib
    g = taco_amd.GriffinLim(hp, flavor=flavor)
    Fq, R, c = hp.num_freq, 7, np.float32(M / (1 + M))
    rs = np.random.RandomState(Fq)
    est, prev = rs.randn(R, 2 * Fq).astype(np.float32), rs.randn(R, 2 * Fq).astype(np.float32)
    S = rs.rand(R, Fq).astype(np.float32) + 0.1
    S[2] = 0.0; S[5, ::3] = 0.0
    dead = S == 0
    for a, bad in ((est, np.nan), (prev, np.inf)):
        a[:, :Fq][dead] = bad; a[:, Fq:][dead] = -bad
    est[0, 3] = prev[0, 3] = est[0, Fq + 3] = prev[0, Fq + 3] = 0.0           # z = 0 on a live bin: angle(0) = 0, or the 1e-8 branch
    d = [torch.from_numpy(x).cuda() for x in (est, prev, S)]
    X = torch.full((R, 2 * Fq), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(g.device):
        _lib.check(g._lib.taco_debug_gl_project(g._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(d[0]), p(d[1]), p(d[2]), p(X), C.c_float(c), R))
    X = X.cpu().numpy()
    g.close()
    e64, p64, S64, c64, eps = est.astype(np.float64), prev.astype(np.float64), S.astype(np.float64), float(c), 2.0 ** -24
    with np.errstate(invalid="ignore", divide="ignore"):
        zr, zi = e64[:, :Fq] - c64 * p64[:, :Fq], e64[:, Fq:] - c64 * p64[:, Fq:]
        mag = np.sqrt(zr * zr + zi * zi)
        dz = 2 * eps * (np.abs(e64[:, :Fq]) + c64 * np.abs(p64[:, :Fq]) + np.abs(e64[:, Fq:]) + c64 * np.abs(p64[:, Fq:]))
        bound = S64 * (2 * dz / mag + 6 * eps)
        xr, xi = S64 * zr / mag, S64 * zi / mag
    assert np.all(X[:, :Fq][dead] == 0) and np.all(X[:, Fq:][dead] == 0)
    live = ~dead
    live[0, 3] = False                                         # z = 0: checked exactly below
    ratio = max(float((np.abs(X[:, :Fq] - xr)[live] / bound[live]).max()), float((np.abs(X[:, Fq:] - xi)[live] / bound[live]).max()))
    print("%s, %d bins: k_gl_project_fast vs float64, largest error over the derived bound %.3g; smallest |z| %.3g" % (flavor, Fq, ratio, float(mag[live].min())))
    assert np.isfinite(X).all() and ratio <= 1.0, ratio
    assert (X[0, 3], X[0, Fq + 3]) == ((0.0, 0.0) if flavor == "tensorflow" else (S[0, 3], 0.0))


# ---- 2. ragged rows ----
def test_ragged_rows_are_the_fast_loop_on_the_trimmed_spectrogram(dev):
    wav, ns = dev["ragged"].cpu().numpy(), dev["ns"]
    assert ns.tolist() == [HOP * (f - 1) for f in RAGGED]
    for b, f in enumerate(RAGGED):
        n = HOP * (f - 1)
        e = _cmp(wav[b, :n], _ref(5, b, f, 3, M))
        print("momentum 0.99, 3 iterations, row %d, %d of %d frames: error over peak %.3g (bar %.3g)" % (b, f, T, e, BAR))
        assert e < BAR, (b, f, e)
        assert np.all(wav[b, n:] == 0.0)                      # exact zeros past the row's own samples


# ---- 3. mel and TensorFlow flavours ----
def test_mel_vocoder_with_momentum(gl):
    from taco_amd import audio
    rs = np.random.RandomState(21)
    mel = (rs.rand(B, T, 12) * 1.2 - 0.1).astype(np.float32)
    u = rs.rand(B, T, F).astype(np.float32)
    inv = audio.inv_mel_basis(SMALL)
    wav, ns = gl.inv_melspectrogram(mel, init_uniform=u, iters=3, momentum=M)
    gl.set_momentum(0)
    wav = wav.cpu().numpy()
    assert ns.cpu().numpy().tolist() == [HOP * (T - 1)] * B
    for b in range(B):
        ref, lo = FG.inv_melspectrogram(mel[b], inv, SMALL, u[b], iters=3, momentum=M, return_min_z=True)
        e = _cmp(wav[b], ref)
        print("mel vocoder, momentum 0.99, 3 iterations, row %d: error over peak %.3g (bar %.3g), smallest |z| %.3g" % (b, e, BAR, lo))
        # the librosa normalisation branches only at z = 0 exactly (angle(0) = 0).  The mel magnitudes are small -- no ref_level_db, a
        # floor of 1e-10 -- and so is the smallest |z|, 4.2e-4 on these inputs: still three orders above the float32 rounding of a
        # z of this scale (1e-7), so no bin of the device can land on the branch that the restatement does not take
        assert lo > 1e-4, lo
        assert e < BAR, e


def test_tensorflow_flavour_with_momentum():
    import taco_amd
    spec, _ = _inputs(1)
    g = taco_amd.GriffinLim(SMALL, flavor="tensorflow", momentum=M)
    assert abs(g.momentum - M) < 1e-7
    wav, ns = g.inv_spectrogram_tensorflow(spec, iters=3)
    one, _ = g.inv_spectrogram_tensorflow(spec, iters=1)
    zero, _ = g.inv_spectrogram_tensorflow(spec, iters=1, momentum=0)
    assert g.momentum == 0.0 and np.array_equal(one.cpu().numpy(), zero.cpu().numpy())      # one iteration has no previous estimate
    g.close()
    wav = wav.cpu().numpy()
    assert wav.shape == (B, HOP * (T - 1) + 80)
    for b in range(B):
        ref, lo = FG.inv_spectrogram_tensorflow(spec[b], SMALL, iters=3, momentum=M, return_min_z=True)
        e = _cmp(wav[b], ref)
        print("TF flavour, momentum 0.99, 3 iterations, row %d: error over peak %.3g (bar %.3g), smallest |z| %.3g" % (b, e, BAR, lo))
        assert lo > 1e-3, lo                                   # far from the 1e-8 branch
        assert e < BAR, e


# ---- 4. the default is unchanged; determinism; capture ----
def test_momentum_zero_after_a_change_is_a_fresh_handle():
    import torch, taco_amd
    spec, u = _inputs(2)
    mel = (np.random.RandomState(4).rand(B, T, 12)).astype(np.float32)
    fr = np.array(RAGGED, np.int32)

    def three(lr, tf):
        return [lr.inv_spectrogram_rows(spec, fr, init_uniform=u, iters=3)[0].cpu().numpy(), lr.inv_melspectrogram(mel, fr, seed=3, iters=3)[0].cpu().numpy(),
                tf.inv_spectrogram_tensorflow(spec, fr, iters=3)[0].cpu().numpy()]

    lr, tf = taco_amd.GriffinLim(SMALL), taco_amd.GriffinLim(SMALL, flavor="tensorflow")
    lr.set_inv_mel_basis()
    fresh = three(lr, tf)
    size = lr._lib.taco_gl_rows_workspace_bytes(lr._h, B, T)
    for g in (lr, tf):
        g.set_momentum(M)
    assert lr._lib.taco_gl_rows_workspace_bytes(lr._h, B, T) > size
    moved = three(lr, tf)
    again = three(lr, tf)
    for g in (lr, tf):
        g.set_momentum(0)
    assert lr._lib.taco_gl_rows_workspace_bytes(lr._h, B, T) == size
    back = three(lr, tf)
    for a, m, m2, z in zip(fresh, moved, again, back):
        assert np.array_equal(a, z) and np.array_equal(m, m2) and not np.array_equal(a, m) and np.isfinite(m).all()
    lr.close(); tf.close()


def test_a_captured_fast_loop_replays_to_the_eager_bits(gl):
    import torch
    spec, u = _inputs(2)
    x, uu = torch.from_numpy(spec.copy()).cuda(), torch.from_numpy(u.copy()).cuda()
    fr = torch.tensor(RAGGED, dtype=torch.int32, device="cuda")
    a, na = gl.inv_spectrogram_rows(x, fr, init_uniform=uu, iters=3, momentum=M)
    a, na = a.clone(), na.clone()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):            # the workspace has its size from the call above: nothing is allocated by the library
            c, nc = gl.inv_spectrogram_rows(x, fr, init_uniform=uu, iters=3)
    torch.cuda.current_stream().wait_stream(side)
    gl.set_momentum(0)                                         # host state: the graph keeps the value it was captured with
    c.zero_(); nc.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, a) and torch.equal(nc, na)
    del graph


# ---- 5. the convergence kernels ----
def _sc_bound(D, S, sc):
    """|sc_device - sc| <= ETA * max|D| * sqrt(n) / ||S|| + 4 * 2^-23 * sc.  The device's |stft| differs from the float64 D = |stft(p)|
    by at most ETA x the frame's peak per element (the bar tests/test_gpu_spec.py holds the same analysis product to), so by the
    triangle inequality the norm of the difference moves by at most ETA * max|D| * sqrt(n), n the row's frames x bins; the second
    term covers the float32 sums, the quotient and the root."""
    return ETA * float(D.max()) * np.sqrt(D.size) / float(np.linalg.norm(S)) + 4 * 2.0 ** -23 * sc


@pytest.mark.parametrize("which,frames", [("full", (T,) * B), ("ragged", RAGGED)])
@pytest.mark.parametrize("kind", ["normalised", "magnitude"])
def test_convergence_matches_float64_on_the_downloaded_waveform(gl, dev, which, frames, kind):
    import torch
    spec, _ = _inputs(5)
    wav = dev[which]
    fr = None if which == "full" else np.array(frames, np.int32)
    mags = FG.magnitudes(spec.transpose(0, 2, 1), SMALL).transpose(0, 2, 1).astype(np.float32)      # [B, T, F], what kind "magnitude" is given
    target = spec if kind == "normalised" else mags
    sc = gl.convergence(target, wav, fr, kind=kind)
    assert sc.dtype == torch.float32 and tuple(sc.shape) == (B,)
    sc = sc.cpu().numpy().astype(np.float64)
    y = wav.cpu().numpy()
    for b, f in enumerate(frames):
        S = FG.magnitudes(spec[b, :f].T, SMALL) if kind == "normalised" else mags[b, :f].T.astype(np.float64)
        yb = y[b, :HOP * (f - 1)]
        D = FG.analysed_magnitudes(yb, SMALL)
        ref = FG.spectral_convergence(yb, S, SMALL)
        bound = _sc_bound(D, S, ref)
        print("%s, kind %s, row %d (%d frames): device %.7g, float64 %.7g, |difference| %.3g (bound %.3g)" % (which, kind, b, f, sc[b], ref, abs(sc[b] - ref), bound))
        assert D.shape == (F, f) and 0.05 < ref < 2.0
        assert abs(sc[b] - ref) <= bound, (b, sc[b], ref, bound)


def test_convergence_edges_determinism_and_row_independence(gl, dev):
    import torch
    spec, _ = _inputs(5)
    x = torch.from_numpy(spec.copy()).cuda()
    wav = dev["ragged"]
    fr = torch.tensor(RAGGED, dtype=torch.int32, device="cuda")
    assert gl.min_frames() == RAGGED[1]                        # row 1 sits at the clamp
    a = gl.convergence(x, wav, fr).clone()
    b = gl.convergence(x, wav, fr).clone()
    assert torch.equal(a, b) and bool(torch.isfinite(a).all()) and bool((a > 0).all())
    clamped = gl.convergence(x, wav, torch.tensor([99, -4, 20], dtype=torch.int32, device="cuda"))      # clamped as the vocoder clamps
    assert torch.equal(clamped, a)
    # a silent target: den = 0 -> exactly 0, and the other rows keep their bits
    mags = torch.from_numpy(FG.magnitudes(spec.transpose(0, 2, 1), SMALL).transpose(0, 2, 1).astype(np.float32)).cuda()
    loud = gl.convergence(mags, wav, fr, kind="magnitude").clone()
    quiet = mags.clone(); quiet[1] = 0.0
    q = gl.convergence(quiet, wav, fr, kind="magnitude").clone()
    assert float(q[1]) == 0.0 and torch.equal(q[[0, 2]], loud[[0, 2]])
    # another row's waveform and target change nothing of this row's result
    x2, w2 = x.clone(), wav.clone()
    x2[1] = x[0]; w2[1] = wav[2]
    other = gl.convergence(x2, w2, fr)
    assert torch.equal(other[[0, 2]], a[[0, 2]]) and float(other[1]) != float(a[1])
    # capture
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            c = gl.convergence(x, wav, fr)
    torch.cuda.current_stream().wait_stream(side)
    c.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(c, a)
    del graph
    with pytest.raises(Exception, match="wav"):
        gl.convergence(x, wav[:, :-1], fr)
    import taco_amd
    with pytest.raises(taco_amd._lib.TacoError) as e:
        gl.convergence(x, wav, fr, kind="decibel")
    assert e.value.code == taco_amd._lib.TACO_ERR_ARG


# ---- 6. quality ----
def test_momentum_at_30_iterations_beats_the_plain_loop_at_60():
    """The 129-bin consistent spectrogram of test_gpu_audio.test_full_iterations_reach_the_same_spectral_consistency, initial phases of
    seeds 9 and 2 as one batch.  In float64 momentum 0.99 at 30 iterations is 0.038 and 0.031 below the plain loop at 60
    (tests/test_fast_gl_host.py), more than the 0.03 within which the device's result must agree with the restatement's."""
    import taco_amd
    cases = [FG.consistent_case(seed) for seed in (9, 2)]
    spec = np.stack([c[0].T for c in cases]).astype(np.float32)              # [2, T, F]
    u = np.stack([c[2].T for c in cases]).astype(np.float32)
    g = taco_amd.GriffinLim(CONSISTENT)
    fast = g.inv_spectrogram(spec, init_uniform=u, iters=30, momentum=M)
    sc_fast = g.convergence(spec, fast).cpu().numpy()
    plain = g.inv_spectrogram(spec, init_uniform=u, iters=60, momentum=0)
    sc_plain = g.convergence(spec, plain).cpu().numpy()
    g.close()
    fast = fast.cpu().numpy()
    for b, seed in enumerate((9, 2)):
        target = FG.magnitudes(spec[b].T, CONSISTENT)
        ref = FG.spectral_convergence(FG.inv_spectrogram(spec[b].T, CONSISTENT, u[b].T, iters=30, momentum=M), target, CONSISTENT)
        got = FG.spectral_convergence(fast[b], target, CONSISTENT)
        print("seed %d: momentum 0.99 at 30 iterations, device %.4f (its own report %.4f), restatement %.4f; plain loop at 60 on the device %.4f"
              % (seed, got, sc_fast[b], ref, sc_plain[b]))
        assert abs(got - ref) < 0.03, (got, ref)
        assert sc_fast[b] < sc_plain[b], (sc_fast[b], sc_plain[b])


# ---- 7. Synthesizer.synthesize_audio(momentum=, return_convergence=) ----
def test_synthesizer_surface(tmp_path):
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
    got = s.synthesize_audio(tokens=ids, momentum=M, iters=3, return_convergence=True, pcm=False)
    frames = torch.from_numpy(np.asarray(s.spec_end_idx, np.int32)).cuda()
    g = taco_amd.GriffinLim(s.hparams)
    wav, ns = g.inv_spectrogram_rows(s.model.linear_outputs, frames, iters=3, momentum=M)
    sc = g.convergence(s.model.linear_outputs, wav, frames).cpu().numpy()
    wav, ns = wav.cpu().numpy(), ns.cpu().numpy()
    assert len(got) == 2 and all(a.dtype == np.float32 and np.array_equal(a, x[:n]) for a, x, n in zip(got, wav, ns))
    assert s.convergence.shape == (2,) and s.convergence.dtype == np.float32 and np.isfinite(s.convergence).all() and (s.convergence > 0).all()
    assert np.array_equal(s.convergence, sc)
    plain = s.synthesize_audio(tokens=ids, momentum=0, iters=3, pcm=False)
    assert s.convergence is None and not all(np.array_equal(a, b) for a, b in zip(plain, got))
    g.set_momentum(0)
    assert all(np.array_equal(a, x[:n]) for a, x, n in zip(plain, g.inv_spectrogram_rows(s.model.linear_outputs, frames, iters=3)[0].cpu().numpy(), ns))
    g.close()
    s.synthesize_audio(tokens=ids, vocoder="mel", momentum=M, iters=3, return_convergence=True)
    assert s.convergence.shape == (2,) and np.isfinite(s.convergence).all() and (s.convergence > 0).all()
    with pytest.raises(taco_amd._lib.TacoError) as e:
        s.synthesize_audio(tokens=ids, vocoder="tensorflow", return_convergence=True)
    assert e.value.code == taco_amd._lib.TACO_ERR_ARG
    assert len(s.synthesize_audio(tokens=ids, vocoder="tensorflow", momentum=M, iters=2)) == 2
    s.close()
