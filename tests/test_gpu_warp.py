"""Rate, per-token duration and pitch control on the spectrogram on the device (taco_spec_warp_map, taco_spec_warp: csrc/taco_warp.h)
against the NumPy restatement tests/warp_reference.py: the integer map as integer equality at every size at which k_warp_map changes
path, the warp on the bits where fp32 is exact, the identity, random data against float64 within a derived bound (and against the float32
restatement on the bits), graph replay, and Synthesizer.synthesize_audio(rate=, token_stretch=, pitch=, return_durations=).

THE BOUND of the random tier, u = 2^-24, M = max |x|, data in [0, M] so that |x1 - x0| <= M.  The inputs are fp32 and enter the float64
restatement unchanged, the map is the same integers, w_t = frac * 2^-16 and w_f = q - k0 (q = fp32(k * c) in both) are exact: only the
interpolation's arithmetic differs, and the order is fixed -- time first, then frequency, every operation rounded on its own.
  time:       d = fl(x1 - x0), |d - (x1 - x0)| <= u M;  p = fl(w_t d), |p - w_t (x1 - x0)| <= 2 u M (1 + u);  v' = fl(x0 + p), whose exact sum
              is at most M (1 + 2 u): |v' - v| <= 3 u M + O(u^2 M).  Without a frequency scale that is the output: bound 4 u M.
  frequency:  the exact formula on the perturbed v0', v1' is a convex combination: off by at most 3 u M.  Its own three roundings, on values
              of magnitude at most M (1 + 6 u), add u M, u M and u M as above: |out' - out| <= 6 u M + O(u^2 M).  Bound 7 u M.
Every element is held to it; none is left out."""
import ctypes as C

import numpy as np
import pytest

import warp_reference as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def _mods():
    import torch
    from taco_amd import _lib, prosody
    return torch, _lib, prosody


def _info():
    from taco_amd import _lib
    out = (C.c_int * 4)()
    assert _lib.load_library().taco_debug_warp_info(out, 4) == 0
    return list(out)                       # scan chunk, wave width, output rows per workgroup, widest row staged in LDS


def _up(x, dtype=None):
    import torch
    return None if x is None else torch.as_tensor(np.asarray(x, dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _map(frames, T, r, T_out, al=None, row=None, tok=None, token_frames=False):
    """the device map as host arrays"""
    torch, _, prosody = _mods()
    m = prosody.warp_map(_up(frames, np.int32), T, r, _up(al, np.float32), _up(row, np.float32), _up(tok, np.float32), out_cap=T_out,
                         return_token_frames=token_frames, device="cuda")
    torch.cuda.synchronize()
    return m, dict(src=m.src.cpu().numpy(), frac=m.frac.cpu().numpy(), out_frames=m.out_frames.cpu().numpy(),
                   token_frames=None if m.token_frames is None else m.token_frames.cpu().numpy())


def _same_map(got, want, what):
    for k in ("src", "frac", "out_frames", "token_frames"):
        if k == "token_frames" and got[k] is None:                            # not asked for
            continue
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:5])


def _stretches(rs, shape):
    """arbitrary float32 stretches in [0.05, 20]: a row stretch times a token stretch spans [0.0025, 400], so both clamps bite"""
    return np.exp(rs.uniform(np.log(0.05), np.log(20.0), size=shape)).astype(np.float32)


def _alignments(rs, B, T_in, n):
    """random, with exact ties at the maximum and NaNs (several in a column: the first wins) planted in a fifth of the columns each"""
    al = rs.rand(B, T_in, n).astype(np.float32)
    if T_in > 1:
        for b in range(B):
            for s in rs.choice(n, size=max(1, n // 5), replace=False):
                e = rs.choice(T_in, size=min(T_in, 3), replace=False)
                al[b, e, s] = 2.0
            for s in rs.choice(n, size=max(1, n // 5), replace=False):
                e = rs.choice(T_in, size=min(T_in, 2), replace=False)
                al[b, e, s] = np.nan
    return al


# ---- 1. the map, as integer equality ----
@pytest.mark.parametrize("r", [1, 5])
@pytest.mark.parametrize("T_in", [1, 7, 70])
def test_map_equals_the_restatement(T_in, r):
    chunk, wave = _info()[:2]
    n = -(-(2 * chunk + 1) // r)
    T = n * r
    edges = [1] + [e + d for e in (wave, chunk, 2 * chunk) for d in (-1, 0, 1)]
    assert max(edges) <= T and len(edges) == 10
    rs = np.random.RandomState(1000 * T_in + r)
    B = 3
    al = _alignments(rs, B, T_in, n)
    low = high = 0
    for i, frames in enumerate([edges[0:3], edges[3:6], edges[6:9], [edges[9], 0, T + 7]]):      # the last two: clamped to 1 and to T
        row, tok = _stretches(rs, B), _stretches(rs, (B, T_in))
        T_out = 16 * T + 1
        want = R.warp_map(frames, T, r, T_out, alignments=al, row_stretch=row, token_stretch=tok)
        _, got = _map(frames, T, r, T_out, al, row, tok, token_frames=True)
        _same_map(got, want, (T_in, r, frames))
        d = np.concatenate([np.diff(np.concatenate([[0], c])) for c in want["C"]])
        low, high = low + int((d == R.D_MIN).sum()), high + int((d == R.D_MAX).sum())
        assert (want["token_frames"].sum(1) == want["f"]).all()
    assert low > 0 and high > 0                                                                    # both clamps were met


def test_map_with_a_small_capacity_null_frames_and_no_alignments():
    chunk, wave = _info()[:2]
    rs = np.random.RandomState(7)
    B, T_in, r = 3, 7, 5
    n = -(-(chunk + 70) // r)
    T = n * r
    al, row, tok = _alignments(rs, B, T_in, n), _stretches(rs, B), _stretches(rs, (B, T_in))
    frames = [T, chunk + 1, 33]
    full = R.warp_map(frames, T, r, 16 * T + 1, alignments=al, row_stretch=row, token_stretch=tok)
    T_out = int(np.sort(full["out_frames"])[1]) - 3                                                # cuts two rows, leaves one whole
    want = R.warp_map(frames, T, r, T_out, alignments=al, row_stretch=row, token_stretch=tok)
    assert sorted((want["out_frames"] == T_out).tolist()) == [False, True, True]
    _same_map(_map(frames, T, r, T_out, al, row, tok, True)[1], want, "small T_out")
    for T_out in (1, 2):
        _same_map(_map(frames, T, r, T_out, al, row, tok)[1], R.warp_map(frames, T, r, T_out, alignments=al, row_stretch=row, token_stretch=tok),
                  T_out)
    # d_frames NULL: every row keeps T
    want = R.warp_map(None, T, r, 16 * T + 1, alignments=al, row_stretch=row, token_stretch=tok)
    assert (want["f"] == T).all()
    _same_map(_map(None, T, r, 16 * T + 1, al, row, tok, True)[1], want, "NULL frames")
    # no alignments: the row stretch alone; no stretch at all: the identity
    want = R.warp_map(frames, T, r, 16 * T + 1, row_stretch=row)
    _same_map(_map(frames, T, r, 16 * T + 1, None, row)[1], want, "no alignments")
    ident = _map(frames, T, r, T + 2)[1]
    _same_map(ident, R.warp_map(frames, T, r, T + 2), "identity")
    assert ident["out_frames"].tolist() == frames and not ident["frac"].any()
    # alignments with only a row stretch, and only a token stretch
    _same_map(_map(frames, T, r, 16 * T + 1, al, row, None, True)[1], R.warp_map(frames, T, r, 16 * T + 1, alignments=al, row_stretch=row), "row only")
    _same_map(_map(frames, T, r, 16 * T + 1, al, None, tok)[1], R.warp_map(frames, T, r, 16 * T + 1, alignments=al, token_stretch=tok), "token only")


def test_the_default_capacity_comes_from_the_host_side_stretches():
    """out_cap = ceil(T * max row stretch * max token stretch) + 1, no device read; a stretch on the device needs an explicit one"""
    torch, L, prosody = _mods()
    B, T_in, r, n = 3, 4, 2, 20
    T = n * r
    rs = np.random.RandomState(9)
    al = _alignments(rs, B, T_in, n)
    row, tok = np.array([0.5, 1.25, 1.0], np.float32), rs.choice([0.5, 1.0, 1.5], size=(B, T_in)).astype(np.float32)
    tok[0, 0] = 1.5
    m = prosody.warp_map(None, T, r, _up(al), row, tok, return_token_frames=True)
    assert m.T_out == int(np.ceil(T * 1.25 * 1.5)) + 1 == tuple(m.src.shape)[1]
    want = R.warp_map(None, T, r, m.T_out, alignments=al, row_stretch=row, token_stretch=tok)
    got = dict(src=m.src.cpu().numpy(), frac=m.frac.cpu().numpy(), out_frames=m.out_frames.cpu().numpy(), token_frames=m.token_frames.cpu().numpy())
    _same_map(got, want, "default capacity")
    assert (want["out_frames"] < m.T_out).all()                                                    # no row was cut
    assert prosody.warp_map([T, 3, 9], T, r, device="cuda").T_out == T + 1 and prosody.warp_map(None, T, r, row_stretch=2.0, device="cuda").T_out == 2 * T + 1
    with pytest.raises(L.TacoError) as e:
        prosody.warp_map(None, T, r, _up(al), _up(row), tok)
    assert e.value.code == L.TACO_ERR_ARG
    tf = prosody.token_frames(_up(al), _up([T, 7, 1], np.int32), r).cpu().numpy()
    assert np.array_equal(tf, R.warp_map([T, 7, 1], T, r, 1, alignments=al)["token_frames"]) and tf.sum(1).tolist() == [T, 7, 1]


def test_map_stretches_that_are_not_numbers():
    B, T_in, r, n = 3, 4, 2, 40
    T = n * r
    rs = np.random.RandomState(3)
    al = _alignments(rs, B, T_in, n)
    row = np.array([np.nan, 1.0, -2.0], np.float32)
    tok = np.array([[1, 2, 3, 4], [np.inf, 0.0, np.nan, -1.0], [1e-45, 3e38, 0.5, 1]], np.float32)
    want = R.warp_map([T, T, 51], T, r, 16 * T + 1, alignments=al, row_stretch=row, token_stretch=tok)
    _same_map(_map([T, T, 51], T, r, 16 * T + 1, al, row, tok, True)[1], want, "NaN / inf / zero / negative / subnormal")
    assert want["out_frames"][0] == T // 16                                                       # a NaN row stretch: the floor throughout


# ---- 2. the warp on the bits where fp32 is exact ----
EXACT_T_IN, EXACT_R, EXACT_N = 5, 3, 12
SCALES = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0]


def _exact_case(W):
    """integer spectrogram in [-1024, 1024], token stretches from {0.5, 1, 2, 4}, frequency scales from {0.25 .. 2}: durations are 2^15 ..
    2^18 and prefix sums multiples of 2^15, so w_t is a multiple of 1/8 and w_f of 1/4; differences stay below 2^12: every product and sum
    is exact in 24 bits."""
    rs = np.random.RandomState(W)
    B, T = len(SCALES), EXACT_N * EXACT_R
    x = rs.randint(-1024, 1025, size=(B, T, W)).astype(np.float32)
    al = _alignments(rs, B, EXACT_T_IN, EXACT_N)
    tok = rs.choice([0.5, 1.0, 2.0, 4.0], size=(B, EXACT_T_IN)).astype(np.float32)
    frames = np.array([T, T - 1, 20, 7, 2, 1])
    return x, al, tok, frames, T


def _direct(x, frames, m, scale):
    """taco_debug_spec_warp_direct: the frequency gather from the cache at every width"""
    import torch
    from taco_amd import _device, _lib
    B, T, W = x.shape
    out = torch.empty((B, m.T_out, W), dtype=torch.float32, device=x.device)
    _device.call(x.device, _lib.load_library().taco_debug_spec_warp_direct, _device.STREAM, x, frames, m.src, m.frac, m.out_frames, scale, B, T, W,
                 m.T_out, out)
    return out


def test_the_exact_widths_sit_on_both_sides_of_the_staged_gather():
    assert _info()[3] == 2048                                                                      # the two widest cases of the next test


@pytest.mark.parametrize("W", [1, 63, 64, 65, 80, 1025, 2048, 2049])
def test_warp_is_bit_equal_on_exact_data(W):
    torch, _, prosody = _mods()
    x, al, tok, frames, T = _exact_case(W)
    T_out = 4 * T + 3
    want_map = R.warp_map(frames, T, EXACT_R, T_out, alignments=al, token_stretch=tok)
    m, got_map = _map(frames, T, EXACT_R, T_out, al, None, tok)
    _same_map(got_map, want_map, W)
    assert len(set(want_map["frac"].ravel().tolist())) >= 4 and want_map["out_frames"].max() > 2 * _info()[2]      # several workgroups per row
    dx, df = _up(x), _up(frames, np.int32)
    for scale in (None, np.array(SCALES, np.float32), np.array(SCALES[::-1], np.float32)):
        out, of = prosody.warp(dx, df, m, None if scale is None else _up(scale))
        out = out.cpu().numpy()
        ref = R.warp64(x, frames, want_map, scale)
        assert np.array_equal(ref, ref.astype(np.float32))                                         # the restatement met no rounding
        assert np.array_equal(ref, R.warp32(x, frames, want_map, scale))
        assert np.array_equal(_bits(out), _bits(ref)), (W, scale)
        if scale is not None:                                                                      # the other form of the gather: the same bits
            assert np.array_equal(_bits(_direct(dx, df, m, _up(scale)).cpu().numpy()), _bits(ref)), (W, "direct")
        assert np.array_equal(of.cpu().numpy(), want_map["out_frames"])


# ---- 3. the identity ----
@pytest.mark.parametrize("W", [7, 1025])
def test_stretch_one_copies_the_bits_and_reads_nothing_past_the_frames(W):
    torch, _, prosody = _mods()
    rs = np.random.RandomState(W)
    B, T = 4, 50
    frames = np.array([50, 31, 1, 8])
    x = rs.standard_normal((B, T, W)).astype(np.float32)
    x[0, 3, 0], x[0, 4, W - 1], x[1, 0, 0] = -0.0, np.float32(1e-42), np.float32(3e38)              # a signed zero, a subnormal, a large value
    planted = x.copy()
    for b, f in enumerate(frames):
        planted[b, f:] = np.nan                                                                     # every frame >= f
    dx, df = _up(planted), _up(frames, np.int32)
    for T_out, row in ((T, None), (T + 9, np.ones(B, np.float32))):
        m, got = _map(frames, T, 1, T_out, None, row)
        assert got["out_frames"].tolist() == frames.tolist()
        for scale in (None, np.ones(B, np.float32)):
            out = prosody.warp(dx, df, m, None if scale is None else _up(scale))[0].cpu().numpy()
            assert not np.isnan(out).any()
            for b, f in enumerate(frames):
                assert np.array_equal(_bits(out[b, :f]), _bits(x[b, :f])), (W, b)
                assert not _bits(out[b, f:]).any()                                                  # +0, not -0


# ---- 4. random data against float64 ----
@pytest.mark.parametrize("W", [80, 1025])
def test_random_data_stays_within_the_derived_bound(W):
    torch, _, prosody = _mods()
    rs = np.random.RandomState(100 + W)
    B, T_in, r, n = 4, 9, 4, 30
    T = n * r
    x = rs.rand(B, T, W).astype(np.float32)
    al = _alignments(rs, B, T_in, n)
    row, tok = _stretches(rs, B) ** 0.5, _stretches(rs, (B, T_in)) ** 0.5
    frames = np.array([T, 77, 13, 1])
    scale = np.array([0.8908987, 1.1224620, 0.3333, 2.7], np.float32)
    T_out = 21 * T
    want_map = R.warp_map(frames, T, r, T_out, alignments=al, row_stretch=row, token_stretch=tok)
    m, got_map = _map(frames, T, r, T_out, al, row, tok)
    _same_map(got_map, want_map, W)
    M = float(x.max())
    for sc, mult in ((None, 4), (scale, 7)):
        out = prosody.warp(_up(x), _up(frames, np.int32), m, None if sc is None else _up(sc))[0].cpu().numpy()
        ref = R.warp64(x, frames, want_map, sc)
        err, bound = float(np.abs(out - ref).max()), mult * U * M
        r32 = R.warp32(x, frames, want_map, sc)
        diff32 = int((_bits(out) != _bits(r32)).sum())
        print("W %d, %s: max |gpu - float64| %.3g, bound %d u M = %.3g (%.2f of it); elements that differ from the float32 restatement: %d of %d"
              % (W, "no scale" if sc is None else "scaled", err, mult, bound, err / bound, diff32, out.size))
        assert (np.abs(out - ref) <= bound).all()
        assert diff32 == 0


# ---- 5. graph capture and replay ----
def test_second_call_and_graph_replay_give_the_same_bits():
    torch, _, prosody = _mods()
    rs = np.random.RandomState(11)
    B, T_in, r, n, W = 3, 6, 2, 150, 33
    T = n * r
    x, al = _up(rs.rand(B, T, W), np.float32), _up(_alignments(rs, B, T_in, n))
    row, tok = _up(_stretches(rs, B) ** 0.5), _up(_stretches(rs, (B, T_in)) ** 0.5)
    frames, scale = _up([T, 200, 5], np.int32), _up([0.9, 1.0, 1.3], np.float32)

    def run():
        m = prosody.warp_map(frames, T, r, al, row, tok, out_cap=5 * T, return_token_frames=True)
        out, of = prosody.warp(x, frames, m, scale)
        return out, of, m.src, m.frac, m.token_frames

    first = [t.clone() for t in run()]
    outs = run()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                                      # one stream, one chain of two launches
        captured = run()
    for t in captured:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(captured, outs))                       # the buffer set of the shape, not new memory
    for a, b in zip(first, captured):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert int(first[1].max()) > T                                                                 # something was stretched


# ---- 6. end to end: Synthesizer.synthesize_audio ----
def test_synthesize_audio_rate_token_stretch_and_pitch(tmp_path):
    import taco_amd
    import taco_oracle as O
    from util import tiny_hp, to_product_hp
    torch, L, prosody = _mods()
    ohp = tiny_hp(num_freq=65, max_iters=20)
    hp = to_product_hp(ohp)
    hp.add_hparam("sample_rate", 1600); hp.add_hparam("griffin_lim_iters", 3)
    taco_amd.save_hparams(str(tmp_path), hp)
    taco_amd.weights.save_weights(str(tmp_path / "model.ckpt-1.safetensors"), O.init_weights(ohp, 1, 31))
    ids, _ = O.synthetic_inputs(2, 9, 41)
    s = taco_amd.Synthesizer().load(str(tmp_path), num_speakers=1)
    r = hp.reduction_factor

    def same(a, b):
        return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))

    # rate 1.0 is the call without the keyword, sample for sample
    plain = s.synthesize_audio(tokens=ids, seed=3)
    end = np.asarray(s.spec_end_idx).copy()
    assert s.warped_frames is None and s.token_frames is None
    T = s.model.linear_outputs.shape[1]
    gl = s._griffin_lim()
    print("trimmed frames %s of %d, the vocoder's smallest %d" % (end.tolist(), T, gl.min_frames()))
    assert (end >= gl.min_frames()).all()          # (a row below it is raised to it by the vocoder, which then reads frames the warp wrote as +0)
    one = s.synthesize_audio(tokens=ids, seed=3, rate=1.0, return_durations=True)
    assert same(plain, one)
    assert np.array_equal(s.spec_end_idx, end) and np.array_equal(s.warped_frames, np.clip(end, 1, T))
    assert s.token_frames.shape == ids.shape and np.array_equal(s.token_frames.sum(1), np.clip(end, 1, T))
    al = s.model.alignments.cpu().numpy()
    assert np.array_equal(s.token_frames, R.warp_map(end, T, r, 1, alignments=al)["token_frames"])
    assert same(s.synthesize_audio(tokens=ids, vocoder="tensorflow"), s.synthesize_audio(tokens=ids, vocoder="tensorflow", rate=[1.0, 1.0]))
    s.synthesize_audio(tokens=ids, return_durations=True)                                          # durations alone: nothing is warped
    assert s.warped_frames is None and np.array_equal(s.token_frames.sum(1), np.clip(end, 1, T))

    # rate 0.5: twice the frames, audio of the matching sample count
    slow = s.synthesize_audio(tokens=ids, seed=3, rate=0.5, pcm=False)
    want = R.warp_map(end, T, r, 2 * T, row_stretch=np.float32(2.0))["out_frames"]
    assert np.array_equal(s.warped_frames, want) and np.array_equal(want, 2 * np.clip(end, 1, T)) and np.array_equal(s.spec_end_idx, end)
    hop = gl.num_samples(2)
    assert [len(a) for a in slow] == [hop * (int(f) - 1) for f in np.clip(want, gl.min_frames(), 2 * T)]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() and np.abs(a).max() > 0 for a in slow)

    # per-token stretch and pitch: the warped frames are the restatement's on the model's own alignments
    stretch = [[2.0, 0.5, 1.0, 3.0], [0.25]]
    both = s.synthesize_audio(tokens=ids, seed=3, rate=[0.8, 1.25], token_stretch=stretch, pitch=[2.0, -3.0], return_durations=True)
    tok = np.ones(ids.shape, np.float32)
    tok[0, :4], tok[1, :1] = stretch[0], stretch[1]
    row = (1.0 / np.array([0.8, 1.25])).astype(np.float32)
    want = R.warp_map(end, T, r, prosody.out_frames_bound(T, row, tok), alignments=s.model.alignments.cpu().numpy(), row_stretch=row, token_stretch=tok)
    assert np.array_equal(s.warped_frames, want["out_frames"]) and np.array_equal(s.token_frames, want["token_frames"])
    assert [len(a) for a in both] == [hop * (int(f) - 1) for f in np.clip(want["out_frames"], gl.min_frames(), None)]
    mel = s.synthesize_audio(tokens=ids, seed=3, vocoder="mel", rate=0.5)
    assert np.array_equal(s.warped_frames, 2 * np.clip(end, 1, T)) and [len(a) for a in mel] == [len(a) for a in slow]
    with pytest.raises(L.TacoError) as e:
        s.synthesize_audio(tokens=ids, vocoder="mel", pitch=1.0)
    assert e.value.code == L.TACO_ERR_ARG
    s.close()
