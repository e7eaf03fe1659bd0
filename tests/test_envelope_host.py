"""The spectral envelope and the pitch / formant shift, the host side (CPU): the NumPy restatement tests/envelope_reference.py on
hand-worked cases and on a synthetic voiced frame (the property the feature exists for: the formants stay where the pitch moves), the C
entry points with their prototypes and declarations, every argument error of taco_envelope_create / taco_spec_envelope /
taco_spec_warp_formant -- all returned before the first device call, so they are reached here --, the two fp32 tables bit for bit, and
the TACO_ERR_ARG cases of Synthesizer.synthesize_audio's new keywords on a Synthesizer without a model."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import envelope_reference as E
import warp_reference as R
from taco_amd import _lib, prosody

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = dict(src=np.zeros((1, 1), np.int32), frac=np.zeros((1, 1), np.int32), out_frames=np.ones(1, np.int32))      # one frame, copied


# ---- the restatement on hand-worked cases ----
def test_a_constant_frame_is_its_own_envelope():
    for W, Q in ((3, 1), (9, 4), (130, 49)):
        A, S = E.tables(W, Q)
        c, env, e = E.separate(np.full((1, W), 0.625, np.float32), A, S, np.float64)
        assert abs(c[0, 0] - 0.625) < 1e-7 and np.abs(c[0, 1:]).max(initial=0) < 1e-7                # the weights w_k / M sum to 1
        assert np.abs(env - 0.625).max() < 1e-6 and np.abs(e).max() < 1e-6


def test_a_single_cosine_is_kept_by_four_coefficients_and_removed_by_three():
    W = 33
    M = W - 1
    v = np.cos(np.pi * 3 * np.arange(W) / M).astype(np.float32)[None]
    A, S = E.tables(W, 4)
    c, env, e = E.separate(v, A, S, np.float64)
    assert np.abs(c[0] - [0, 0, 0, 0.5]).max() < 1e-7                                                # a_3 = 2 brings the half back
    assert np.abs(env - v).max() < 1e-6 and np.abs(e).max() < 1e-6
    A, S = E.tables(W, 3)
    c, env, e = E.separate(v, A, S, np.float64)
    assert np.abs(c).max() < 1e-7 and np.abs(env).max() < 1e-6 and np.abs(e - v).max() < 1e-6


def test_the_cepstrum_is_the_inverse_fft_of_the_even_extension_and_full_order_gives_the_frame_back():
    rs = np.random.RandomState(0)
    for W in (3, 10, 130, 1025):
        v = rs.rand(4, W).astype(np.float32)
        A, S = E.tables(W, W - 1)
        c = E.separate(v, A, S, np.float64)[0]
        ext = np.concatenate([v, v[:, -2:0:-1]], axis=1).astype(np.float64)                          # length 2 M, even
        assert ext.shape[1] == 2 * (W - 1)
        ref = np.fft.ifft(ext, axis=1).real[:, :W - 1]
        assert np.abs(c - ref).max() < 2e-7, W
        # Q = W with the last a halved: the DCT-I pair
        A64, S64 = E.tables64(W, W - 1)
        b = E.cosine_basis(W, W)
        w = np.ones(W); w[0] = w[-1] = 0.5
        a = np.full(W, 2.0); a[0] = a[-1] = 1.0
        full = ((v.astype(np.float64) @ ((w[None, :] * b) / (W - 1)).T) @ (a[:, None] * b))
        assert np.abs(full - v).max() < 1e-12, W


def test_the_float32_restatement_is_exact_on_the_exact_tier():
    """Q = 1, W - 1 a power of two, multiples of 2^-8 in [0, 1): every product and every sum is exact, env is the weighted mean"""
    rs = np.random.RandomState(1)
    for W in (3, 65, 1025, 2049):
        v = (rs.randint(0, 256, size=(5, W)) / 256.0).astype(np.float32)
        A, S = E.tables(W, 1)
        c32, env32, e32 = E.separate(v, A, S, np.float32)
        c64, env64, e64 = E.separate(v, A, S, np.float64)
        assert c32.dtype == np.float32 and np.array_equal(c32, c64) and np.array_equal(env32, env64) and np.array_equal(e32, e64)
        mean = (v.astype(np.float64).sum(1) - 0.5 * (v[:, 0].astype(np.float64) + v[:, -1])) / (W - 1)
        assert np.array_equal(env64, np.repeat(mean[:, None], W, 1))


# ---- the property: pitch moves, formants stay ----
def _voiced(W):
    """three Gaussian formants on a sloped floor, and harmonics 15 bins apart"""
    k = np.arange(W)
    smooth = 0.55 - 0.3 * k / W
    for centre, amp, width in ((60, 0.35, 14.0), (170, 0.25, 20.0), (300, 0.2, 26.0)):
        smooth = smooth + amp * np.exp(-0.5 * ((k - centre) / width) ** 2)
    return (smooth + 0.12 * np.cos(2 * np.pi * k / 15)).astype(np.float32)


def _peaks(env):
    return [lo + int(np.argmax(env[lo:hi])) for lo, hi in ((30, 110), (120, 250), (250, 400))]


def _spacing(e, n=600):
    seg = e[:n] - e[:n].mean()
    ac = np.correlate(seg, seg, "full")[n - 1:]
    return 5 + int(np.argmax(ac[5:40]))


def test_the_formants_stay_where_the_pitch_moves():
    W, Q = 1025, 49
    x = _voiced(W)
    A, S = E.tables(W, Q)
    _, env, e = E.separate(x[None], A, S, np.float64)
    orig = _peaks(env[0])
    assert all(abs(p - q) <= 2 for p, q in zip(orig, (60, 170, 300))) and _spacing(e[0]) == 15
    for semitones in (4, -4):
        s = prosody.semitones_to_scale(semitones)
        out = E.warp_formant(x[None, None], None, IDENTITY, A, S, pitch_scale=s, formant_scale=prosody.semitones_to_scale(0))
        _, env2, e2 = E.separate(out[0].astype(np.float32), A, S, np.float64)
        kept = _peaks(env2[0])
        assert all(abs(p - q) <= 1 for p, q in zip(kept, orig)), (semitones, kept, orig)              # the voice stays
        assert _spacing(e2[0]) == int(round(15 / float(s))) and _spacing(e2[0]) in (19, 12)            # the pitch moves
        plain = R.warp64(x[None, None], None, IDENTITY, s)                                             # the plain bin-axis scale moves both
        _, env3, e3 = E.separate(plain[0].astype(np.float32), A, S, np.float64)
        moved = _peaks(env3[0])[:2]
        assert all(abs(p - c / float(s)) <= 3 and abs(p - o) > 10 for p, o, c in zip(moved, orig, (60, 170))), (semitones, moved)
        assert _spacing(e3[0]) == int(round(15 / float(s)))
        # and the other way round: the formants move, the harmonics stay
        out = E.warp_formant(x[None, None], None, IDENTITY, A, S, pitch_scale=None, formant_scale=s)
        _, env4, e4 = E.separate(out[0].astype(np.float32), A, S, np.float64)
        assert all(abs(p - c / float(s)) <= 3 for p, c in zip(_peaks(env4[0])[:2], (60, 170))) and _spacing(e4[0]) == 15


def test_equal_scales_are_the_plain_warp_and_a_zero_lifter_is_it_on_the_bits():
    rs = np.random.RandomState(2)
    B, T, W, Q = 2, 6, 40, 7
    x = rs.rand(B, T, W).astype(np.float32)
    m = R.warp_map([6, 4], T, 1, 14, row_stretch=np.float32(1.7))
    s = np.array([0.8, 1.3], np.float32)
    A, S = E.tables(W, Q)
    assert np.abs(E.warp_formant(x, [6, 4], m, A, S, s, s) - R.warp64(x, [6, 4], m, s)).max() < 1e-12
    A0, S0 = E.tables(W, Q, lifter=np.zeros(Q))
    assert not S0.any()
    for fs in (None, s[::-1]):
        got = E.warp_formant(x, [6, 4], m, A0, S0, s, fs, dt=np.float32)
        assert np.array_equal(got.view(np.int32), R.warp32(x, [6, 4], m, s).view(np.int32))


# ---- the C ABI ----
def _info():
    out = (C.c_int * 8)()
    assert _lib.load_library().taco_debug_envelope_info(out, 8) == 0
    return list(out)


def test_symbols_prototypes_and_declarations():
    lib = _lib.load_library()
    pub = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    dbg = open(os.path.join(ROOT, "include", "taco_debug.h")).read()
    for name, nargs, text in (("taco_envelope_create", 6, pub), ("taco_envelope_destroy", 1, pub), ("taco_envelope_width", 1, pub),
                              ("taco_envelope_order", 1, pub), ("taco_envelope_tables", 3, pub), ("taco_spec_envelope", 8, pub),
                              ("taco_spec_warp_formant", 13, pub), ("taco_debug_envelope_info", 2, dbg)):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "taco_debug_envelope" not in pub and "typedef struct taco_envelope taco_envelope;" in pub
    assert pub.index("int taco_spec_warp(void*") < pub.index("taco_envelope_create(int") < pub.index("taco_stop_steps(void*")
    doc = pub[pub.index("the spectral envelope of a frame"):pub.index("typedef struct taco_envelope")]
    for phrase in ("NOT in the reference", "A[n, k] = fp32((w_k * basis[n, k]) / M)", "S[n, k] = fp32((a_n * l[n]) * basis[n, k])",
                   "G(env, formant_scale[b])[k] + G(e, pitch_scale[b])[k]", "outside stream capture", "W > 2304", "Q > 128"):
        assert phrase in doc, phrase
    warp_doc = pub[pub.index("rate, per-token duration and pitch control"):pub.index("size_t taco_spec_warp_workspace_bytes")]
    assert "formant-preserving" not in warp_doc and "waveform-domain stretching" in warp_doc           # the gap the header named is closed
    rows, wave, tile, kstep, wmax, w16, rows_wide, qmax = _info()
    assert (rows, wave, tile, kstep, qmax) == (16, 64, 16, 4, 128) and wmax >= 2049 and w16 < wmax and rows_wide < rows
    for w in range(qmax + 1, wmax + 1):                      # the LDS plan holds at every width: v, then env or the eight waves' partial sums, then c
        wp, r = -(-w // tile) * tile, rows if w <= w16 else rows_wide
        assert 4 * (r * (wp + 4) + max(r * (wp + 4), 8 * tile * qmax) + tile * (qmax + 4)) <= 160 * 1024, w
    assert lib.taco_debug_envelope_info(None, 3) == _lib.TACO_ERR_ARG and lib.taco_debug_envelope_info((C.c_int * 3)(), -1) == _lib.TACO_ERR_ARG
    import taco_amd
    assert taco_amd.warp_formant is prosody.warp_formant
    assert list(inspect.signature(prosody.envelope).parameters) == ["spec", "frames", "order", "lifter", "return_cepstrum"]
    assert list(inspect.signature(prosody.warp_formant).parameters) == ["spec", "frames", "map", "pitch_scale", "formant_scale", "order", "lifter"]
    assert list(inspect.signature(prosody.warp).parameters) == ["spec", "frames", "map", "freq_scale"]
    p = inspect.signature(taco_amd.Synthesizer.synthesize_audio).parameters
    assert [p[k].default for k in ("formant", "envelope_order")] == [None, None]
    assert prosody.default_order(24000) == 48 and prosody.default_order(16000) == 32
    assert np.array_equal(prosody.cosine_basis(130, 49), E.cosine_basis(130, 49))


def _create(W, Q, basis="auto", lifter=None, out="auto"):
    lib = _lib.load_library()
    if isinstance(basis, str):
        basis = E.cosine_basis(max(W, 2), max(Q, 1))
    basis = None if basis is None else np.ascontiguousarray(basis, np.float64)
    lifter = None if lifter is None else np.ascontiguousarray(lifter, np.float64)
    h = C.c_void_p()
    rc = lib.taco_envelope_create(W, Q, None if basis is None else basis.ctypes.data_as(C.c_void_p),
                                  None if lifter is None else lifter.ctypes.data_as(C.c_void_p), 0, C.byref(h) if out == "auto" else None)
    return rc, h


def test_every_argument_error_is_returned_without_a_device():
    """The pointers are host arrays: a call that passed the checks would hand them to a kernel, so every call here must fail first."""
    lib = _lib.load_library()
    ARG, UNSUP = _lib.TACO_ERR_ARG, _lib.TACO_ERR_UNSUPPORTED
    wmax, qmax = _info()[4], _info()[7]
    assert _create(9, 4, basis=None)[0] == ARG and b"null" in lib.taco_last_error()
    assert _create(9, 4, out=None)[0] == ARG and b"null" in lib.taco_last_error()
    for W, Q in ((2, 1), (0, 1), (-5, 1), (9, 0), (9, -1), (9, 9), (9, 100), (3, 3)):
        assert _create(W, Q)[0] == ARG and b"Q <= W - 1" in lib.taco_last_error(), (W, Q)
    for bad in (np.nan, np.inf, -np.inf, 1.0000001, -1.5):
        b = E.cosine_basis(9, 4)
        b[2, 5] = bad
        assert _create(9, 4, basis=b)[0] == ARG and b"host_basis[2, 5]" in lib.taco_last_error(), bad
    for bad in (np.nan, np.inf, -np.inf):
        assert _create(9, 4, lifter=[1.0, 1.0, bad, 1.0])[0] == ARG and b"host_lifter[2]" in lib.taco_last_error(), bad
    assert _create(300, qmax + 1)[0] == UNSUP and b"Q = 129" in lib.taco_last_error()
    assert _create(wmax + 1, 5)[0] == UNSUP and b"W = " in lib.taco_last_error()
    assert _create(wmax + 1, 0)[0] == ARG                                                           # argument errors come first

    rc, h = _create(7, 3)
    assert rc == 0 and lib.taco_envelope_width(h) == 7 and lib.taco_envelope_order(h) == 3
    assert lib.taco_envelope_width(None) == 0 and lib.taco_envelope_order(None) == 0
    A = np.zeros((3, 7), np.float32)
    P = lambda x, off=0: None if x is None else C.c_void_p(x.ctypes.data + off)
    assert lib.taco_envelope_tables(None, P(A), P(A)) == ARG and lib.taco_envelope_tables(h, None, P(A)) == ARG and lib.taco_envelope_tables(h, P(A), None) == ARG
    B, T, T_out, W, Q = 2, 5, 9, 7, 3
    spec, frames = np.zeros((B, T, W), np.float32), np.zeros(B, np.int32)
    env, cep = np.zeros((B, T, W), np.float32), np.zeros((B, T, Q), np.float32)

    def ecall(**kw):
        v = dict(h=h, spec=P(spec), frames=P(frames), B=B, T=T, env=P(env), cep=P(cep))
        v.update(kw)
        return lib.taco_spec_envelope(v["h"], None, v["spec"], v["frames"], v["B"], v["T"], v["env"], v["cep"])

    for kw in (dict(h=None), dict(spec=None), dict(env=None), dict(env=None, cep=None)):
        assert ecall(**kw) == ARG and b"null" in lib.taco_last_error(), kw
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T=-7)):
        assert ecall(**kw) == ARG and b">= 1" in lib.taco_last_error(), kw
    for kw in (dict(env=P(spec)), dict(env=P(spec, spec.nbytes - 4)), dict(cep=P(spec)), dict(cep=P(env, env.nbytes - 4)), dict(env=P(cep, 8)),
               dict(env=P(frames, 4)), dict(cep=P(frames)), dict(spec=P(env, 16)), dict(B=2 ** 31 - 1, T=2 ** 31 - 1)):
        assert ecall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw

    src, frac, of = np.zeros((B, T_out), np.int32), np.zeros((B, T_out), np.int32), np.zeros(B, np.int32)
    ps, fs, out = np.ones(B, np.float32), np.ones(B, np.float32), np.zeros((B, T_out, W), np.float32)

    def wcall(**kw):
        v = dict(h=h, spec=P(spec), frames=P(frames), src=P(src), frac=P(frac), of=P(of), ps=P(ps), fs=P(fs), B=B, T=T, T_out=T_out, out=P(out))
        v.update(kw)
        return lib.taco_spec_warp_formant(v["h"], None, v["spec"], v["frames"], v["src"], v["frac"], v["of"], v["ps"], v["fs"], v["B"], v["T"],
                                          v["T_out"], v["out"])

    for kw in (dict(h=None), dict(spec=None), dict(src=None), dict(frac=None), dict(of=None), dict(out=None)):
        assert wcall(**kw) == ARG and b"null" in lib.taco_last_error(), kw
    for kw in (dict(B=0), dict(T=0), dict(T_out=0), dict(T_out=-3), dict(B=-2)):
        assert wcall(**kw) == ARG and b">= 1" in lib.taco_last_error(), kw
    for kw in (dict(out=P(spec)), dict(out=P(spec, spec.nbytes - 4)), dict(out=P(frames, 4)), dict(out=P(src)), dict(out=P(frac, frac.nbytes - 4)),
               dict(out=P(of)), dict(out=P(ps, 4)), dict(out=P(fs)), dict(spec=P(out, out.nbytes - 4)), dict(fs=P(out, 12)), dict(ps=P(out)),
               dict(B=2 ** 31 - 1, T=2 ** 31 - 1, T_out=2 ** 31 - 1)):
        assert wcall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw
    assert wcall(ps=None, fs=None, out=P(src)) == ARG and b"overlap" in lib.taco_last_error()
    lib.taco_envelope_destroy(h)
    lib.taco_envelope_destroy(None)


@pytest.mark.parametrize("W,Q", [(3, 1), (3, 2), (130, 49), (1025, 49), (2049, 128)])
def test_the_tables_are_the_restatements_rounded_once(W, Q):
    lib = _lib.load_library()
    rs = np.random.RandomState(W + Q)
    for lifter in (None, rs.uniform(-1.5, 1.5, size=Q), np.zeros(Q), 0.5 + 0.5 * np.cos(np.pi * np.arange(Q) / Q)):
        rc, h = _create(W, Q, lifter=lifter)
        assert rc == 0
        A, S = np.full((Q, W), 7, np.float32), np.full((Q, W), 7, np.float32)
        assert lib.taco_envelope_tables(h, A.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p)) == 0
        lib.taco_envelope_destroy(h)
        wantA, wantS = E.tables(W, Q, lifter)
        assert np.array_equal(A.view(np.int32), wantA.view(np.int32)) and np.array_equal(S.view(np.int32), wantS.view(np.int32))
        e = prosody.Envelope(W, Q, lifter)                                                           # the package's handle: no device is touched
        gotA, gotS = e.tables()
        e.close()
        assert np.array_equal(gotA.view(np.int32), wantA.view(np.int32)) and np.array_equal(gotS.view(np.int32), wantS.view(np.int32))
    assert abs(float(wantA[0].astype(np.float64).sum()) - 1.0) < 1e-6


def test_the_envelope_class_refuses_what_the_library_refuses():
    for W, Q, code in ((2, 1, _lib.TACO_ERR_ARG), (9, 9, _lib.TACO_ERR_ARG), (9, 0, _lib.TACO_ERR_ARG), (300, 129, _lib.TACO_ERR_UNSUPPORTED),
                       (2305, 5, _lib.TACO_ERR_UNSUPPORTED)):
        with pytest.raises(_lib.TacoError) as e:
            prosody.Envelope(W, Q)
        assert e.value.code == code, (W, Q)
    with pytest.raises(_lib.TacoError) as e:
        prosody.Envelope(9, 4, lifter=[1.0, 2.0])
    assert e.value.code == _lib.TACO_ERR_SHAPE
    with pytest.raises(_lib.TacoError) as e:
        prosody.Envelope(9, 4, lifter=[1.0, np.nan, 1.0, 1.0])
    assert e.value.code == _lib.TACO_ERR_ARG


# ---- Python ----
def test_the_new_keywords_are_refused_before_the_model_is_touched():
    """Every refusal comes before the forward, so a Synthesizer without a model shows them."""
    import taco_amd
    s = taco_amd.Synthesizer()
    ids = np.array([[5, 6, 7, 1], [8, 9, 1, 0]])
    bad = [dict(formant=2.0, vocoder="mel"), dict(formant=0.0, vocoder="mel", rate=1.0), dict(formant=[1.0, 2.0], pitch=1.0, vocoder="mel"),
           dict(formant=float("nan")), dict(formant=float("inf")), dict(formant=[1.0, float("-inf")]), dict(formant=[1.0]),
           dict(formant=[1.0, 2.0, 3.0]), dict(formant=[[1.0, 2.0]]), dict(formant="dark"),
           dict(envelope_order=48), dict(envelope_order=48, pitch=2.0), dict(formant=0.0, envelope_order=-1), dict(formant=0.0, envelope_order=2.5),
           dict(formant=1.0, pitch=float("nan")), dict(formant=1.0, pitch=[1.0]), dict(formant=1.0, rate=0.0)]
    for kw in bad:
        with pytest.raises(_lib.TacoError) as e:
            s.synthesize_audio(tokens=ids, **kw)
        assert e.value.code == _lib.TACO_ERR_ARG, kw
    for kw in (dict(formant=0.0), dict(formant=[-2.0, 1.5], pitch=3), dict(formant=-2, rate=[1.0, 2.0], envelope_order=20, vocoder="tensorflow")):
        with pytest.raises(AttributeError):                                     # past the checks: the first use of the model that is not there
            s.synthesize_audio(tokens=ids, **kw)
    assert s._formant_args(2, None, None, "mel") is None
    sc = s._formant_args(2, [12, -12], None, "griffin_lim")
    assert sc.dtype == np.float32 and sc.tolist() == [0.5, 2.0] and s._formant_args(3, 0.0, 7, "tensorflow").tolist() == [1.0, 1.0, 1.0]
