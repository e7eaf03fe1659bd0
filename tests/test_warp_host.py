"""Rate, duration and pitch control on the spectrogram, the host side (CPU): the NumPy restatement tests/warp_reference.py on hand-worked
cases, the C entry points with their prototypes and declarations, every argument error of taco_spec_warp_map / taco_spec_warp -- all
returned before the first device call, so they are reached here -- semitones_to_scale by hand, and the TACO_ERR_ARG cases of
Synthesizer.synthesize_audio's new keywords on a Synthesizer without a model."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import warp_reference as R
from taco_amd import _lib, prosody

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = 1 << 16


# ---- the restatement on hand-worked cases ----
def test_stretch_one_is_the_identity_map():
    T, frames = 12, [12, 7, 1, 0, 99]                                        # the last two are clamped to 1 and T
    for rs in (None, 1.0):
        m = R.warp_map(frames, T, 1, T + 3, row_stretch=rs)
        assert m["out_frames"].tolist() == [12, 7, 1, 1, 12] and m["f"].tolist() == [12, 7, 1, 1, 12]
        for b, f in enumerate(m["f"]):
            assert m["src"][b, :f].tolist() == list(range(f)) and not m["frac"][b].any()
            assert (m["src"][b, f:] == f - 1).all()                           # past the end: the last frame, frac 0
            assert m["C"][b].tolist() == [(t + 1) * ONE for t in range(f)]


def test_uniform_two_doubles_every_frame():
    T, f = 9, 7
    m = R.warp_map([f], T, 3, 2 * T, row_stretch=2.0)
    assert m["out_frames"][0] == 2 * f
    j = np.arange(2 * f)
    assert np.array_equal(m["src"][0, :2 * f], j // 2) and np.array_equal(m["frac"][0, :2 * f], (j % 2) * 32768)
    assert set(m["frac"][0].tolist()) == {0, 32768}


def test_uniform_half_takes_every_second_frame():
    for f in (8, 9):
        m = R.warp_map([f], 10, 1, 10, row_stretch=0.5)
        of = (f + 1) // 2                                                     # (f * 2^15 + 2^15) >> 16
        assert m["out_frames"][0] == of
        assert m["src"][0, :of].tolist() == [2 * j for j in range(of)] and not m["frac"][0].any()


def test_a_two_token_row_with_stretches_one_and_two_by_hand():
    """r = 2, three steps, T = 6, f = 5.  Step 0 attends to token 0, steps 1 and 2 to token 1 (step 2 by a tie the first index does NOT win:
    token 1 holds the larger value).  Frames 0, 1 last 1; frames 2, 3, 4 last 2.  C = (1, 2, 4, 6, 8) * 2^16, out_frames = 8.
    j:    0  1  2  3      4  5      6  7      8  9
    src:  0  1  2  2      3  3      4  4      4  4   (past the end: f - 1)
    frac: 0  0  0  2^15   0  2^15   0  2^15   0  0"""
    al = np.array([[[0.9, 0.1, 0.2], [0.1, 0.9, 0.8]]], np.float32)          # [1, T_in = 2, n_steps = 3]
    m = R.warp_map([5], 6, 2, 10, alignments=al, token_stretch=np.array([[1.0, 2.0]], np.float32))
    assert m["C"][0].tolist() == [ONE, 2 * ONE, 4 * ONE, 6 * ONE, 8 * ONE] and m["out_frames"][0] == 8
    assert m["src"][0].tolist() == [0, 1, 2, 2, 3, 3, 4, 4, 4, 4]
    assert m["frac"][0].tolist() == [0, 0, 0, 32768, 0, 32768, 0, 32768, 0, 0]
    assert m["token_frames"][0].tolist() == [2, 3]
    # the row stretch multiplies in: 0.5 * (1, 2) = (0.5, 1): C = (0.5, 1, 2, 3, 4) * 2^16, four output frames 0, 2 (tau = 1: C_1 = 1 is not > 1), 3, 4
    h = R.warp_map([5], 6, 2, 10, alignments=al, row_stretch=0.5, token_stretch=np.array([[1.0, 2.0]], np.float32))
    assert h["out_frames"][0] == 4 and h["src"][0, :4].tolist() == [0, 2, 3, 4] and not h["frac"][0].any()
    # a tie: the first maximum wins; a NaN is the maximum and the first NaN wins
    tie = np.array([[[0.5, np.nan, 0.3], [0.5, np.nan, 0.3], [0.1, 0.7, np.nan]]], np.float32)
    assert R.tokens_of(tie).tolist() == [[0, 0, 2]]


def test_the_clamps_and_the_values_that_are_not_numbers():
    d = R.durations(np.array([1.0, 1 / 16, 16.0, 0.01, 0.0624, 100.0, 17.0, np.inf, 0.0, -1.0, -np.inf, np.nan, 1e-45, 3e38], np.float32))
    assert d.tolist() == [ONE, 1 << 12, 1 << 20, 1 << 12, 1 << 12, 1 << 20, 1 << 20, 1 << 20, 1 << 12, 1 << 12, 1 << 12, 1 << 12, 1 << 12, 1 << 20]
    assert R.durations(np.float32(1.5))[()] == 98304 and R.durations(np.float32(0.1))[()] == 6554          # lrint(6553.6000001)
    assert R.durations(np.float32(2.5 / 65536 * 4096))[()] == 10240                                            # exact products stay exact
    assert R.durations(np.float32(0.5 + 0.5 / 65536))[()] == 32768 and R.durations(np.float32(0.5 + 1.5 / 65536))[()] == 32770      # halves go to even
    # a row of NaN stretch runs at the floor: 1/16 of a frame each
    m = R.warp_map([32], 32, 1, 40, row_stretch=float("nan"))
    assert m["out_frames"][0] == 2 and m["src"][0, :2].tolist() == [0, 16] and not m["frac"][0].any()
    # T_out smaller than needed cuts the row; larger leaves src = f - 1 behind
    m = R.warp_map([32], 32, 1, 5, row_stretch=16.0)
    assert m["out_frames"][0] == 5 and m["src"][0].tolist() == [0] * 5 and m["frac"][0].tolist() == [j * 4096 for j in range(5)]


def _random_rows(seed, B=6, T_in=9, n_steps=40, r=3):
    rs = np.random.RandomState(seed)
    al = rs.rand(B, T_in, n_steps).astype(np.float32)
    frames = rs.randint(1, n_steps * r + 1, size=B)
    row = np.exp(rs.uniform(np.log(0.05), np.log(20), size=B)).astype(np.float32)
    tok = np.exp(rs.uniform(np.log(0.05), np.log(20), size=(B, T_in))).astype(np.float32)
    return al, frames, row, tok, n_steps * r, r


def test_tau_stays_below_the_last_prefix_sum_and_the_map_never_steps_back():
    """tau < C_{f-1} for every j < out_frames: j <= out_frames - 1 <= ((C_{f-1} + 2^15) >> 16) - 1, so j << 16 <= C_{f-1} - 2^15.  And the
    position src * 2^16 + frac never decreases with j."""
    rows = 0
    for seed in range(40):
        al, frames, row, tok, T, r = _random_rows(seed)
        for T_out in (T * 20 * 16 // 16 + 2, 7):
            m = R.warp_map(frames, T, r, T_out, alignments=al, row_stretch=row, token_stretch=tok)
            for b in range(len(frames)):
                of, Cl = int(m["out_frames"][b]), int(m["C"][b][-1])
                assert 1 <= of <= T_out and ((of - 1) << 16) < Cl
                if of < T_out:
                    assert of == max(1, (Cl + 32768) >> 16)
                pos = m["src"][b, :of].astype(np.int64) * ONE + m["frac"][b, :of]
                assert (np.diff(pos) >= 0).all() and (m["frac"][b] >= 0).all() and (m["frac"][b] < ONE).all()
                assert (m["src"][b] >= 0).all() and (m["src"][b] < m["f"][b]).all()
                assert m["token_frames"][b].sum() == m["f"][b]
                rows += 1
    assert rows == 480


def test_the_warp_restatements_on_a_row_by_hand():
    """x = frames (0, 10), (4, 20), (8, 40) of W = 2; stretch 2 gives the frames and their midpoints, the last one repeated (t1 = f - 1)."""
    x = np.array([[[0, 10], [4, 20], [8, 40], [np.nan, np.nan]]], np.float32)
    m = R.warp_map([3], 4, 1, 8, row_stretch=2.0)
    for warp in (R.warp64, R.warp32):
        o = warp(x, [3], m)
        assert o[0].tolist() == [[0, 10], [2, 15], [4, 20], [6, 30], [8, 40], [8, 40], [0, 0], [0, 0]]
        # scale 0.5: out[k] = v(k / 2): bin 1 is the midpoint of bins 0 and 1; scale 2: bin 1 reads bin 2, past the axis: +0
        assert warp(x, [3], m, 0.5)[0, :3].tolist() == [[0, 5], [2, 8.5], [4, 12]]
        assert warp(x, [3], m, 2.0)[0, :3].tolist() == [[0, 0], [2, 0], [4, 0]]
        assert warp(x, [3], m, 1.0).tolist() == o.tolist()
        assert not warp(x, [3], m, -1.0)[0, :, 1].any() and not warp(x, [3], m, float("nan")).any()


# ---- the C ABI ----
def _info():
    out = (C.c_int * 4)()
    assert _lib.load_library().taco_debug_warp_info(out, 4) == 0
    return list(out)


def test_symbols_prototypes_and_declarations():
    lib = _lib.load_library()
    pub = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    dbg = open(os.path.join(ROOT, "include", "taco_debug.h")).read()
    for name, nargs, text in (("taco_spec_warp_workspace_bytes", 2, pub), ("taco_spec_warp_map", 17, pub), ("taco_spec_warp", 12, pub),
                              ("taco_debug_warp_info", 2, dbg), ("taco_debug_spec_warp_direct", 12, dbg)):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", text, flags=re.S))
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert "taco_debug_warp" not in pub
    assert pub.index("taco_manual_alignments(void*") < pub.index("taco_spec_warp_workspace_bytes(int") < pub.index("taco_stop_steps(void*")
    doc = pub[pub.index("rate, per-token duration and pitch control"):pub.index("size_t taco_spec_warp_workspace_bytes")]
    for phrase in ("NOT in the reference", "clamp(lrint(fp32(row_stretch[b] * token_stretch[b, tok(t / r)]) * 65536), 2^12, 2^20)",
                   "clamp((C_{f-1} + 2^15) >> 16, 1, T_out)", "THE TIME INTERPOLATION FIRST, THEN THE FREQUENCY INTERPOLATION", "NOT reproduced"):
        assert phrase in doc, phrase
    chunk, wave, rows, stage = _info()
    assert wave == 64 and chunk % wave == 0 and chunk > wave and rows >= 1 and 4 * (stage + 1) * 4 <= 64 * 1024      # dynamic LDS that needs no attribute
    assert lib.taco_debug_warp_info(None, 3) == _lib.TACO_ERR_ARG and lib.taco_debug_warp_info((C.c_int * 3)(), -1) == _lib.TACO_ERR_ARG
    assert lib.taco_spec_warp_workspace_bytes(3, 100) >= 3 * 100 * 8 and lib.taco_spec_warp_workspace_bytes(0, 5) == 0
    import taco_amd
    assert taco_amd.prosody is prosody and taco_amd.warp_map is prosody.warp_map
    p = inspect.signature(prosody.warp_map).parameters
    assert list(p)[:8] == ["frames", "T", "reduction_factor", "alignments", "row_stretch", "token_stretch", "out_cap", "return_token_frames"]
    assert list(inspect.signature(prosody.warp).parameters) == ["spec", "frames", "map", "freq_scale"]
    assert list(inspect.signature(prosody.token_frames).parameters) == ["alignments", "frames", "reduction_factor"]
    p = inspect.signature(taco_amd.Synthesizer.synthesize_audio).parameters
    assert [p[k].default for k in ("rate", "token_stretch", "pitch", "return_durations")] == [None, None, None, False]
    assert "rate" not in inspect.signature(taco_amd.Synthesizer.synthesize).parameters


def test_every_argument_error_is_returned_without_a_device():
    """The pointers are host arrays: a call that passed the checks would hand them to a kernel, so every call here must fail first."""
    lib = _lib.load_library()
    ARG, STATE, UNSUP = _lib.TACO_ERR_ARG, _lib.TACO_ERR_STATE, _lib.TACO_ERR_UNSUPPORTED
    B, T_in, n, r, T_out, W = 2, 5, 6, 3, 40, 7
    T = n * r
    al, frames = np.zeros((B, T_in, n), np.float32), np.zeros(B, np.int32)
    rs, ts = np.ones(B, np.float32), np.ones((B, T_in), np.float32)
    src, frac, of, tf = np.zeros((B, T_out), np.int32), np.zeros((B, T_out), np.int32), np.zeros(B, np.int32), np.zeros((B, T_in), np.int32)
    need = lib.taco_spec_warp_workspace_bytes(B, T)
    ws = np.zeros(need // 8 + 2, np.int64)
    P = lambda x, off=0: None if x is None else C.c_void_p(x.ctypes.data + off)

    def mcall(**kw):
        v = dict(al=P(al), frames=P(frames), rs=P(rs), ts=P(ts), B=B, T_in=T_in, n=n, r=r, T=T, T_out=T_out, src=P(src), frac=P(frac), of=P(of),
                 tf=P(tf), ws=P(ws), nws=need)
        v.update(kw)
        return lib.taco_spec_warp_map(None, v["al"], v["frames"], v["rs"], v["ts"], v["B"], v["T_in"], v["n"], v["r"], v["T"], v["T_out"], v["src"],
                                      v["frac"], v["of"], v["tf"], v["ws"], v["nws"])

    for kw in (dict(src=None), dict(frac=None), dict(of=None), dict(ws=None)):                                    # null required pointer
        assert mcall(**kw) == ARG and b"null" in lib.taco_last_error(), kw
    for kw in (dict(B=0), dict(B=-1), dict(T=0), dict(T_out=0), dict(T_out=-4), dict(r=0), dict(T_in=0), dict(n=0), dict(n=-1)):
        assert mcall(**kw) == ARG and b">= 1" in lib.taco_last_error(), kw
    for kw in (dict(T=T + 1), dict(T=T - 1), dict(r=r + 1), dict(n=n + 1), dict(T=2 ** 31 - 1, n=2 ** 31 - 1, r=2 ** 31 - 1)):
        assert mcall(**kw) == ARG and b"n_steps * reduction_factor" in lib.taco_last_error(), kw
    for kw in (dict(al=None), dict(al=None, tf=None), dict(al=None, ts=None)):                                     # stretch / durations per token need tokens
        assert mcall(**kw) == ARG and b"needs d_alignments" in lib.taco_last_error(), kw
    assert mcall(ws=P(ws, 4)) == ARG and b"aligned" in lib.taco_last_error()
    for kw in (dict(nws=need - 1), dict(nws=0)):
        assert mcall(**kw) == STATE and b"taco_spec_warp_workspace_bytes" in lib.taco_last_error(), kw
    assert mcall(src=None, nws=0) == ARG                                                                          # argument errors come first
    overlaps = (dict(src=P(frac)), dict(src=P(frac, frac.nbytes - 4)), dict(frac=P(of)), dict(of=P(src, 8)), dict(tf=P(src)), dict(tf=P(of, 4)),
                dict(ws=P(src.view(np.int64), 8)), dict(src=P(ws, 8)), dict(of=P(ws, need - 8)),                    # output on output or workspace
                dict(src=P(al)), dict(frac=P(al, al.nbytes - 4)), dict(of=P(frames, 4)), dict(tf=P(rs)), dict(src=P(ts, ts.nbytes - 4)),
                dict(of=P(rs, 4)), dict(ws=P(al.view(np.int64))), dict(frac=P(frames)), dict(tf=P(ts)))             # output on input
    for kw in overlaps:
        assert mcall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw
    assert mcall(al=None, ts=None, tf=None, src=P(frac)) == ARG and b"overlap" in lib.taco_last_error()           # also without alignments
    assert mcall(al=None, ts=None, tf=None, T_in=0, n=0, src=None) == ARG                                         # (T_in, n_steps are not read then)

    spec, out, fs = np.zeros((B, T, W), np.float32), np.zeros((B, T_out, W), np.float32), np.ones(B, np.float32)

    for fn in (lib.taco_spec_warp, lib.taco_debug_spec_warp_direct):
        _warp_errors(lib, fn, P, spec, frames, src, frac, of, fs, out, B, T, W, T_out)


def _warp_errors(lib, fn, P, spec, frames, src, frac, of, fs, out, B, T, W, T_out):
    ARG, UNSUP = _lib.TACO_ERR_ARG, _lib.TACO_ERR_UNSUPPORTED

    def wcall(**kw):
        v = dict(spec=P(spec), frames=P(frames), src=P(src), frac=P(frac), of=P(of), fs=P(fs), B=B, T=T, W=W, T_out=T_out, out=P(out))
        v.update(kw)
        return fn(None, v["spec"], v["frames"], v["src"], v["frac"], v["of"], v["fs"], v["B"], v["T"], v["W"], v["T_out"], v["out"])

    for kw in (dict(spec=None), dict(src=None), dict(frac=None), dict(of=None), dict(out=None)):
        assert wcall(**kw) == ARG and b"null" in lib.taco_last_error(), kw
    for kw in (dict(B=0), dict(T=0), dict(W=0), dict(T_out=0), dict(W=-3), dict(B=-2)):
        assert wcall(**kw) == ARG and b">= 1" in lib.taco_last_error(), kw
    for kw in (dict(out=P(spec)), dict(out=P(spec, spec.nbytes - 4)), dict(out=P(frames, 4)), dict(out=P(src)), dict(out=P(frac, frac.nbytes - 4)),
               dict(out=P(of)), dict(out=P(fs, 4)), dict(spec=P(out, out.nbytes - 4)), dict(fs=P(out, 12)),
               dict(B=2 ** 31 - 1, T=2 ** 31 - 1, T_out=2 ** 31 - 1, W=2 ** 24 - 1)):                                # byte counts that do not fit 64 bits
        assert wcall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw
    assert wcall(W=1 << 24) == UNSUP and b"2^24" in lib.taco_last_error()
    assert wcall(W=1 << 24, out=None) == ARG


# ---- Python ----
def test_semitones_to_scale_by_hand():
    s = prosody.semitones_to_scale
    assert s(0) == 1 and s(12) == 0.5 and s(-12) == 2 and s(24) == 0.25 and s(6) == np.float32(0.5 ** 0.5)
    assert s(1).dtype == np.float32 and s(1) == np.float32(0.9438743126816935) and s(-1) == np.float32(1.0594630943592953)
    assert s([0, 12, -12]).tolist() == [1.0, 0.5, 2.0] and s([0, 12]).dtype == np.float32


def test_the_bound_on_out_frames_is_exact_for_host_side_stretches():
    assert prosody.out_frames_bound(100) == 100 and prosody.out_frames_bound(100, [1.0, 1.0]) == 100           # stretch 1: the capacity stays T
    assert prosody.out_frames_bound(100, 2.0) == 200 and prosody.out_frames_bound(101, 0.5) == 51
    assert prosody.out_frames_bound(10, 1e9) == 160 and prosody.out_frames_bound(64, float("nan")) == 64 and prosody.out_frames_bound(64, -1.0) == 4
    for seed in range(10):
        al, frames, row, tok, T, r = _random_rows(seed)
        cap = prosody.out_frames_bound(T, row, tok)
        m = R.warp_map(frames, T, r, cap + 5, alignments=al, row_stretch=row, token_stretch=tok)
        assert (m["out_frames"] <= cap).all()


def test_the_new_keywords_are_refused_before_the_model_is_touched():
    """Every refusal comes before the forward, so a Synthesizer without a model shows them."""
    import taco_amd
    s = taco_amd.Synthesizer()
    ids = np.array([[5, 6, 7, 1], [8, 9, 1, 0]])
    bad = [dict(pitch=2.0, vocoder="mel"), dict(pitch=[1.0, 2.0], vocoder="mel", rate=1.0),
           dict(rate=0.0), dict(rate=-1.0), dict(rate=float("nan")), dict(rate=float("inf")), dict(rate=[1.0, 2.0, 3.0]), dict(rate=[1.0, 0.0]),
           dict(rate=[[1.0, 1.0]]), dict(rate="fast"),
           dict(pitch=float("nan")), dict(pitch=[1.0]), dict(pitch=float("inf")),
           dict(token_stretch=[[1.0], [1.0], [1.0]]), dict(token_stretch=[[1.0] * 5]), dict(token_stretch=[[1.0, -2.0]]),
           dict(token_stretch=[[1.0, 0.0]]), dict(token_stretch=[[float("nan")]]), dict(token_stretch=[1.0, 2.0]),      # a flat row for a batch of two
           dict(token_stretch=[[[1.0]]])]
    for kw in bad:
        with pytest.raises(_lib.TacoError) as e:
            s.synthesize_audio(tokens=ids, **kw)
        assert e.value.code == _lib.TACO_ERR_ARG, kw
    for kw in (dict(rate=1.0), dict(rate=[1.0, 2.0], pitch=-3, token_stretch=[[2.0, 1.0]]), dict(token_stretch=[[1.0] * 4, []], vocoder="mel"),
               dict(return_durations=True)):
        with pytest.raises(AttributeError):                                     # past the checks: the first use of the model that is not there
            s.synthesize_audio(tokens=ids, **kw)
    row, tok, scale = s._prosody_args(2, 4, [2.0, 0.5], [[3.0, 0.5]], 12, "griffin_lim")
    assert row.dtype == np.float32 and row.tolist() == [0.5, 2.0] and scale.tolist() == [0.5, 0.5]
    assert tok.dtype == np.float32 and tok.tolist() == [[3.0, 0.5, 1.0, 1.0], [1.0] * 4]
    assert s._prosody_args(1, 3, None, [2.0, 3.0], None, "mel")[1].tolist() == [[2.0, 3.0, 1.0]] and s._prosody_args(2, 4, None, None, None, "mel") is None
