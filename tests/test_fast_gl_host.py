"""Host side of Fast Griffin-Lim: the float64 restatement tests/fast_gl_reference.py against the two restatements it extends and against
the convergence it promises, and the symbols, the argument and state errors and the workspace sizes of the new entry points, all of
which come before their first device call.  No GPU."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import audio_oracle as A
import fast_gl_reference as FG
import vocoder_reference as V
from taco_amd import _lib, audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = A.AudioHParams(num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, griffin_lim_iters=3)        # n_fft 128, hop 20, win 80
CONSISTENT = FG.CONSISTENT
NEW = ("taco_gl_set_momentum", "taco_gl_momentum", "taco_gl_convergence_workspace_bytes", "taco_gl_convergence")


@functools.lru_cache(maxsize=None)
def consistent_sc(seed, momentum, iters):
    spec, target, u = FG.consistent_case(seed)
    return FG.spectral_convergence(FG.inv_spectrogram(spec, CONSISTENT, u, iters=iters, momentum=momentum), target, CONSISTENT)


# ---- the restatement ----
@pytest.mark.parametrize("iters", [0, 1, 4])
def test_momentum_zero_is_the_two_restatements_it_extends(iters):
    rs = np.random.RandomState(iters)
    spec, u = rs.rand(65, 23) * 1.2 - 0.1, rs.rand(65, 23)
    assert np.array_equal(FG.inv_spectrogram(spec, SMALL, u, iters=iters), A.inv_spectrogram(spec, SMALL, u, iters=iters))
    S = FG.magnitudes(spec, SMALL)
    assert np.array_equal(FG.griffin_lim(S, SMALL, u, iters=iters), A.griffin_lim(S, SMALL, u, iters=iters))
    assert np.array_equal(FG.inv_spectrogram_tensorflow(spec.T, SMALL, iters=iters), V.inv_spectrogram_tensorflow(spec.T, SMALL, iters=iters))
    hp = A.AudioHParams(**{k: getattr(SMALL, k) for k in ("num_freq", "sample_rate", "frame_length_ms", "frame_shift_ms")})
    hp.num_mels = 12
    inv, mel = audio.inv_mel_basis(hp), rs.rand(23, 12)
    assert np.array_equal(FG.inv_melspectrogram(mel, inv, SMALL, u.T, iters=iters), V.inv_melspectrogram(mel, inv, SMALL, u.T, iters=iters))


def test_the_first_iteration_has_no_previous_estimate():
    rs = np.random.RandomState(3)
    spec, u = rs.rand(65, 23), rs.rand(65, 23)
    assert np.array_equal(FG.inv_spectrogram(spec, SMALL, u, iters=1, momentum=0.99), FG.inv_spectrogram(spec, SMALL, u, iters=1))
    assert np.array_equal(FG.inv_spectrogram_tensorflow(spec.T, SMALL, iters=1, momentum=0.99), FG.inv_spectrogram_tensorflow(spec.T, SMALL, iters=1))
    assert not np.array_equal(FG.inv_spectrogram(spec, SMALL, u, iters=2, momentum=0.99), FG.inv_spectrogram(spec, SMALL, u, iters=2))


def test_spectral_convergence_of_a_consistent_waveform_is_zero():
    t = np.arange(40 * 59) / 3200.0
    y0 = np.sin(2 * np.pi * 220 * t) + 0.5 * np.sin(2 * np.pi * 555 * t * (1 + 0.2 * t))
    mag = np.abs(A.stft(y0, CONSISTENT))
    assert FG.spectral_convergence(A.inv_preemphasis(y0, CONSISTENT), mag, CONSISTENT) < 1e-12
    assert FG.spectral_convergence(y0, np.zeros_like(mag), CONSISTENT) == 0.0


@pytest.mark.parametrize("seed", [9, 2])
def test_momentum_reaches_the_plain_loops_convergence_in_half_the_iterations(seed):
    """On the inputs of test_gpu_audio.test_full_iterations_reach_the_same_spectral_consistency (seed: the initial phases) momentum 0.99
    at 30 iterations is below the plain loop at 60 by more than 0.03.  Measured with this restatement: seed 9, 0.1327 against 0.1708;
    seed 2, 0.1109 against 0.1422 (at 20 iterations 0.1520 and 0.1262: below the plain loop's 60 as well).  The proposal of the
    feature quoted 0.075 against 0.122 and 0.083 against 0.119 for the same set-up; those figures are not reproduced here -- the
    result depends on the draw of the phases, not only on the seed's number -- the margin it asked for is."""
    p, f = consistent_sc(seed, 0.0, 60), consistent_sc(seed, 0.99, 30)
    print("seed %d: plain loop, 60 iterations %.4f; momentum 0.99, 30 iterations %.4f" % (seed, p, f))
    assert p - f > 0.03, (p, f)


# ---- the C ABI ----
def _host_handle(lib, hp, tf):
    h = C.c_void_p()
    chp = audio.c_audio_hparams(hp)
    assert lib.taco_debug_gl_create_host(C.byref(chp), int(tf), C.byref(h)) == 0
    return h


def test_the_four_symbols_are_exported_mirrored_and_declared():
    lib = _lib.load_library()
    header = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/taco_abi.h" % name
    assert _lib.PROTOTYPES["taco_gl_momentum"][0] is C.c_float and _lib.PROTOTYPES["taco_gl_set_momentum"][1][1] is C.c_float
    assert "READ THE HANDLE" in header                      # the header says that the three workspace sizes depend on the momentum


def test_momentum_argument_errors_and_state():
    lib = _lib.load_library()
    for tf in (False, True):
        h = _host_handle(lib, SMALL, tf)
        assert lib.taco_gl_momentum(h) == 0.0 and lib.taco_gl_momentum(None) == 0.0
        for bad in (-0.1, 1.5, float("nan"), float("inf")):
            assert lib.taco_gl_set_momentum(h, bad) == _lib.TACO_ERR_ARG and b"momentum" in lib.taco_last_error()
            assert lib.taco_gl_momentum(h) == 0.0
        assert lib.taco_gl_set_momentum(None, 0.5) == _lib.TACO_ERR_ARG
        for ok in (0.99, 1.0, 0.0):
            assert lib.taco_gl_set_momentum(h, ok) == 0 and lib.taco_gl_momentum(h) == np.float32(ok)
        lib.taco_gl_destroy(h)


def test_convergence_argument_and_state_errors_need_no_device():
    lib = _lib.load_library()
    err = lambda: lib.taco_last_error()
    tf, lr = _host_handle(lib, SMALL, True), _host_handle(lib, SMALL, False)
    buf = (C.c_float * 16)()
    d = C.cast(buf, C.c_void_p)          # never dereferenced: every call below returns before its first device call
    big = 1 << 30

    def run(g=lr, target=d, kind=0, frames=None, wav=d, B=3, T=37, sc=d, ws=d, nbytes=big):
        return lib.taco_gl_convergence(g, None, target, kind, frames, wav, B, T, sc, ws, nbytes)

    for kw in (dict(g=None), dict(target=None), dict(wav=None), dict(sc=None), dict(ws=None)):
        assert run(**kw) == _lib.TACO_ERR_ARG, kw
    assert run(kind=2) == _lib.TACO_ERR_ARG and b"target kind" in err()
    assert run(kind=-1) == _lib.TACO_ERR_ARG
    for kw in (dict(B=0), dict(B=-1), dict(B=65536), dict(T=1), dict(T=0)):
        assert run(**kw) == _lib.TACO_ERR_ARG, kw
    assert lib.taco_gl_min_frames(lr) == 5
    assert run(T=4) == _lib.TACO_ERR_SHAPE and b"reflect padding" in err()         # shorter than the vocoder itself accepts
    assert run(g=tf) == _lib.TACO_ERR_STATE and b"taco_gl_create_tf" in err()
    need = lib.taco_gl_convergence_workspace_bytes(lr, 3, 37)
    assert need > 0 and need >= lib.taco_spec_workspace_bytes(lr, 3, 20 * 36)
    assert run(nbytes=need - 1) == _lib.TACO_ERR_STATE and b"workspace too small" in err()
    assert run(nbytes=0) == _lib.TACO_ERR_STATE
    assert lib.taco_gl_convergence_workspace_bytes(None, 3, 37) == 0 and lib.taco_gl_convergence_workspace_bytes(lr, 0, 37) == 0
    assert lib.taco_gl_convergence_workspace_bytes(lr, 3, 1) == 0
    assert lib.taco_gl_convergence_workspace_bytes(lr, 6, 37) > need
    lib.taco_gl_destroy(tf); lib.taco_gl_destroy(lr)


@pytest.mark.parametrize("hp,B,T", [(SMALL, 3, 37), (A.AudioHParams(), 32, 512)], ids=["small", "reference"])
def test_workspace_grows_by_one_estimate_buffer_and_only_with_momentum(hp, B, T):
    lib = _lib.load_library()
    n_fft, hop, win = hp.stft_parameters()
    R = B * (T + -(-n_fft // hop))                       # frame rows of the loop (gl_rows)
    extra = -(-(R * 2 * hp.num_freq * 4) // 256) * 256   # one [R, 2F] float buffer, rounded as the carver rounds
    for tf in (False, True):
        h = _host_handle(lib, hp, tf)
        sizes = lambda: (lib.taco_gl_workspace_bytes(h, B, T), lib.taco_gl_rows_workspace_bytes(h, B, T), lib.taco_gl_tf_workspace_bytes(h, B, T))
        base = sizes()
        assert min(base) > 0
        assert lib.taco_gl_set_momentum(h, 0.99) == 0
        assert sizes() == tuple(b + extra for b in base)
        assert lib.taco_gl_set_momentum(h, 0.0) == 0
        assert sizes() == base
        lib.taco_gl_destroy(h)
    # the size at momentum 0 is the sum of the six buffers it always was
    slot = (T + -(-n_fft // hop)) * hop
    r256 = lambda n: -(-(n * 4) // 256) * 256
    h = _host_handle(lib, hp, False)
    assert lib.taco_gl_workspace_bytes(h, B, T) == (r256(R * hp.num_freq) + 2 * r256(R * 2 * hp.num_freq) + r256(R * win) + r256(B * slot + 2 * n_fft + win)
                                                   + r256(hop * (T - 1) + n_fft))
    lib.taco_gl_destroy(h)
