"""Host side of the Griffin-Lim stage tests: the restatement tests/gl_reference.py against oracle/audio_oracle.py, the mutation table --
every named mistake of gl_reference.MUTATIONS misses the equality or the bound of its stage on the inputs tests/test_gpu_gl_stages.py
gives the device, by the factor each case prints -- the symbols and the argument errors of the taco_debug_gl_* hooks, which all come
before their first device call, and the preconditions of the GPU tests.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import audio_oracle as A
import gl_reference as G
from taco_amd import _lib, audio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOOKS = ("taco_debug_gl_info", "taco_debug_gl_prologue", "taco_debug_gl_overlap_add", "taco_debug_gl_inv_preemphasis", "taco_debug_gl_dft")
A97 = float(np.float32(0.97))                     # the coefficient the device holds


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _host_handle(lib, hp, tf=False):
    h = C.c_void_p()
    chp = audio.c_audio_hparams(hp)
    assert lib.taco_debug_gl_create_host(C.byref(chp), int(tf), C.byref(h)) == 0
    return h


# ---- the restatement ----
@pytest.mark.parametrize("name,T", [("small", 13), ("hop30", 14), ("win_is_nfft", 9), ("hop_is_win", 5), ("reference", 6)])
def test_the_stages_compose_to_the_oracle_at_zero_iterations(name, T):
    """Float64 rounding: the matrix product sums 2F terms where irfft does a transform, so the two differ by a few K * 2^-53 of the
    frame's absolute sum; 1e-11 of the peak covers K = 2050 a hundred times over and is nine orders below any mistake."""
    hp = G.HANDLES[name]
    rs = np.random.RandomState(T)
    spec, u = rs.rand(hp.num_freq, T) * 1.2 - 0.1, rs.rand(hp.num_freq, T)
    ref = A.inv_spectrogram(spec, hp, u, iters=0)
    got = G.inv_spectrogram64(spec, hp, u)
    e = float(np.abs(got - ref).max() / np.abs(ref).max())
    print("%s, T %d: composed stages vs audio_oracle.inv_spectrogram, error over peak %.3g" % (name, T, e))
    assert got.shape == ref.shape == (G.Geometry(hp).hop * (T - 1),) and e < 1e-11, e


def test_the_float32_forms_are_the_float64_forms_rounded():
    """On integer frames the float32 overlap-add differs from float64 by the two roundings of the window sum's reciprocal and the product
    alone: 3 * 2^-24 relative (the sum of squares itself adds ceil(win/hop) - 1 more)."""
    for name, T in G.OVERLAP_ADD_CASES:
        geo, frames, Y = G.overlap_add_case(name, T)
        for b, f in enumerate(frames):
            fb = geo.frames(f, T)
            row, _ = G.overlap_add32(Y[b], geo, T, f)
            y64, _ = G.overlap_add64(Y[b], geo, fb)
            y32 = row[geo.half:geo.half + geo.hop * (fb - 1)]
            n = -(-geo.win // geo.hop)
            assert np.all(np.abs(y32 - y64) <= (n + 2) * G.U * np.abs(y64) + 1e-300), (name, T, b)
            assert np.array_equal(row[:geo.hop * (fb - 1) + geo.n_fft], np.pad(y32, geo.half, mode="reflect")) and not row[geo.hop * (fb - 1) + geo.n_fft:].any()
    x = np.random.RandomState(0).randn(3000)
    assert np.array_equal(G.inv_preemphasis64(x, A97), A.inv_preemphasis(x, type("H", (), {"preemphasis": A97})))
    got = G.chunked_scan(x, A97, 3000, 3000, np.float64)
    assert np.abs(got - G.inv_preemphasis64(x, A97)).max() < 1e-12 * np.abs(got).max()


def test_the_dft_matrices_are_the_transform_pair():
    for name in ("small", "win_is_nfft", "hop30"):
        geo = G.Geometry(G.HANDLES[name])
        fwd, inv = G.dft_matrices(geo)
        w = np.zeros(geo.n_fft); w[geo.lpad:geo.lpad + geo.win] = G.window64(geo.win)
        x = np.random.RandomState(1).randn(geo.win)
        frame = np.zeros(geo.n_fft); frame[geo.lpad:geo.lpad + geo.win] = x
        X = np.fft.rfft(frame * w)
        assert np.allclose(x @ fwd, np.concatenate([X.real, X.imag]), atol=1e-12)
        Z = np.random.RandomState(2).randn(2 * geo.F)
        back = (np.fft.irfft(Z[:geo.F] + 1j * Z[geo.F:], geo.n_fft) * w)[geo.lpad:geo.lpad + geo.win]
        assert np.allclose(Z @ inv, back, atol=1e-12)
        assert not inv[geo.F].any() and not inv[2 * geo.F - 1].any()             # no imaginary part on DC and Nyquist


# ---- the mutation table ----
def test_every_mutation_has_a_stage():
    listed = [m for ms in G.STAGE_MUTATIONS.values() for m in ms]
    assert sorted(listed) == sorted(G.MUTATIONS) and len(set(listed)) == len(listed)


@pytest.mark.parametrize("name,T", G.OVERLAP_ADD_CASES)
def test_overlap_add_mutations_break_the_equality(name, T):
    """The bit equality of the integer tier, on its inputs: per mutation the samples of the padded rows that change.  A mutation must
    change some row of every case it can reach: the tiny branch exists on the hop == win handle only, and there the window sum has a
    single covering frame at every position, so `wss_missing_last_frame` is seen as the whole table."""
    geo, frames, Y = G.overlap_add_case(name, T)
    good = [G.overlap_add32(Y[b], geo, T, f)[0] for b, f in enumerate(frames)]
    tiny_rows = sum(int(G.overlap_add32(Y[b], geo, T, f)[1].sum()) for b, f in enumerate(frames))
    for m in G.STAGE_MUTATIONS["overlap_add"]:
        bad = [G.overlap_add32(Y[b], geo, T, f, mutation=m)[0] for b, f in enumerate(frames)]
        changed = sum(int((_bits(a) != _bits(c)).sum()) for a, c in zip(good, bad))
        print("%s, T %d, %s: %d of %d samples of the padded rows change" % (name, T, m, changed, sum(a.size for a in good)))
        if m == "tiny_returns_0":
            # the sample is acc * 1 against acc * 0: it changes wherever the frame's first sample is not itself 0
            assert (changed > 0) == (tiny_rows > 0) == (name == "hop_is_win"), (name, m, changed, tiny_rows)
        elif m == "short_row_full_table":
            # frames that do not overlap: inside a short row's own samples the table of T frames holds the row's own sums
            assert (changed > 0) == (name != "hop_is_win"), (name, T, m, changed)
        else:
            assert changed > 0, (name, T, m)


def test_the_tiny_branch_is_taken_at_every_frame_start_of_the_hop_is_win_handle():
    geo, frames, Y = G.overlap_add_case("hop_is_win", 5)
    for b, f in enumerate(frames):
        fb = geo.frames(f, 5)
        _, small = G.overlap_add32(Y[b], geo, 5, f)
        s = np.arange(geo.hop * (fb - 1))
        assert np.array_equal(small, (s + geo.half - geo.lpad) % geo.hop == 0) and small.sum() == fb - 1, b


@pytest.mark.parametrize("name", ["small", "hop30"])
def test_overlap_add_mutations_miss_the_random_tier(name):
    """The derived bound of the random tier (gl_reference.overlap_add64), on its inputs: the largest error over bound per mutation"""
    T = 14
    geo, frames, Y = G.overlap_add_case(name, T, integers=False)
    for m in ("reflect_one_off", "wss_missing_last_frame", "short_row_full_table"):
        worst = 0.0
        for b, f in enumerate(frames):
            fb = geo.frames(f, T)
            L = geo.hop * (fb - 1)
            y, bound = G.overlap_add64(Y[b], geo, fb)
            bad = G.overlap_add32(Y[b], geo, T, f, mutation=m)[0][:L + geo.n_fft].astype(np.float64)
            ref, bnd = np.pad(y, geo.half, mode="reflect"), np.pad(bound, geo.half, mode="reflect")
            worst = max(worst, float((np.abs(bad - ref) / bnd).max()))
        print("%s, random frames, %s: misses the bound by a factor %.3g" % (name, m, worst))
        assert worst > 100, (name, m, worst)


@pytest.mark.parametrize("L", G.PREEMPHASIS_LENGTHS)
def test_preemphasis_mutations(L):
    """Integer tier (a = 1, equality): a carry taken from the wrong chunk changes an integer at every length with more than one sample; the
    two other mutations are invisible at a = 1 (a^C = a^(C-1) = 1, f = 1) and are the random tier's to see.  Random tier (a = 0.97, the
    derived bound of gl_reference.preemphasis_bound_units): all three miss it at every length with more than two samples.  A single
    sample has no carry to get wrong: nothing changes there.  With two samples the wrong chunk's carry and the factor started at 1 miss the
    bound as well; the power does not show, because the only carry in use is ends[0] + a^C * 0."""
    fmin, frames, x = G.preemphasis_case(L, integers=True)
    T = L + 1
    lens = [min(max(int(f), fmin), T) - 1 for f in frames]
    good = [G.chunked_scan(x[b], 1.0, L, n) for b, n in enumerate(lens)]
    for b, n in enumerate(lens):
        assert np.array_equal(good[b][:n], np.cumsum(x[b, :n].astype(np.float64)).astype(np.float32)) and not good[b][n:].any()
        assert np.abs(good[b]).max() < 2 ** 24
    bad = [G.chunked_scan(x[b], 1.0, L, n, mutation="carry_from_wrong_chunk") for b, n in enumerate(lens)]
    changed = sum(int((a != c).sum()) for a, c in zip(good, bad))
    print("L %d, a = 1, carry_from_wrong_chunk: %d integers change" % (L, changed))
    assert (changed > 0) == (L > 1), (L, changed)
    for m in ("power_c_minus_1", "factor_starts_at_1"):
        assert all(np.array_equal(a, G.chunked_scan(x[b], 1.0, L, n, mutation=m)) for b, (a, n) in enumerate(zip(good, lens)))
    fmin, frames, x = G.preemphasis_case(L, integers=False)
    units = G.preemphasis_bound_units(A97, L)
    for m in G.STAGE_MUTATIONS["preemphasis"]:
        worst = 0.0
        for b, n in enumerate(lens):
            if n == 0:
                continue
            ref = G.inv_preemphasis64(x[b, :n], A97)
            got = G.chunked_scan(x[b], A97, L, n, np.float64, mutation=m)[:n]
            worst = max(worst, float(np.abs(got - ref).max() / (units * G.U * np.abs(ref).max())))
        print("L %d, a = 0.97, %s: misses the bound of %.0f units by a factor %.3g" % (L, m, units, worst))
        if L > 2 or (L == 2 and m != "power_c_minus_1"):
            assert worst > 3, (L, m, worst)
        elif L == 2:
            assert worst < 1, (L, m, worst)           # two samples in two chunks: the second chunk's carry is ends[0] + a^C * 0 whatever the power
        else:
            assert worst == 0, (L, m, worst)
    # and the float32 restatement itself is inside the bound
    for b, n in enumerate(lens):
        if n:
            ref = G.inv_preemphasis64(x[b, :n], A97)
            e = float(np.abs(G.chunked_scan(x[b], A97, L, n)[:n] - ref).max() / (units * G.U * np.abs(ref).max()))
            assert e <= 1.0, (L, b, e)


@pytest.mark.parametrize("name", ["small", "reference"])
def test_inverse_matrix_mutation_misses_the_unit_rows(name):
    """A unit row at DC or Nyquist reads that row of the inverse matrix alone: its bound is one product's, and a weight of 2 there doubles the
    frame.  On the random rows the mutation moves an element by about 1 / (2F) of its absolute sum, which the worst-case bounds of a
    2F-term sum do not separate; the unit rows do."""
    geo, X, zero, units = G.dft_inverse_case(name)
    inv = G.dft_matrices(geo)[1]
    bad = G.dft_matrices(geo, "hermitian_2_at_dc_nyquist")[1]
    for row, k in units.items():
        x = X[row].astype(np.float64)
        bound = (3.03 * 2.0 ** -18 + 3 * 2 * geo.F * G.U) * (np.abs(x) @ np.abs(inv))           # the split-bf16 bound, the wider of the two
        d = np.abs(x @ bad - x @ inv)
        edge = k in (0, geo.F - 1)
        if edge:
            f = float((d[bound > 0] / bound[bound > 0]).min())
            print("%s, unit row at column %d: the mutation misses the bound by a factor of at least %.3g" % (name, k, f))
            assert f > 1000, (name, k, f)
        else:
            assert not d.any()


# ---- preconditions of the GPU tests ----
def test_preconditions():
    for name in ("small", "reference"):
        geo, B, T, frames, spec, u = G.prologue_case(name)
        inside = float(((spec > 0) & (spec < 1)).mean())
        assert inside >= 0.8, (name, inside)                                   # most inputs exercise the power law, not the clip
        assert (spec <= 0).any() and (spec >= 1).any() and (u >= 0).all() and (u < 1).all()
        assert frames.min() < geo.fmin and frames.max() == T
    hops = set()
    for name, T in G.OVERLAP_ADD_CASES:
        geo, frames, Y = G.overlap_add_case(name, T)
        assert geo.hop * (T - 1) > geo.half and np.array_equal(Y, np.round(Y)) and np.abs(Y).max() <= 8
        assert frames.min() < geo.fmin and frames.max() > T and geo.fmin + 1 < T
        hops.add((geo.n_fft, geo.win, geo.hop, geo.lpad))
    assert hops == {(128, 80, 20, 24), (80, 80, 20, 0), (128, 80, 30, 24), (128, 80, 80, 24), (2048, 1200, 300, 424)}
    assert [20 * (T - 1) for n, T in G.OVERLAP_ADD_CASES if n == "small"] == [240, 260, 500, 520]                # around one and two 256-thread blocks
    for L in G.PREEMPHASIS_LENGTHS:
        fmin, frames, x = G.preemphasis_case(L, True)
        C = -(-L // 1024)
        if L > 2:
            assert (frames[1] - 1) % C != 0 or C == 1
        if 2 < L < 100000:
            assert (frames[2] - 1) % C == 0 and 0 < frames[2] - 1 < L and frames[3] < fmin
    assert -(-153300 // 1024) == 150 and -(-3073 // 1024) == 4 and -(-1025 // 1024) == 2


# ---- the C ABI ----
def test_the_hooks_are_exported_mirrored_and_declared():
    lib = _lib.load_library()
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "taco_debug.h")).read(), flags=re.S)
    for name in HOOKS:
        assert hasattr(lib, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\s*\(" % name, code), "%s is not declared in include/taco_debug.h" % name
    assert _lib.PROTOTYPES["taco_debug_gl_inv_preemphasis"][1][7] is C.c_float


@pytest.mark.parametrize("name", sorted(G.HANDLES))
@pytest.mark.parametrize("tf", [False, True])
def test_the_geometry_the_library_reports_is_the_restatements(name, tf):
    lib = _lib.load_library()
    h = _host_handle(lib, G.HANDLES[name], tf)
    geo = G.Geometry(G.HANDLES[name], tf)
    out = (C.c_int * 8)()
    for T in (1, 2, 13, 27):
        assert lib.taco_debug_gl_info(h, T, out, 8) == 0 and list(out) == geo.info(T), (name, tf, T, list(out), geo.info(T))
    keep = (C.c_int * 8)(*([-7] * 8))
    assert lib.taco_debug_gl_info(h, 13, keep, 3) == 0 and list(keep) == geo.info(13)[:3] + [-7] * 5
    assert lib.taco_debug_gl_info(None, 13, out, 8) == lib.taco_debug_gl_info(h, 13, None, 8) == _lib.TACO_ERR_ARG
    assert lib.taco_debug_gl_info(h, 0, out, 8) == lib.taco_debug_gl_info(h, 13, out, -1) == _lib.TACO_ERR_ARG
    lib.taco_gl_destroy(h)


def test_hook_argument_errors_need_no_device():
    lib = _lib.load_library()
    err = lambda: lib.taco_last_error()
    E = _lib
    lr, tf = _host_handle(lib, G.HANDLES["small"]), _host_handle(lib, G.HANDLES["small"], True)
    buf = (C.c_float * 16)()
    d = C.cast(buf, C.c_void_p)          # never dereferenced: every call below returns before its first device call

    def prologue(g=lr, spec=d, frames=None, u=None, B=3, T=13, S=d, X=d):
        return lib.taco_debug_gl_prologue(g, None, spec, frames, u, 0, B, T, S, X)

    for kw in (dict(g=None), dict(spec=None), dict(S=None), dict(X=None), dict(B=0), dict(B=-2), dict(B=65536), dict(T=1), dict(T=0), dict(g=tf, T=0)):
        assert prologue(**kw) == E.TACO_ERR_ARG, kw
    assert prologue(B=40000, T=30000) == E.TACO_ERR_SHAPE
    for kw in ({}, dict(frames=d, u=d), dict(g=tf, T=1)):
        assert prologue(**kw) == E.TACO_ERR_STATE and b"host-only" in err(), kw

    def ola(g=lr, Y=d, frames=None, B=3, T=13, ypad=d, wss=d):
        return lib.taco_debug_gl_overlap_add(g, None, Y, frames, B, T, ypad, wss)

    for kw in (dict(g=None), dict(Y=None), dict(ypad=None), dict(wss=None), dict(B=0), dict(B=65536), dict(T=1), dict(g=tf, T=0)):
        assert ola(**kw) == E.TACO_ERR_ARG, kw
    assert ola(T=4) == E.TACO_ERR_SHAPE and b"reflect padding" in err()       # 20 * 3 <= 64, as the vocoder answers
    for kw in ({}, dict(T=5), dict(frames=d), dict(g=tf, wss=None), dict(g=tf, T=1, wss=None)):
        assert ola(**kw) == E.TACO_ERR_STATE and b"host-only" in err(), kw

    def pre(x=d, frames=None, fmin=2, T=9, hop=1, B=2, a=0.97, wav=d, ns=None):
        return lib.taco_debug_gl_inv_preemphasis(None, x, frames, fmin, T, hop, B, a, wav, ns)

    for kw in (dict(x=None), dict(wav=None), dict(B=0), dict(B=65536), dict(T=1), dict(hop=0), dict(fmin=0), dict(fmin=10), dict(a=float("nan")),
               dict(a=float("inf")), dict(hop=1 << 20, T=1 << 20)):
        assert pre(**kw) == E.TACO_ERR_ARG, kw

    def dft(g=lr, which=0, exact=0, rows=d, n=1 << 20, M=8, ld=20, out=d):
        return lib.taco_debug_gl_dft(g, None, which, exact, rows, n, M, ld, out)

    for kw in (dict(g=None), dict(rows=None), dict(out=None), dict(M=0), dict(ld=0), dict(which=2), dict(which=-1), dict(exact=2), dict(exact=-1)):
        assert dft(**kw) == E.TACO_ERR_ARG, kw
    assert dft(n=7 * 20 + 79) == E.TACO_ERR_ARG and b"d_rows holds" in err()                    # forward: K = win = 80
    assert dft(which=1, ld=130, n=7 * 130 + 129) == E.TACO_ERR_ARG                                # inverse: K = 2F = 130
    assert dft(M=1 << 24, ld=130, n=1 << 40) == E.TACO_ERR_SHAPE and b"too many elements" in err()  # M * max(N, ld) past an int
    assert dft(which=1, M=1 << 25, ld=130, n=1 << 40) == E.TACO_ERR_SHAPE
    for kw in (dict(n=7 * 20 + 80), dict(which=1, ld=130, n=8 * 130), dict(exact=1)):
        assert dft(**kw) == E.TACO_ERR_STATE and b"host-only" in err(), kw
    lib.taco_gl_destroy(lr); lib.taco_gl_destroy(tf)
