"""The stages of the librosa-flavour Griffin-Lim path alone on the GPU -- k_gl_magnitude, k_gl_init_phase, the two windowed-DFT products,
k_gl_wss, k_gl_overlap_add (and k_gl_overlap_add_tf), the reflect padding, k_inv_preemphasis -- through the taco_debug_gl_* hooks
(include/taco_debug.h), which launch the product path's kernels with its launch shapes, against tests/gl_reference.py.

Two kinds of bar.  Equalities, on uint32 views: wherever the data make every sum exact (small integers) the float32 restatement in the
kernel's order is the kernel's result to the bit.  Bounds against float64 on random data, each derived where it is used from the count and
kind of the roundings; every case prints `error / bound`.  One bar is measured, not derived: S_REL_BAR below.
tests/test_gl_stages_host.py shows, without a GPU, that every mistake named in gl_reference.MUTATIONS misses these bars on these inputs.

Handles (gl_reference.HANDLES, all at 1600 Hz): small (n_fft 128, win 80, hop 20), win == n_fft (80, 80, 20: lpad 0), a hop that does not
divide the window (128, 80, 30), hop == win (128, 80, 80: the window sum is zero at every frame's first sample and librosa's tiny branch
is taken) and the reference's (2048, 1200, 300)."""
import ctypes as C

import numpy as np
import pytest

import gl_reference as G

pytestmark = pytest.mark.gpu

A97 = float(np.float32(0.97))        # the reference's preemphasis as the device holds it
# MEASURED, not derived: the relative error of k_gl_magnitude's two nested powf against float64.  Worst value met on an MI355X over the
# small and the reference parameters 1.26e-6 (small 1.21e-6, reference 1.26e-6; profiles/r28_gl_stages.txt); the bar is 4 x that,
# tests/test_gpu_spec.py's convention.
S_REL_WORST = 1.26e-6
S_REL_BAR = 4 * S_REL_WORST


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def handles():
    import taco_amd
    made = {}

    def get(name, tf=False):
        if (name, tf) not in made:
            made[name, tf] = taco_amd.GriffinLim(G.HANDLES[name], flavor="tensorflow" if tf else "librosa")
        return made[name, tf]

    yield get
    for g in made.values():
        g.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()             # (a copy: the shared inputs are read-only)


def _call(g, name, *args):
    """One hook on the current stream of g's device (g None: a hook without a handle)"""
    import taco_amd
    from taco_amd._device import call
    call(g.device if g is not None else "cuda:0", getattr(taco_amd._lib.load_library(), name), *args)


def _info(g, geo, T):
    out = (C.c_int * 8)()
    assert g._lib.taco_debug_gl_info(g._h, T, out, 8) == 0 and list(out) == geo.info(T)
    return list(out)


def _overlap_add(g, geo, T, Y, frames):
    """-> (padded rows [B, slot], the tail behind them, the window-sum table) as the device left them"""
    import torch
    from taco_amd._device import STREAM
    B = Y.shape[0]
    slot = geo.slot(T)
    ypad = torch.full((B * slot + geo.tail,), 7.0, dtype=torch.float32, device="cuda")
    wss = torch.full((geo.hop * (T - 1) + geo.n_fft,), 7.0, dtype=torch.float32, device="cuda")
    _call(g, "taco_debug_gl_overlap_add", g._h, STREAM, _dev(Y), None if frames is None else _dev(frames), B, T, ypad, None if geo.tf else wss)
    out = ypad.cpu().numpy()
    return out[:B * slot].reshape(B, slot), out[B * slot:], wss.cpu().numpy()


# ---- overlap-add, window sum, reflect padding ----
@pytest.mark.parametrize("name,T", G.OVERLAP_ADD_CASES)
def test_overlap_add_window_sum_and_reflect_padding_to_the_bit(handles, name, T):
    """Integer frames: every sum is exact, the only roundings are the window sum's, its reciprocal and the final product, and the float32
    restatement reproduces all three.  Rows [T, T-1, fmin+1, fmin] and two whose counts are clamped; L next to the 256-thread block."""
    geo, frames, Y = G.overlap_add_case(name, T)
    g = handles(name)
    _info(g, geo, T)
    rows, tail, wss = _overlap_add(g, geo, T, Y, frames)
    table, small = G.wss_inv32(geo, T)
    assert np.array_equal(_bits(wss), _bits(table)), "k_gl_wss"
    taken = 0
    for b, f in enumerate(frames):
        ref, tiny = G.overlap_add32(Y[b], geo, T, f)
        taken += int(tiny.sum())
        Lb = geo.hop * (geo.frames(f, T) - 1)
        bad = int((_bits(rows[b]) != _bits(ref)).sum())
        assert bad == 0, (name, T, b, bad)
        y = rows[b, geo.half:geo.half + Lb]
        k = np.arange(1, geo.half + 1)
        assert np.array_equal(_bits(rows[b, geo.half - k]), _bits(y[k])) and np.array_equal(_bits(rows[b, geo.half + Lb - 1 + k]), _bits(y[Lb - 1 - k]))
        assert not _bits(rows[b, Lb + geo.n_fft:]).any()                     # exact zeros past the row's own padded samples
    assert not _bits(tail).any()
    assert (taken > 0) == (name == "hop_is_win")                             # the tiny branch: taken there (at every frame's first sample), nowhere else
    # frames == T given through d_frames is the NULL path to the bit (the row's own sums against the table)
    full, _, _ = _overlap_add(g, geo, T, Y, None)
    assert np.array_equal(_bits(full[0]), _bits(rows[0])) and np.array_equal(_bits(full[5]), _bits(rows[5]))
    for b in range(len(frames)):
        assert np.array_equal(_bits(full[b]), _bits(G.overlap_add32(Y[b], geo, T, T)[0])), b
    print("%s, T %d (L %d): padded rows, window-sum table and reflections equal the float32 restatement, 0 of %d words differ; tiny branch taken %d times"
          % (name, T, geo.hop * (T - 1), rows.size + wss.size, taken))


def test_tensorflow_overlap_add_is_the_plain_sum(handles):
    """No window sum, no padding: on integer frames the sums are exact and equal float64; zeros past hop*(f-1) + win; frames clamp to [1, T]"""
    T = 14
    geo, frames, Y = G.overlap_add_case("small", T, tf=True)
    g = handles("small", True)
    _info(g, geo, T)
    rows, tail, _ = _overlap_add(g, geo, T, Y, frames)
    for b, f in enumerate(frames):
        ref, _ = G.overlap_add_tf64(Y[b], geo, T, f)
        n = geo.samples(min(max(int(f), 1), T))
        assert np.array_equal(rows[b].astype(np.float64), ref) and not _bits(rows[b, n:]).any() and np.abs(rows[b, :n]).max() > 0, b
    assert not _bits(tail).any()
    full, _, _ = _overlap_add(g, geo, T, Y, None)
    assert np.array_equal(_bits(full[0]), _bits(rows[0]))
    print("tensorflow flavour, T %d: equal to float64 on integer frames, 0 of %d words differ" % (T, rows.size))


@pytest.mark.parametrize("name", ["small", "hop30"])
def test_overlap_add_on_random_frames_within_the_operation_count(handles, name):
    """Against float64 on the same float32 operands.  Bound (gl_reference.overlap_add64): at most ceil(win/hop) - 1 additions in each of
    the two sums, one division, one multiplication: 2 ceil(win/hop) * 2^-24 * sum|Y| / s."""
    T = 14
    geo, frames, Y = G.overlap_add_case(name, T, integers=False)
    rows, _, _ = _overlap_add(handles(name), geo, T, Y, frames)
    worst = 0.0
    for b, f in enumerate(frames):
        fb = geo.frames(f, T)
        Lb = geo.hop * (fb - 1)
        y, bound = G.overlap_add64(Y[b], geo, fb)
        ref, bnd = np.pad(y, geo.half, mode="reflect"), np.pad(bound, geo.half, mode="reflect")
        worst = max(worst, float((np.abs(rows[b, :Lb + geo.n_fft] - ref) / bnd).max()))
        assert not _bits(rows[b, Lb + geo.n_fft:]).any()
    print("%s, random frames: error / bound %.3g" % (name, worst))
    assert worst <= 1.0, worst


# ---- inverse pre-emphasis ----
def _preemphasis(x, frames, fmin, a):
    import torch
    from taco_amd._device import STREAM
    B, L = x.shape
    wav = torch.full((B, L), 7.0, dtype=torch.float32, device="cuda")
    ns = torch.full((B,), -1, dtype=torch.int32, device="cuda")
    _call(None, "taco_debug_gl_inv_preemphasis", STREAM, _dev(x), None if frames is None else _dev(frames), fmin, L + 1, 1, B, C.c_float(a), wav, ns)
    return wav.cpu().numpy(), ns.cpu().numpy()


def _lens(L, fmin, frames):
    return [min(max(int(f), fmin), L + 1) - 1 for f in frames]


@pytest.mark.parametrize("L", G.PREEMPHASIS_LENGTHS)
def test_inv_preemphasis_exact_tiers(L):
    """a = 0: the input's bits, zeros after the row's own samples.  a = 1 on integers in [-8, 8]: an exact prefix sum below 2^24, where any
    mistake in the chunks or the carries changes an integer.  Lengths through hop = 1: one and two samples, both sides of one, two and three
    chunks of 1024 threads, and the workload's 153 300 (C = 150); rows that end inside a chunk, on a chunk boundary and at fmin."""
    fmin, frames, xi = G.preemphasis_case(L, integers=True)
    _, _, xr = G.preemphasis_case(L, integers=False)
    lens = _lens(L, fmin, frames)
    copy, ns = _preemphasis(xr, frames, fmin, 0.0)
    assert ns.tolist() == lens
    for b, n in enumerate(lens):
        assert np.array_equal(_bits(copy[b, :n]), _bits(xr[b, :n])) and not _bits(copy[b, n:]).any(), (L, b)
    summed, ns = _preemphasis(xi, frames, fmin, 1.0)
    assert ns.tolist() == lens
    for b, n in enumerate(lens):
        ref = G.chunked_scan(xi[b], 1.0, L, n)
        assert np.array_equal(ref[:n].astype(np.float64), np.cumsum(xi[b, :n].astype(np.float64)))
        bad = int((_bits(summed[b]) != _bits(ref)).sum())
        assert bad == 0, (L, b, n, bad)
    full, ns = _preemphasis(xi, None, fmin, 1.0)                             # no frames: every row whole
    assert ns.tolist() == [L] * len(lens) and np.array_equal(_bits(full[0]), _bits(summed[0]))
    print("L %d (C %d), rows of %s samples: a = 0 copies, a = 1 is the exact prefix sum (largest %d), 0 of %d words differ"
          % (L, -(-L // 1024), lens, int(np.abs(summed).max()), 2 * summed.size))


@pytest.mark.parametrize("L", G.PREEMPHASIS_LENGTHS)
def test_inv_preemphasis_random_tier(L):
    """a = 0.97 (the reference's value) on random rows against the float64 loop.  The bound is derived from the recurrence in
    gl_reference.preemphasis_bound_units -- the serial part, the carry recurrence over 1024 chunks, the C repeated multiplications in f,
    powf(a, C) -- in units of 2^-24 * max|y|: 329 units at C = 1, 237 at C = 2, 280 at C = 150."""
    fmin, frames, x = G.preemphasis_case(L, integers=False)
    lens = _lens(L, fmin, frames)
    wav, ns = _preemphasis(x, frames, fmin, A97)
    assert ns.tolist() == lens
    units, worst = G.preemphasis_bound_units(A97, L), 0.0
    for b, n in enumerate(lens):
        assert not _bits(wav[b, n:]).any()
        if n:
            ref = G.inv_preemphasis64(x[b, :n], A97)
            worst = max(worst, float(np.abs(wav[b, :n] - ref).max() / (G.U * np.abs(ref).max())))
    print("L %d (C %d), a = 0.97: error %.3g units of 2^-24 max|y| / bound %.0f units = %.3g" % (L, -(-L // 1024), worst, units, worst / units))
    assert worst <= units, (worst, units)


# ---- prologue ----
def _prologue(g, geo, B, T, spec, frames, u, seed=0):
    import torch
    from taco_amd._device import STREAM
    Tr = geo.rows(T)
    S = torch.full((B, Tr, geo.F), 7.0, dtype=torch.float32, device="cuda")
    X = torch.full((B, Tr, 2 * geo.F), 7.0, dtype=torch.float32, device="cuda")
    _call(g, "taco_debug_gl_prologue", g._h, STREAM, _dev(spec), None if frames is None else _dev(frames), None if u is None else _dev(u),
          C.c_ulonglong(seed), B, T, S, X)
    return S.cpu().numpy(), X.cpu().numpy()


@pytest.mark.parametrize("name", ["small", "reference"])
def test_prologue_zero_rows_clip_and_zero_phase(handles, name):
    geo, B, T, frames, spec, u = G.prologue_case(name)
    g = handles(name)
    S, X = _prologue(g, geo, B, T, spec, frames, u)
    for b, f in enumerate(frames):
        fb = geo.frames(f, T)
        assert not _bits(S[b, fb:]).any() and not _bits(X[b, fb:]).any(), b          # rows at or past frames[b], and the Tr - T tail rows
        assert (S[b, :fb] > 0).all()
    Sc, Xc = _prologue(g, geo, B, T, np.clip(spec, 0, 1), frames, u)                 # x <= 0 and x >= 1 give the clipped value's bits
    assert np.array_equal(_bits(S), _bits(Sc)) and np.array_equal(_bits(X), _bits(Xc))
    assert len(set(_bits(S[0, 0, [0, 2, 4]]).tolist())) == 1 and len(set(_bits(S[0, 0, [1, 3, 5]]).tolist())) == 1
    S0, X0 = _prologue(g, geo, B, T, spec, frames, np.zeros_like(u))                 # u = 0: X = [S | 0] exactly
    assert np.array_equal(_bits(S0), _bits(S))
    assert np.array_equal(_bits(X0[..., :geo.F]), _bits(S)) and not _bits(X0[..., geo.F:]).any()
    Sn, Xn = _prologue(g, geo, B, T, spec, None, u)                                  # no frames: every row keeps T
    assert np.array_equal(_bits(Sn[0]), _bits(S[0])) and np.array_equal(_bits(Xn[0]), _bits(X[0])) and (Sn[:, :T] > 0).all() and not _bits(Sn[:, T:]).any()
    print("%s: zero rows, clipped bits and [S | 0] at zero phase hold exactly" % name)


@pytest.mark.parametrize("name", ["small", "reference"])
def test_prologue_with_the_counter_hash_as_phase(handles, name):
    """d_init_uniform NULL: the phase comes from the counter hash of `seed`.  S keeps its bits, the zero rows stay zero, the same seed gives
    the same bits and another seed does not, and every live bin keeps its magnitude: with cos and sin held to 2 ulp of a value below 1
    (4 * 2^-24 each), the vector (cos, sin) is within 4 sqrt(2) * 2^-24 of length 1, and the two products add one rounding:
    | |X| - S | <= (4 sqrt(2) + 1) * 2^-24 * S, 1 % added for the second-order terms."""
    geo, B, T, frames, spec, u = G.prologue_case(name)
    g = handles(name)
    S, _ = _prologue(g, geo, B, T, spec, frames, u)
    Sh, Xh = _prologue(g, geo, B, T, spec, frames, None, seed=11)
    Sh2, Xh2 = _prologue(g, geo, B, T, spec, frames, None, seed=11)
    _, Xo = _prologue(g, geo, B, T, spec, frames, None, seed=12)
    assert np.array_equal(_bits(Sh), _bits(S)) and np.array_equal(_bits(Xh), _bits(Xh2)) and np.array_equal(_bits(Sh), _bits(Sh2))
    assert not np.array_equal(_bits(Xh), _bits(Xo))
    worst, spread = 0.0, []
    for b, f in enumerate(frames):
        fb = geo.frames(f, T)
        assert not _bits(Xh[b, fb:]).any(), b
        s64, x64 = S[b, :fb].astype(np.float64), Xh[b, :fb].astype(np.float64)
        mag = np.hypot(x64[..., :geo.F], x64[..., geo.F:])
        worst = max(worst, float((np.abs(mag - s64) / (1.01 * (4 * np.sqrt(2) + 1) * G.U * s64)).max()))
        spread.append(np.arctan2(x64[..., geo.F:], x64[..., :geo.F]).ravel())
    ph = np.concatenate(spread)
    print("%s, hashed phase: | |X| - S | error / derived bound %.3g; phases in all four quadrants: %s" % (name, worst, [int(((ph >= lo) & (ph < lo + np.pi / 2)).sum()) for lo in (-np.pi, -np.pi / 2, 0, np.pi / 2)]))
    assert worst <= 1.0, worst
    assert all(((ph >= lo) & (ph < lo + np.pi / 2)).mean() > 0.2 for lo in (-np.pi, -np.pi / 2, 0, np.pi / 2))      # a uniform phase, not a constant one


@pytest.mark.parametrize("name", ["small", "reference"])
def test_prologue_on_random_data(handles, name):
    """S against float64 on the same float32 inputs, relative: the error of two nested powf (the inner result's error is multiplied by
    `power`, the exponent's by ln 10 / 20 times its size) is MEASURED, not derived: worst 1.26e-6 on an MI355X over both parameter sets
    (small 1.21e-6, reference 1.26e-6), bar 4 x that = 5.04e-6 (profiles/r28_gl_stages.txt).
    X against float64 from the device's own S, derived: the angle fl(fl(2 pi) u) carries two roundings of a value below 2 pi, so it moves
    by at most 4 pi * 2^-24; sincosf is held to 2 ulp of a value below 1 (4 * 2^-24; HIP documents 1 ulp at most 2); the product with S
    adds one rounding: |error| <= (4 pi + 5) * 2^-24 * S."""
    geo, B, T, frames, spec, u = G.prologue_case(name)
    S, X = _prologue(handles(name), geo, B, T, spec, frames, u)
    es, ex = 0.0, 0.0
    for b, f in enumerate(frames):
        fb = geo.frames(f, T)
        ref = G.magnitudes64(spec[b, :fb], geo.hp)
        es = max(es, float((np.abs(S[b, :fb] - ref) / ref).max()))
        s64 = S[b, :fb].astype(np.float64)
        bound = (4 * np.pi + 5) * G.U * np.concatenate([s64, s64], axis=-1)
        ex = max(ex, float((np.abs(X[b, :fb] - G.init_phase64(s64, u[b, :fb])) / bound).max()))
    print("%s: S relative error %.3g / measured bar %.3g = %.3g; X error / derived bound %.3g" % (name, es, S_REL_BAR, es / S_REL_BAR, ex))
    assert es <= S_REL_BAR, es
    assert ex <= 1.0, ex


# ---- the two DFT products alone ----
def _dft(g, which, exact, rows_t, M, ld, N):
    import torch
    from taco_amd._device import STREAM
    out = torch.full((M, N), 7.0, dtype=torch.float32, device="cuda")
    _call(g, "taco_debug_gl_dft", g._h, STREAM, which, exact, rows_t, C.c_size_t(rows_t.numel()), M, ld, out)
    return out.cpu().numpy()


def _dft_bounds(K, absum):
    """exact-fp32 engine: the dot-product bound K * 2^-24 * sum|a||b|.  Split-bf16 engine, derived from the split: an operand is a = hi + lo
    + r with hi = bf16(a), lo = bf16(a - hi), both round-to-nearest on 8-bit significands, so |lo| <= 2^-9 |a| and |r| <= 2^-18 |a|; the three
    products hi*hi + hi*lo + lo*hi (each exact in float32) leave out lo*lo, r_a*b and a*r_b, 3 * 2^-18 |a||b| (1 % added for the cross
    terms); the 3K products are accumulated in float32, 3K * 2^-24 sum|a||b| at worst."""
    return K * G.U * absum, (3.03 * 2.0 ** -18 + 3 * K * G.U) * absum


@pytest.mark.parametrize("name", ["small", "reference"])
def test_inverse_product_alone(handles, name):
    """X [M, 2F] . IDFT_w [2F, win], M = B * Tr (small: T = 13; reference: T = 24, K = 2050, no multiple of the plane width), against the
    float64 matrix built as gl_create builds it before its cast.  A zero row gives a zero row; a unit row at DC or Nyquist reads that
    row of the matrix alone (weight 1/N, not 2/N), at their imaginary twins a row of zeros."""
    geo, X, zero, units = G.dft_inverse_case(name)
    g = handles(name)
    inv = G.dft_matrices(geo)[1]
    M, K, N = X.shape[0], 2 * geo.F, geo.win
    x64 = X.astype(np.float64)
    ref, absum = x64 @ inv, np.abs(x64) @ np.abs(inv)
    bounds = _dft_bounds(K, absum)
    xt = _dev(X)
    res = []
    for exact in (1, 0):
        Y = _dft(g, 1, exact, xt, M, K, N)
        assert Y.shape == (M, N) and np.isfinite(Y).all()
        assert not _bits(Y[zero]).any()
        for row, k in units.items():
            if k in (geo.F, 2 * geo.F - 1):
                assert not Y[row].any(), (row, k)
        live = bounds[1 - exact] > 0
        assert not live[:, 0].any() and not Y[~live].any()                   # w[0] = 0: column 0 of the matrix is zero, and nothing else may land there
        res.append(float((np.abs(Y - ref)[live] / bounds[1 - exact][live]).max()))
        res.append(float(np.abs(Y - ref).max() / np.abs(ref).max()))
    print("%s inverse product, M %d K %d N %d: exact-fp32 error / bound %.3g (over peak %.3g); split-bf16 error / bound %.3g (over peak %.3g)"
          % ((name, M, K, N) + tuple(res)))
    assert res[0] <= 1.0 and res[2] <= 1.0, res


@pytest.mark.parametrize("name", ["small", "hop30", "reference"])
def test_forward_product_alone_at_the_loops_stride(handles, name):
    """The loop's own read: row t of the frame matrix is ypad[lpad + t*hop ...][0 .. win), ld = hop < K = win, on a padded row of the
    overlap-add test (hop 30: a stride that is no multiple of 4, the scalar load path)."""
    T = {"small": 14, "hop30": 14, "reference": 7}[name]
    geo, frames, Yf = G.overlap_add_case(name, T)
    row, _ = G.overlap_add32(Yf[0], geo, T, T)
    g = handles(name)
    fwd = G.dft_matrices(geo)[0]
    K, N = geo.win, 2 * geo.F
    M = (row.size - geo.lpad - K) // geo.hop + 1
    assert geo.hop < K and M >= T
    frames64 = np.stack([row[geo.lpad + t * geo.hop:geo.lpad + t * geo.hop + K] for t in range(M)]).astype(np.float64)
    ref, absum = frames64 @ fwd, np.abs(frames64) @ np.abs(fwd)
    bounds = _dft_bounds(K, absum)
    xt = _dev(row)[geo.lpad:]
    res = []
    for exact in (1, 0):
        E = _dft(g, 0, exact, xt, M, geo.hop, N)
        live = bounds[1 - exact] > 0
        assert np.isfinite(E).all() and not E[~live].any()
        res.append(float((np.abs(E - ref)[live] / bounds[1 - exact][live]).max()))
        res.append(float(np.abs(E - ref).max() / np.abs(ref).max()))
    print("%s forward product, M %d K %d N %d at stride %d: exact-fp32 error / bound %.3g (over peak %.3g); split-bf16 error / bound %.3g (over peak %.3g)"
          % ((name, M, K, N, geo.hop) + tuple(res)))
    assert res[0] <= 1.0 and res[2] <= 1.0, res
