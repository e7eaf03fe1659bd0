"""Dynamic time warping, the host side (CPU): the float64 restatement tests/dtw_reference.py on cases with known answers, its
properties (dist <= mean diagonal cost, valid paths whose weighted cost is the total), the three C entry points with their prototypes, every
argument error of taco_dtw / taco_dtw_path -- all returned before the first device call, so they are reached here -- and the constant of
mel_cepstral_distortion on a pair of single frames worked by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import dtw_reference as R
from taco_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement on known answers ----
@pytest.mark.parametrize("kind", [0, 1])
def test_identical_sequences_are_at_distance_zero(kind):
    a = np.random.RandomState(0).randn(9, 5)
    total, dist, dr, _ = R.dtw(a, a, kind)
    assert total == 0 and dist == 0
    assert np.array_equal(R.walk(dr, 9, 9), np.stack([np.arange(9)] * 2, 1))          # all ties: the diagonal is tried first


@pytest.mark.parametrize("kind", [0, 1])
def test_one_frame_doubled_costs_nothing(kind):
    a = np.random.RandomState(1).randn(7, 3)
    b = np.concatenate([a[:4], a[3:]])                                              # frame 3 twice
    total, dist, dr, c = R.dtw(a, b, kind)
    assert total == 0 and dist == 0
    path = R.walk(dr, 7, 8)
    assert R.path_is_valid(path, 7, 8) and R.path_cost(path, c) == 0
    assert R.dtw(b, a, kind)[0] == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_a_single_frame_gives_the_plain_sum(kind):
    rs = np.random.RandomState(2)
    a, b = rs.randn(1, 4), rs.randn(6, 4)
    c = R.frame_costs(a, b, kind)
    total, dist, dr, _ = R.dtw(a, b, kind)
    want = 2 * c[0, 0]
    for j in range(1, 6):
        want = want + c[0, j]
    assert total == want and dist == want / 7 and dr[0].tolist() == [0, 2, 2, 2, 2, 2]
    total_t, _, dr_t, _ = R.dtw(b, a, kind)
    assert total_t == want and dr_t[:, 0].tolist() == [0, 1, 1, 1, 1, 1]
    assert R.dtw(a, a[:1] + 1.0, 0)[0] == 2.0                                        # 1 x 1: twice the one cost


def test_three_by_three_worked_by_hand():
    """D = 1, kind 0: a = (0, 2, 3), b = (0, 1, 3), c = |a_i - b_j|:
          c = 0 1 3        G = 0 1 4        dir = 0 2 2
              2 1 1            2 2 3              1 0 0
              3 2 0            5 4 2              1 1 0
    G(1,1): diagonal 0 + 2*1 = 2, from above 1 + 1 = 2, from the left 2 + 1 = 3 -- a tie of the diagonal with the cell above: the diagonal,
    tried first, stays.  G(1,2): diagonal 1 + 2*1 = 3, above 4 + 1 = 5, left 2 + 1 = 3 -- a tie with the left: the diagonal stays.
    G(2,1): diagonal 2 + 2*2 = 6, above 2 + 2 = 4, left 5 + 2 = 7: above.  G(2,2): c = 0, so 2, 3, 4: the diagonal.  total 2, dist 2/6."""
    a, b = np.array([[0.], [2.], [3.]]), np.array([[0.], [1.], [3.]])
    total, dist, dr, c = R.dtw(a, b, 0)
    assert c.tolist() == [[0, 1, 3], [2, 1, 1], [3, 2, 0]]
    assert dr.tolist() == [[0, 2, 2], [1, 0, 0], [1, 1, 0]]
    assert total == 2 and dist == 2 / 6
    path = R.walk(dr, 3, 3)
    assert path.tolist() == [[0, 0], [1, 1], [2, 2]] and R.path_cost(path, c) == 2
    # strictly cheaper candidates do win: a = (0, 1), b = (0, 0, 1), c = [[0, 0, 1], [1, 1, 0]], G row 0 = 0 0 1, G(1,0) = 1;
    # G(1,1): 0 + 2 = 2, above 0 + 1 = 1, left 1 + 1 = 2 -> above; G(1,2): c = 0: 0, 1, 1 -> diagonal.  Transposed, (1,1) comes from the left.
    a2, b2 = np.array([[0.], [1.]]), np.array([[0.], [0.], [1.]])
    t2, _, dr2, _ = R.dtw(a2, b2, 0)
    assert dr2.tolist() == [[0, 2, 2], [1, 1, 0]] and t2 == 0
    t3, _, dr3, _ = R.dtw(b2, a2, 0)
    assert dr3.tolist() == [[0, 2], [1, 2], [1, 0]] and t3 == 0
    assert R.walk(dr3, 3, 2).tolist() == [[0, 0], [1, 0], [2, 1]]


def test_kind_one_is_the_euclidean_distance():
    a, b = np.array([[3., 0.]]), np.array([[0., 4.]])
    assert R.dtw(a, b, 1)[0] == 10.0 and R.dtw(a, b, 0)[0] == 7.0                   # 2 * 5 and 2 * (3 + 4) / 2


@pytest.mark.parametrize("kind", [0, 1])
def test_distance_is_at_most_the_mean_diagonal_cost(kind):
    rs = np.random.RandomState(3)
    for n, D in ((1, 3), (2, 1), (17, 5), (40, 13)):
        a, b = rs.randn(n, D), rs.randn(n, D)
        total, dist, dr, c = R.dtw(a, b, kind)
        diag = np.mean(np.diag(c))
        assert dist <= diag * (1 + 1e-12), (n, D, dist, diag)


@pytest.mark.parametrize("kind", [0, 1])
def test_paths_are_valid_and_cost_the_total(kind):
    rs = np.random.RandomState(4)
    for n, m, D in ((1, 1, 2), (1, 9, 2), (9, 1, 2), (5, 8, 1), (23, 17, 7), (30, 31, 13)):
        a, b = rs.randn(n, D), rs.randn(m, D)
        total, dist, dr, c = R.dtw(a, b, kind)
        path = R.walk(dr, n, m)
        assert R.path_is_valid(path, n, m) and max(n, m) <= len(path) <= n + m - 1
        assert abs(R.path_cost(path, c) - total) <= 1e-12 * total                    # the same terms, added in the same order
        assert dist == total / (n + m)


def test_the_walk_survives_any_bytes():
    rs = np.random.RandomState(5)
    for n, m in ((1, 1), (1, 7), (7, 1), (6, 9), (40, 33)):
        dr = rs.randint(0, 256, size=(n, m)).astype(np.uint8)
        path = R.walk(dr, n, m)
        assert R.path_is_valid(path, n, m) and len(path) <= n + m - 1


@pytest.mark.parametrize("kind", [0, 1])
def test_the_diagonal_form_is_the_cell_by_cell_form(kind):
    """dtw (one anti-diagonal at a time, what the GPU tests use) against dtw_loops (the definition as it reads): same bits, ties included."""
    rs = np.random.RandomState(7)
    for n, m, D, ints in ((1, 1, 1, True), (1, 5, 2, True), (6, 1, 2, True), (9, 13, 1, True), (14, 8, 3, True), (21, 19, 5, False)):
        a = rs.randint(-2, 3, size=(n, D)).astype(np.float64) if ints else rs.randn(n, D)         # small integers: many ties
        b = rs.randint(-2, 3, size=(m, D)).astype(np.float64) if ints else rs.randn(m, D)
        t0, d0, dr0, c0 = R.dtw_loops(a, b, kind)
        t1, d1, dr1, c1 = R.dtw(a, b, kind)
        assert t0 == t1 and d0 == d1 and np.array_equal(dr0, dr1) and np.array_equal(c0, c1)


def test_non_finite_input_and_lengths():
    a, b = np.ones((4, 2)), np.ones((5, 2))
    for bad in (np.nan, np.inf, -np.inf):
        x = a.copy()
        x[2, 1] = bad
        assert np.isnan(R.dtw(x, b, 0)[0]) and np.isnan(R.dtw(b, x, 1)[1])
    assert [R.clamp_len(v, 6) for v in (None, -3, 0, 1, 6, 7, 2 ** 31 - 1)] == [6, 1, 1, 1, 6, 6, 6]
    A = np.random.RandomState(6).randn(2, 6, 3)
    A[:, 4:] = np.nan                                                                 # slack past the lengths is not read
    out = R.dtw_batch(A, A, [4, 0], [3, 9 - 5])
    assert (out[0]["n"], out[0]["m"], out[1]["n"], out[1]["m"]) == (4, 3, 1, 4) and all(np.isfinite(o["total"]) for o in out)


# ---- the C ABI ----
def test_the_three_symbols_exist_with_prototypes_and_declarations():
    lib = _lib.load_library()
    pub = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    for name, nargs in (("taco_dtw_workspace_bytes", 4), ("taco_dtw", 15), ("taco_dtw_path", 9)):
        assert hasattr(lib, name) and name in _lib.PROTOTYPES
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, re.sub(r"/\*.*?\*/", "", pub, flags=re.S))
        assert m, name
        assert len(m.group(1).split(",")) == nargs == len(_lib.PROTOTYPES[name][1]), name
    assert _lib.PROTOTYPES["taco_dtw_workspace_bytes"][0] is C.c_size_t
    dbg = open(os.path.join(ROOT, "include", "taco_debug.h")).read()
    assert "taco_debug_dtw_info" in dbg and "taco_debug_dtw_info" not in pub


def _info():
    out = (C.c_int * 6)()
    assert _lib.load_library().taco_debug_dtw_info(out, 6) == 0
    return list(out)


def test_workspace_query():
    lib = _lib.load_library()
    strip, chunk, dmax, dstep, wave, ring = _info()
    assert strip % wave == 0 and wave % 64 == 0 and chunk & (chunk - 1) == 0 and dmax >= 128 and dmax % dstep == 0 and ring > chunk
    assert lib.taco_dtw_workspace_bytes(3, 50, strip, 80) == 0                        # one strip: nothing is handed over
    assert lib.taco_dtw_workspace_bytes(3, 50, strip + 1, 80) == 3 * 50 * 4          # the last column of a strip, per pair
    assert lib.taco_dtw_workspace_bytes(8, 4000, 4000, 80) == 8 * 4000 * 4
    for bad in ((0, 5, 5, 5), (5, 0, 5, 5), (5, 5, 0, 5), (5, 5, 5, 0), (-1, 5, 5, 5)):
        assert lib.taco_dtw_workspace_bytes(*bad) == 0


def test_every_argument_error_is_returned_without_a_device():
    """The pointers are host arrays: a call that passed the checks would hand them to a kernel, so every call here must fail first."""
    lib = _lib.load_library()
    strip, _, dmax = _info()[:3]
    B, Ta, Tb, D = 2, 6, strip + 3, 4
    a, b = np.zeros((B, Ta, D), np.float32), np.zeros((B, Tb, D), np.float32)
    la, lb = np.zeros(B, np.int32), np.zeros(B, np.int32)
    dist, total = np.zeros(B, np.float32), np.zeros(B, np.float32)
    dr = np.zeros((B, Ta, Tb), np.uint8)
    nws = lib.taco_dtw_workspace_bytes(B, Ta, Tb, D)
    assert nws == B * Ta * 4
    ws = np.zeros(nws, np.uint8)
    P = lambda x, off=0: None if x is None else C.c_void_p(x.ctypes.data + off)

    def call(**kw):
        v = dict(a=P(a), la=P(la), b=P(b), lb=P(lb), B=B, Ta=Ta, Tb=Tb, D=D, kind=0, dist=P(dist), total=P(total), dir=P(dr), ws=P(ws), nws=nws)
        v.update(kw)
        return lib.taco_dtw(None, v["a"], v["la"], v["b"], v["lb"], v["B"], v["Ta"], v["Tb"], v["D"], v["kind"], v["dist"], v["total"], v["dir"],
                            v["ws"], v["nws"])

    ARG, STATE, UNSUP = _lib.TACO_ERR_ARG, _lib.TACO_ERR_STATE, _lib.TACO_ERR_UNSUPPORTED
    for kw in (dict(a=None), dict(b=None), dict(dist=None), dict(ws=None)):                                   # null required pointer
        assert call(**kw) == ARG, kw
    for kw in (dict(B=0), dict(Ta=0), dict(Tb=0), dict(D=0), dict(B=-2), dict(D=-1)):                         # sizes below 1
        assert call(**kw) == ARG, kw
    for kind in (-1, 2, 7):                                                                                  # unknown cost kind
        assert call(kind=kind) == ARG
    overlaps = (dict(dist=P(a)), dict(dist=P(a, a.nbytes - 4)), dict(dist=P(b, 8)), dict(dist=P(la)), dict(dist=P(lb, 4)),   # output on input
                dict(total=P(a, 16)), dict(total=P(lb)), dict(dir=P(b)), dict(dir=P(a, a.nbytes - 1)), dict(ws=P(a)), dict(ws=P(la, 4)),
                dict(total=P(dist)), dict(total=P(dist, 4)), dict(dir=P(dist, 4)), dict(ws=P(dr, dr.nbytes - 1)), dict(ws=P(total, 4)),   # output on output
                dict(dist=P(dr, 1)), dict(dist=P(ws, nws - 4)))
    for kw in overlaps:
        assert call(**kw) == ARG, kw
        assert b"overlap" in lib.taco_last_error()
    assert call(nws=nws - 1) == STATE and call(nws=0) == STATE                                                # a workspace below the query
    big = np.zeros((B, Ta, dmax + 1), np.float32)
    bigb = np.zeros((B, Tb, dmax + 1), np.float32)
    assert call(a=P(big), b=P(bigb), D=dmax + 1) == UNSUP                                                     # D above the maximum
    assert b"%d" % dmax in lib.taco_last_error()

    path, plen = np.zeros((B, Ta + Tb - 1, 2), np.int32), np.zeros(B, np.int32)

    def pcall(**kw):
        v = dict(dir=P(dr), la=P(la), lb=P(lb), B=B, Ta=Ta, Tb=Tb, path=P(path), plen=P(plen))
        v.update(kw)
        return lib.taco_dtw_path(None, v["dir"], v["la"], v["lb"], v["B"], v["Ta"], v["Tb"], v["path"], v["plen"])

    for kw in (dict(dir=None), dict(path=None), dict(plen=None), dict(B=0), dict(Ta=0), dict(Tb=-1),
               dict(path=P(dr)), dict(path=P(la)), dict(path=P(lb, 4)), dict(plen=P(dr, dr.nbytes - 1)), dict(plen=P(la, 4)),
               dict(plen=P(path, path.nbytes - 4)), dict(plen=P(path))):
        assert pcall(**kw) == ARG, kw
    # an overlap says so in its message; the lengths are optional, and without them what is left is still checked.  (A call that passes
    # these checks reaches the launch, so buffers that only touch are tried where a later check still refuses: taco_dtw above.)
    for kw in (dict(path=P(dr, dr.nbytes - 1)), dict(plen=P(lb)), dict(la=None, path=P(lb)), dict(lb=None, plen=P(la)),
               dict(la=None, lb=None, plen=P(path, 8))):
        assert pcall(**kw) == ARG and b"overlap" in lib.taco_last_error(), kw
    back = np.zeros(dr.nbytes + dist.nbytes, np.uint8)                                                        # dir and, touching its end, dist
    assert call(dir=P(back), dist=P(back, dr.nbytes), nws=nws - 1) == STATE
    assert lib.taco_debug_dtw_info(None, 6) == ARG and lib.taco_debug_dtw_info((C.c_int * 6)(), -1) == ARG
    two = (C.c_int * 3)(0, 0, -5)
    assert lib.taco_debug_dtw_info(two, 2) == 0 and two[0] == _info()[0] and two[2] == -5                      # no more than asked for


# ---- the mel-cepstral distortion ----
def test_mcd_on_a_pair_of_single_frames_worked_by_hand():
    """M = 4 bands, min_level_db = -100, frames x = (1, 1, 0.5, 0.5) and y = (1, 1, 1, 1): L = ln10/20 * (0, 0, -50, -50) and 0.  With one
    cepstrum, c_1 = sqrt(2/4) * sum_m L_m cos(pi (m + 1/2) / 4); cos at m = 2, 3 is -sin(pi/8) and -cos(pi/8), so
    c_1(x) = sqrt(1/2) * 2.5 ln10 * (sin(pi/8) + cos(pi/8)), c_1(y) = 0.  One frame against one frame: total = 2 c, dist = c = |c_1(x)|,
    MCD = (10 / ln 10) * sqrt(2) * dist = 25 * (sin(pi/8) + cos(pi/8)) dB: the logarithms cancel."""
    import torch
    from taco_amd import metrics
    hp = type("HP", (), {"min_level_db": -100})()
    x = np.array([[[1.0, 1.0, 0.5, 0.5]]], np.float32)
    y = np.ones((1, 1, 4), np.float32)
    cx, cy = metrics.mel_cepstra(x, hp, 1), metrics.mel_cepstra(torch.as_tensor(y), hp, 1)
    assert tuple(cx.shape) == (1, 1, 1) and float(cy.abs().max()) == 0
    want_c = math.sqrt(0.5) * 2.5 * math.log(10.0) * (math.sin(math.pi / 8) + math.cos(math.pi / 8))
    assert abs(float(cx[0, 0, 0]) - want_c) <= 4 * 2.0 ** -24 * want_c
    total, dist, _, _ = R.dtw(cx[0].numpy(), cy[0].numpy(), 1)
    assert dist == abs(float(cx[0, 0, 0]))
    mcd = metrics.mcd_constant() * dist
    assert metrics.mcd_constant() == 10.0 / math.log(10.0) * math.sqrt(2.0)
    assert abs(mcd - 25.0 * (math.sin(math.pi / 8) + math.cos(math.pi / 8))) <= 1e-5
    # values outside [0, 1] are clipped before the logarithm is undone
    assert torch.equal(metrics.mel_cepstra(np.array([[[1.5, 2.0, 0.5, 0.5]]], np.float32), hp, 1), cx)
    import taco_amd
    assert taco_amd.dtw_distance is metrics.dtw_distance and taco_amd.mel_cepstral_distortion is metrics.mel_cepstral_distortion
    assert callable(taco_amd.Tacotron.mel_dtw)
