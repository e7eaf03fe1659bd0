"""Dynamic time warping on the device (taco_dtw, taco_dtw_path: csrc/taco_dtw.h) against the float64 restatement tests/dtw_reference.py:
bit equality where fp32 is exact, a derived bound on random data, slack / NaN / length rules, the walk on arbitrary bytes, determinism
under graph replay, and the Python surface (metrics.dtw_distance, mel_cepstral_distortion, Tacotron.mel_dtw).

THE BOUND of the random-data tests.  Inputs are fp32 and enter the restatement unchanged, so only the device's arithmetic differs.  With
u = 2^-24, every fp32 operation returns its exact result times (1 + delta), |delta| <= u.  A frame cost is D differences (each exact
difference times (1 + delta)), their absolute values or squares (the square inside an fmaf: one rounding with the addition), D - 1
additions of non-negative terms, and a scaling by 1/D (two roundings: the reciprocal and the product) or a square root (which halves the
error of the sum and adds one rounding): c_dev = c (1 + theta), |theta| <= gamma_(D+4) in the usual notation gamma_k = k u / (1 - k u),
the differences, the additions and "the sqrt and the 1/D scaling inside the + 4".  The value the device holds for a cell is, for the
path its minima followed, a sum of at most n + m - 1 such costs (a doubling is exact), added one by one: every term non-negative, so
path_dev = path (1 + theta'), |theta'| <= gamma_(n+m+D+4).  `min` adds no rounding and the restatement's own float64 error (2^-53 per
operation) is nine orders below, so with gamma = (n + m + D + 4) * 2^-24

    |total_dev - ref| <= gamma / (1 - gamma) * ref,

as the minimum over paths of values each within that factor of its exact value lies within that factor of the exact minimum.  A path the
device reports need not be the restatement's (near-ties may resolve differently), but it was minimal in fp32, so its exact cost is at most
(1 + gamma/(1-gamma))^2 <= 1 + 2 gamma (1 + o(1)) above ref; [ref, ref * (1 + 2 * gamma)] is asserted with the cost recomputed in float64
(never below ref: rounding is monotone, so the recurrence's minimum is at most any path's sequential sum).  Every test prints measured
error / bound; on an MI355X the largest ratio over all cases here was 0.05 (worst-case bounds of this kind are loose by the square root of
the operation count), so a failure of the bound is a bug, not noise."""
import ctypes as C
import itertools

import numpy as np
import pytest

import dtw_reference as R
import taco_oracle as O
from util import tiny_hp, to_product_hp

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _lib():
    from taco_amd import _lib as L
    return L, L.load_library()


def _widths():
    """(columns of a strip, rows of A staged at a time, largest D, D step, columns of a wave, rows of the LDS ring) of k_dtw, from the library"""
    out = (C.c_int * 6)()
    L, lib = _lib()
    L.check(lib.taco_debug_dtw_info(out, 6))
    return tuple(out)


def _up(x, dtype=None):
    import torch
    return None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype)).cuda()


def _call(A, Bm, la, lb, kind, want_dir=True, want_path=True, fill=0xEE):
    """taco_dtw (+ taco_dtw_path) on the current stream through the C ABI, on buffers of this call's own -> dict of NumPy arrays.  dir is
    pre-filled with `fill`, path with -7, so what the kernels leave untouched shows."""
    import torch
    L, lib = _lib()
    A, Bm = _up(A, np.float32), _up(Bm, np.float32)
    B, Ta, D = A.shape
    Tb = Bm.shape[1]
    dla, dlb = _up(la, np.int32), _up(lb, np.int32)
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    dist = torch.full((B,), -1.0, device="cuda")
    total = torch.full((B,), -1.0, device="cuda")
    dr = torch.full((B, Ta, Tb), fill, dtype=torch.uint8, device="cuda") if want_dir or want_path else None
    nws = int(lib.taco_dtw_workspace_bytes(B, Ta, Tb, D))
    ws = torch.empty(max(nws, 1), dtype=torch.uint8, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.taco_dtw(st, P(A), P(dla), P(Bm), P(dlb), B, Ta, Tb, D, kind, P(dist), P(total), P(dr), P(ws) if nws else None, nws))
    out = dict(dist=dist, total=total, dir=dr)
    if want_path:
        out["path"] = torch.full((B, Ta + Tb - 1, 2), -7, dtype=torch.int32, device="cuda")
        out["path_len"] = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        L.check(lib.taco_dtw_path(st, P(dr), P(dla), P(dlb), B, Ta, Tb, P(out["path"]), P(out["path_len"])))
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _check_path_rows(got, p, n, m, want=None):
    """pair p's path rows: path_len entries inside the rectangle, -1 behind; equal to `want` when given"""
    L = int(got["path_len"][p])
    rows = got["path"][p]
    assert 1 <= L <= n + m - 1, (p, L, n, m)
    assert (rows[L:] == -1).all(), p
    assert (rows[:L, 0] >= 0).all() and (rows[:L, 0] < n).all() and (rows[:L, 1] >= 0).all() and (rows[:L, 1] < m).all(), p
    if want is not None:
        assert L == len(want) and np.array_equal(rows[:L], want), (p, n, m)
    return rows[:L]


# ---- 1. exact cases ----
def _exact_batch(pairs, seed):
    """integer features in [-8, 8], D = 4, mean-absolute cost: every cost is a multiple of 1/4 up to 16 and every G a multiple of 1/4 below 2^17
    (at most 2049 cells at weight 2) -- exact in fp32"""
    rs = np.random.RandomState(seed)
    Ta, Tb = max(n for n, _ in pairs), max(m for _, m in pairs)
    A = rs.randint(-8, 9, size=(len(pairs), Ta, 4)).astype(np.float32)
    Bm = rs.randint(-8, 9, size=(len(pairs), Tb, 4)).astype(np.float32)
    la, lb = np.array([n for n, _ in pairs], np.int32), np.array([m for _, m in pairs], np.int32)
    return A, Bm, la, lb


def _assert_exact(pairs, seed):
    A, Bm, la, lb = _exact_batch(pairs, seed)
    got = _call(A, Bm, la, lb, 0)
    ref = R.dtw_batch(A, Bm, la, lb, 0)
    for p, ((n, m), r) in enumerate(zip(pairs, ref)):
        assert (r["n"], r["m"]) == (n, m)
        assert float(got["total"][p]) == r["total"], (n, m, got["total"][p], r["total"])
        assert got["dist"][p] == np.float32(r["total"]) / np.float32(n + m), (n, m)
        assert np.array_equal(got["dir"][p, :n, :m], r["dir"]), (n, m, np.argwhere(got["dir"][p, :n, :m] != r["dir"])[:4])
        assert (got["dir"][p, n:] == 0xEE).all() and (got["dir"][p, :, m:] == 0xEE).all(), (n, m)          # outside: untouched
        _check_path_rows(got, p, n, m, r["path"])
    return len(pairs)


def test_exact_cases_are_bit_equal():
    """(n, m) over {1, 2, 63, 64, 65, 129}^2 in one batch of 36 ragged pairs: total, every used cell of dir, path and path_len equal the
    restatement's; cells of dir outside the used region keep their fill.  No case is skipped."""
    sizes = (1, 2, 63, 64, 65, 129)
    assert _assert_exact(list(itertools.product(sizes, sizes)), 0) == 36


def test_exact_cases_at_every_width_the_kernel_changes_path():
    """k_dtw's own widths, each - 1, + 0, + 1: the strip of columns (Tb beyond it runs as further strips through the workspace) and two
    strips, the wave inside a strip (its last lane hands over through LDS), the rows of A staged at a time, and the LDS ring (where a
    row's slot wraps).  Odd and even column counts both occur, so a lane's last column is used and unused."""
    strip, chunk, _, _, wave, ring = _widths()
    assert strip % wave == 0 and ring > chunk
    cols = [strip - 1, strip, strip + 1, 2 * strip - 1, 2 * strip, 2 * strip + 1, wave - 1, wave, wave + 1, 2 * wave - 1, 2 * wave, 2 * wave + 1]
    rows = [chunk - 1, chunk, chunk + 1, ring - 1, ring, ring + 1, 2 * chunk, 2 * chunk + 1, ring - chunk, 1, 2, 3]
    pairs = list(zip(rows, cols)) + [(ring + 1, 2 * strip + 1), (1, 2 * strip + 1), (2 * strip + 1, 1), (2, strip + 1), (strip + 1, 2),
                                     (ring, strip + 2), (chunk + 1, strip + wave + 1)]
    assert _assert_exact(pairs, 1) == len(pairs)


# ---- 2. random data under the derived bound ----
RAGGED = ((65, 63), (70, 600), (33, 513), (1, 129), (129, 100))      # 600 and 513 columns: more than one strip (asserted in the test)


@pytest.mark.parametrize("D", [1, 7, 13, 80, 128])
@pytest.mark.parametrize("kind", [0, 1])
def test_random_data_under_the_derived_bound(D, kind):
    """See the module docstring for the derivation.  Ragged lengths inside one batch (600 and 513 columns cross a strip of 512); dir and path are not
    compared with the restatement's: the path must be valid and its float64 cost within [ref, ref * (1 + 2 gamma)]."""
    assert _widths()[0] < 513
    rs = np.random.RandomState(100 + 10 * D + kind)
    Ta, Tb = max(n for n, _ in RAGGED), max(m for _, m in RAGGED)
    A = rs.standard_normal((len(RAGGED), Ta, D)).astype(np.float32)
    Bm = (0.5 * rs.standard_normal((len(RAGGED), Tb, D)) + 0.3).astype(np.float32)
    la, lb = np.array([n for n, _ in RAGGED], np.int32), np.array([m for _, m in RAGGED], np.int32)
    got = _call(A, Bm, la, lb, kind)
    ref = R.dtw_batch(A, Bm, la, lb, kind)
    worst = 0.0
    for p, ((n, m), r) in enumerate(zip(RAGGED, ref)):
        gamma = (n + m + D + 4) * U
        bound = gamma / (1 - gamma) * r["total"]
        err = abs(float(got["total"][p]) - r["total"])
        worst = max(worst, err / bound)
        print("D %3d kind %d  %3d x %3d  total %.9g  ref %.9g  error / bound %.4f" % (D, kind, n, m, got["total"][p], r["total"], err / bound))
        assert err <= bound, (D, kind, n, m, err, bound)
        assert abs(float(got["dist"][p]) - r["dist"]) <= (gamma / (1 - gamma) + U) * r["dist"]                 # one more rounding: the division
        path = _check_path_rows(got, p, n, m)
        assert R.path_is_valid(path, n, m), (n, m)
        assert (got["dir"][p, :n, :m] <= 2).all()
        pc = R.path_cost(path, r["c"])
        print("      path cost / ref - 1 = %.3e   (allowed %.3e)" % (pc / r["total"] - 1, 2 * gamma))
        assert r["total"] <= pc <= r["total"] * (1 + 2 * gamma), (D, kind, n, m, pc, r["total"])
    print("worst error / bound: %.4f" % worst)


# ---- 3. slack and NaN ----
def test_slack_is_never_read_and_a_nan_stays_in_its_pair():
    rs = np.random.RandomState(7)
    strip = _widths()[0]
    Tb = strip + 88                                                                    # two strips: the workspace is in play
    pairs = ((40, Tb), (65, 20), (1, strip + 1), (50, 50), (33, 64))
    Ta, D = 70, 13
    A = rs.standard_normal((len(pairs), Ta, D)).astype(np.float32)
    Bm = rs.standard_normal((len(pairs), Tb, D)).astype(np.float32)
    la, lb = np.array([n for n, _ in pairs], np.int32), np.array([m for _, m in pairs], np.int32)
    for kind in (0, 1):
        base = _call(A, Bm, la, lb, kind)
        assert np.isfinite(base["total"]).all()
        A2, B2 = A.copy(), Bm.copy()
        for p, (n, m) in enumerate(pairs):
            A2[p, n:] = np.nan
            B2[p, m:] = np.nan
        slack = _call(A2, B2, la, lb, kind)
        for k in ("total", "dist"):
            assert np.array_equal(_bits(slack[k]), _bits(base[k])), (kind, k)
        assert np.array_equal(slack["dir"], base["dir"]) and np.array_equal(slack["path"], base["path"])
        for where, val in ((("a", 1, 64, 12), np.nan), (("b", 0, Tb - 1, 0), np.inf), (("a", 3, 0, 5), -np.inf), (("b", 2, strip, 3), np.nan)):
            A3, B3 = A2.copy(), B2.copy()
            side, p, t, d = where
            (A3 if side == "a" else B3)[p, t, d] = val                                 # inside pair p's used region
            got = _call(A3, B3, la, lb, kind, want_dir=False, want_path=False)
            assert np.isnan(got["total"][p]) and np.isnan(got["dist"][p]), (kind, where)
            others = [q for q in range(len(pairs)) if q != p]
            assert np.array_equal(_bits(got["total"][others]), _bits(base["total"][others])), (kind, where)
            assert np.array_equal(_bits(got["dist"][others]), _bits(base["dist"][others])), (kind, where)


# ---- 4. lengths ----
def test_lengths_are_clamped_on_the_device():
    rs = np.random.RandomState(8)
    B, Ta, Tb, D = 6, 20, 30, 7
    A = rs.standard_normal((B, Ta, D)).astype(np.float32)
    Bm = rs.standard_normal((B, Tb, D)).astype(np.float32)
    la = np.array([0, -7, Ta + 5, 3, 2 ** 31 - 1, -2 ** 31], np.int64)
    lb = np.array([Tb + 1, 2, 0, -1, 1, 2 ** 31 - 1], np.int64)
    ca, cb = np.clip(la, 1, Ta), np.clip(lb, 1, Tb)
    got, want = _call(A, Bm, la, lb, 0), _call(A, Bm, ca, cb, 0)
    for k in ("total", "dist", "dir", "path", "path_len"):
        assert np.array_equal(got[k], want[k]), k
    ref = R.dtw_batch(A, Bm, la, lb, 0)
    assert [(r["n"], r["m"]) for r in ref] == list(zip(ca.tolist(), cb.tolist()))
    for p, r in enumerate(ref):
        gamma = (r["n"] + r["m"] + D + 4) * U
        assert abs(float(got["total"][p]) - r["total"]) <= gamma / (1 - gamma) * r["total"]
        _check_path_rows(got, p, r["n"], r["m"])
    full = _call(A, Bm, None, None, 0)                                                # NULL lengths: full rows
    allrows = _call(A, Bm, np.full(B, Ta), np.full(B, Tb), 0)
    assert np.array_equal(_bits(full["total"]), _bits(allrows["total"])) and np.array_equal(full["path"], allrows["path"])


# ---- 5. the walk on arbitrary bytes ----
def test_path_walk_stays_in_range_on_random_bytes():
    """A bound on the walk, which the kernel is required to keep for any content of dir: it returns, every entry is inside the rectangle or
    -1 past path_len, path_len <= n + m - 1, and the entries are what the restatement's walk makes of the same bytes."""
    import torch
    L, lib = _lib()
    rs = np.random.RandomState(9)
    pairs = ((37, 300), (1, 1), (1, 300), (37, 1), (20, 257), (36, 299))
    B, Ta, Tb = len(pairs), 37, 300
    for hi in (256, 4):                                                                # any byte; mostly legal bytes with some 3s
        dr = rs.randint(0, hi, size=(B, Ta, Tb)).astype(np.uint8)
        d_dir = _up(dr)
        la, lb = _up([n for n, _ in pairs], np.int32), _up([m for _, m in pairs], np.int32)
        path = torch.full((B, Ta + Tb - 1, 2), -7, dtype=torch.int32, device="cuda")
        plen = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        P = lambda t: C.c_void_p(t.data_ptr())
        L.check(lib.taco_dtw_path(C.c_void_p(torch.cuda.current_stream().cuda_stream), P(d_dir), P(la), P(lb), B, Ta, Tb, P(path), P(plen)))
        torch.cuda.synchronize()
        got = dict(path=path.cpu().numpy(), path_len=plen.cpu().numpy())
        for p, (n, m) in enumerate(pairs):
            rows = _check_path_rows(got, p, n, m, R.walk(dr[p], n, m))
            assert R.path_is_valid(rows, n, m)


# ---- 6. batch sizes, repeat calls and graph replay ----
@pytest.mark.parametrize("B", [1, 33])
def test_second_call_and_graph_replay_give_the_same_bits(B):
    import torch
    from taco_amd import metrics
    rs = np.random.RandomState(10 + B)
    Ta, Tb, D = 40, _widths()[0] + 88, 13                                              # two strips: the workspace is in play
    a, b = _up(rs.standard_normal((B, Ta, D)), np.float32), _up(rs.standard_normal((B, Tb, D)), np.float32)
    la, lb = _up(rs.randint(1, Ta + 1, size=B), np.int32), _up(rs.randint(1, Tb + 1, size=B), np.int32)

    def run():
        dist, total, (path, plen) = metrics.dtw_distance(a, b, la, lb, cost="l2", return_total=True, return_path=True)
        return dist, total, path, plen

    first = [t.clone() for t in run()]
    outs = run()
    torch.cuda.synchronize()
    second = [t.clone() for t in outs]
    for x, y in zip(first, second):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    ref = R.dtw_batch(a.cpu().numpy(), b.cpu().numpy(), la.cpu().numpy(), lb.cpu().numpy(), 1)
    for p, r in enumerate(ref):
        gamma = (r["n"] + r["m"] + D + 4) * U
        assert abs(float(first[1][p]) - r["total"]) <= gamma / (1 - gamma) * r["total"], p
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                          # one stream, one chain of two launches
        captured = run()
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(captured, outs))           # the buffer set of the shape, not new memory
    for x, y in zip(first, captured):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


# ---- 7. the model surface ----
def _train_setup(B=3, T_in=9, T_out=12, seed=21):
    """the tiny models of tests/test_gpu_grad_stats.py (its hparams pattern, copied)"""
    hp = tiny_hp(attention_type="bah_mon")
    w = O.init_weights(hp, 1, seed)
    ids, L = O.synthetic_inputs(B, T_in, seed + 6, ragged=True)
    rs = np.random.RandomState(seed + 1)
    mt, lt = rs.rand(B, T_out, hp.num_mels), rs.rand(B, T_out, hp.num_freq)
    co = rs.uniform(0.5, 1.5, size=B)
    return hp, w, (ids, L, mt, lt, co)


def test_mel_dtw_on_the_train_and_test_models():
    import torch
    import taco_amd
    from taco_amd import metrics
    hp, w, (ids, L, mt, lt, co) = _train_setup()
    php = to_product_hp(hp)
    model = taco_amd.create_model(php)
    model.load_weights(w)
    model.initialize(ids, L, 1, None, mel_targets=mt, linear_targets=lt, loss_coeff=co, is_randomly_initialized=True)
    test_model = taco_amd.create_model(php).share_variables_with(model)
    test_model.initialize(ids, L, 1, None, mel_targets=mt, linear_targets=lt, loss_coeff=co, rnn_decoder_test_mode=True)
    B, T, M = mt.shape
    tgt = torch.as_tensor(mt).to("cuda", torch.float32)
    seen = []
    for m in (model, test_model):
        d = m.mel_dtw().clone()
        same = metrics.dtw_distance(m.mel_outputs, tgt, None, None, "l1").clone()
        assert torch.equal(d.view(torch.int32), same.view(torch.int32))
        out = m.mel_outputs.cpu().numpy()
        ref = R.dtw_batch(out, tgt.cpu().numpy(), None, None, 0)
        gamma = (2 * T + M + 4) * U
        diag = np.abs(out.astype(np.float64) - tgt.cpu().numpy().astype(np.float64)).mean(axis=2).mean(axis=1)      # the row's un-weighted mel L1
        for p in range(B):
            assert abs(float(d[p]) - ref[p]["dist"]) <= (gamma / (1 - gamma) + U) * ref[p]["dist"], p
            assert ref[p]["dist"] <= diag[p] * (1 + 1e-12)
            assert float(d[p]) <= diag[p] * (1 + gamma / (1 - gamma) + U), (p, float(d[p]), diag[p])
        # ragged lengths reach the kernel in the documented order: outputs first
        lo, lt_ = np.array([T, 5, 1], np.int32), np.array([7, T, 3], np.int32)
        dl = m.mel_dtw(target_lengths=lt_, output_lengths=lo).clone()
        refl = R.dtw_batch(out, tgt.cpu().numpy(), lo, lt_, 0)
        for p in range(B):
            g2 = (int(lo[p]) + int(lt_[p]) + M + 4) * U
            assert abs(float(dl[p]) - refl[p]["dist"]) <= (g2 / (1 - g2) + U) * refl[p]["dist"], p
        seen.append(d.cpu().numpy())
    assert not np.array_equal(seen[0], seen[1])                                        # the two models do differ (one is fed its own outputs)
    # mel-cepstral distortion: the restatement on the same cepstra, scaled by the constant; three more roundings (the division, the constant in fp32, the product)
    n_cep = min(13, M - 1)
    ahp = taco_amd.hparams                                                             # min_level_db lives in the package's audio hparams
    mcd = metrics.mel_cepstral_distortion(test_model.mel_outputs, tgt, hparams=ahp, n_cepstra=n_cep).cpu().numpy()
    ca = metrics.mel_cepstra(test_model.mel_outputs, ahp, n_cep).cpu().numpy()
    cb = metrics.mel_cepstra(tgt, ahp, n_cep).cpu().numpy()
    refc = R.dtw_batch(ca, cb, None, None, 1)
    gamma = (2 * T + n_cep + 4) * U
    for p in range(B):
        want = metrics.mcd_constant() * refc[p]["dist"]
        print("MCD row %d: %.6f dB  restatement %.6f dB" % (p, mcd[p], want))
        assert want > 0 and abs(float(mcd[p]) - want) <= (gamma / (1 - gamma) + 3 * U) * want, p
    fresh = taco_amd.create_model(php)
    with pytest.raises(RuntimeError):
        fresh.mel_dtw()
