"""The spectral envelope and the pitch / formant shift on the device (taco_spec_envelope, taco_spec_warp_formant: csrc/taco_envelope.h)
against the NumPy restatement tests/envelope_reference.py: on the bits where fp32 is exact in any order (Q = 1), on the bits against
taco_spec_warp under a lifter of zeros, random data against float64 within a derived bound at every width and order at which the kernels
change path, equal scales against taco_spec_warp, NaN and length handling, graph replay, and Synthesizer.synthesize_audio(formant=).

THE BOUND of the random tier, u = 2^-24.  Both sides use the same fp32 tables, the same integer map, the same q = fp32(k * s).  The order
of the two sums is the kernel's (eight waves' partial sums over bins taken 16 at a time), so the bound is the one for a sum in ANY order:
a sum of n products formed with one rounding per product and per addition is off by at most (n + 1) u times the sum of the magnitudes
(first order; zero padding adds exact terms only).  Per output frame, from the float64 restatement's own magnitudes:
  v:    taco_spec_warp's time interpolation: dv = 3 u max|x| (tests/test_gpu_warp.py), 0 for taco_spec_envelope, whose v is the input.
  c_n:  dc_n = (W + 1) u sum_k |A[n, k] v_k| + sum_k |A[n, k]| dv.
  env:  denv_k = sum_n |S[n, k]| dc_n + (Q + 1) u sum_n |S[n, k] c_n|.
  e:    de_k = dv + denv_k + u (|v_k| + |env_k|)                    (the subtraction's one rounding)
  G(y): the exact formula on perturbed neighbours is a convex combination, off by at most max_k dy_k; its own three roundings add
        3 u max|y| (test_gpu_warp.py): dG(y) = max_k dy_k + 3 u max_k |y_k|.  Without a scale G is the identity and this still bounds it.
  out:  dG(env) + dG(e) + u (max|env| + max|e|)                     (the one addition)
Every first-order term is itself perturbed by the errors before it, relatively by at most (W + Q + 8) u < 2^-12 here: the bound carries
the factor 1 + 2^-10 for that.  Every element is held to it; rows past the frame counts must be +0 on the bits.

THE EXACT TIER.  Q = 1, W - 1 a power of two at most 2^11, inputs multiples of 2^-8 in [0, 1).  The maps are arbitrary in src and
out_frames; frac is a multiple of 2^12, so w_t is a multiple of 1/16 and v a multiple of 2^-12 in [0, 1): the terms w_k v_k / M are then
multiples of 2^-24 with a sum below 1, and every product and partial sum is exact in fp32 in any order.  (An arbitrary 16-bit w_t puts v on
a grid of 2^-24 and the mean over 2049 bins on one of 2^-36: no fp32 sum is exact there, in any order, so no two orders need agree.)  The
frequency scales are arbitrary: G and the final addition round, the same operations in the same order on both sides."""
import ctypes as C

import numpy as np
import pytest

import envelope_reference as E
import warp_reference as R

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
ORDERS = [1, 2, 3, 33, 49, 128]


def _mods():
    import torch
    from taco_amd import _lib, prosody
    return torch, _lib, prosody


def _info():
    from taco_amd import _lib
    out = (C.c_int * 8)()
    assert _lib.load_library().taco_debug_envelope_info(out, 8) == 0
    return list(out)       # frames per workgroup, wave, tile edge, terms per instruction, widest W, widest W at 16 frames, frames beyond it, largest Q


def _up(x, dtype=None):
    import torch
    return None if x is None else torch.as_tensor(np.asarray(x, dtype)).cuda()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _rand_map(rs, B, T, T_out, frames, frac_step=1):
    """an arbitrary map: any source frame below f, any frac (a multiple of frac_step, zeros among them), any out_frames in [0, T_out]"""
    fs = np.clip(np.asarray(frames), 1, T)
    src = np.stack([rs.randint(0, f, size=T_out) for f in fs]).astype(np.int32)
    frac = (rs.randint(0, 65536 // frac_step, size=(B, T_out)) * frac_step).astype(np.int32)
    frac[rs.rand(B, T_out) < 0.25] = 0
    of = rs.randint(0, T_out + 1, size=B).astype(np.int32)
    of[0] = T_out
    return dict(src=src, frac=frac, out_frames=of)


def _dev_map(m, T):
    _, _, prosody = _mods()
    return prosody.WarpMap(_up(m["src"], np.int32), _up(m["frac"], np.int32), _up(m["out_frames"], np.int32), None, T, m["src"].shape[1])


def _widths():
    rows, wave, tile, kstep, wmax, w16, rows_wide, qmax = _info()
    edges = [tile - 1, tile, tile + 1, w16 - 1, w16, w16 + 1, wmax - 1, wmax]
    return sorted(set([3, 4, 65, 129, 130, 513, 1025, 2049] + edges))


def _env_bounds(v, c, env, A, S, dv):
    """dc [n, Q], denv [n, W], de [n, W] of the module's header for rows v [n, W] of the float64 restatement"""
    W, Q = A.shape[1], A.shape[0]
    aA, aS = np.abs(A.astype(np.float64)), np.abs(S.astype(np.float64))
    dc = (W + 1) * U * (np.abs(v) @ aA.T) + dv * aA.sum(1)[None, :]
    denv = dc @ aS + (Q + 1) * U * (np.abs(c) @ aS)
    de = dv + denv + U * (np.abs(v) + np.abs(env))
    return dc, denv, de


def test_the_widths_sit_on_both_sides_of_every_edge():
    rows, wave, tile, kstep, wmax, w16, rows_wide, qmax = _info()
    ws = _widths()
    assert len(ws) == 16 and ws[0] == 3 and ws[-1] == wmax == 2304 and {1151, 1152, 1153, 15, 16, 17, 2049} <= set(ws)
    assert (rows, rows_wide, qmax) == (16, 8, 128) and max(ORDERS) == qmax


# ---- 1. random data against float64, at every width and order ----
@pytest.mark.parametrize("W", [3, 4, 15, 16, 17, 65, 129, 130, 513, 1025, 1151, 1152, 1153, 2049, 2303, 2304])
def test_random_data_stays_within_the_derived_bound(W):
    torch, _, prosody = _mods()
    assert W in _widths()
    B, T, T_out = 3, 7, 11
    frames = np.array([T, 4, 1])
    for Q in sorted(set(min(q, W - 1) for q in ORDERS)):
        rs = np.random.RandomState(1000 * W + Q)
        x = (rs.rand(B, T, W) - 0.25).astype(np.float32)
        lifter = None if Q % 2 else 0.5 + 0.5 * np.cos(np.pi * np.arange(Q) / Q)
        A, S = E.tables(W, Q, lifter)
        dx, df = _up(x), _up(frames, np.int32)
        # taco_spec_envelope
        env, cep = prosody.envelope(dx, df, order=Q - 1, lifter=lifter, return_cepstrum=True)
        env, cep = env.cpu().numpy(), cep.cpu().numpy()
        renv, rcep = E.envelope(x, frames, A, S)
        worst = 0.0
        for b, f in enumerate(frames):
            dc, denv, _ = _env_bounds(x[b, :f].astype(np.float64), rcep[b, :f], renv[b, :f], A, S, 0.0)
            ec, ee = np.abs(cep[b, :f] - rcep[b, :f]), np.abs(env[b, :f] - renv[b, :f])
            worst = max(worst, float((ec / (dc * SLACK)).max()), float((ee / (denv * SLACK)).max()))
            assert (ec <= dc * SLACK).all() and (ee <= denv * SLACK).all(), (W, Q, b)
            assert not _bits(env[b, f:]).any() and not _bits(cep[b, f:]).any()                      # +0 past the frames
        # taco_spec_warp_formant
        m = _rand_map(rs, B, T, T_out, frames)
        ps, fs = np.array([0.8908987, 1.1224620, 0.3333], np.float32), np.array([1.0594631, 0.7, 2.7], np.float32)
        worst_w = 0.0
        for p, f_ in ((ps, fs), (None, fs), (ps, None), (None, None)):
            out = prosody.warp_formant(dx, df, _dev_map(m, T), _up(p), _up(f_), order=Q - 1, lifter=lifter)[0].cpu().numpy()
            ref, parts = E.warp_formant(x, frames, m, A, S, p, f_, parts=True)
            dv = 3 * U * float(np.abs(x).max())
            for b in range(B):
                of = int(m["out_frames"][b])
                assert not _bits(out[b, of:]).any()
                if of == 0:
                    continue
                v, c, en, e = parts[b]
                _, denv, de = _env_bounds(v, c, en, A, S, dv)
                menv, me = np.abs(en).max(1), np.abs(e).max(1)
                bound = (denv.max(1) + 3 * U * menv + de.max(1) + 3 * U * me + U * (menv + me))[:, None] * SLACK
                err = np.abs(out[b, :of] - ref[b, :of])
                worst_w = max(worst_w, float((err / bound).max()))
                assert (err <= bound).all(), (W, Q, b)
        print("W %d, Q %d: envelope error / bound %.3f, warp_formant error / bound %.3f" % (W, Q, worst, worst_w))


@pytest.mark.parametrize("W,Q", [(130, 49), (1153, 33)])
def test_row_counts_around_the_workgroup_tile(W, Q):
    """B * T and B * T_out one below, at and one above the frames of a workgroup; T = 1"""
    torch, _, prosody = _mods()
    rows, _, _, _, _, w16, rows_wide, _ = _info()
    R_ = rows if W <= w16 else rows_wide
    A, S = E.tables(W, Q)
    shapes = [(1, 1, 1), (1, R_ - 1, R_ + 1), (1, R_, R_ - 1), (1, R_ + 1, R_), (3, 1, R_ // 2 + 1), (2, R_ // 2, R_ // 2), (3, R_ // 2 + 1, 1)]
    for B, T, T_out in shapes:
        rs = np.random.RandomState(B * 100 + T)
        x = rs.rand(B, T, W).astype(np.float32)
        frames = rs.randint(1, T + 1, size=B)
        frames[0] = T
        env = prosody.envelope(_up(x), _up(frames, np.int32), order=Q - 1).cpu().numpy()
        renv, rcep = E.envelope(x, frames, A, S)
        for b, f in enumerate(frames):
            _, denv, _ = _env_bounds(x[b, :f].astype(np.float64), rcep[b, :f], renv[b, :f], A, S, 0.0)
            assert (np.abs(env[b, :f] - renv[b, :f]) <= denv * SLACK).all() and not _bits(env[b, f:]).any(), (B, T)
        m = _rand_map(rs, B, T, T_out, frames)
        m["out_frames"][:] = T_out
        s = np.full(B, 0.9, np.float32)
        out = prosody.warp_formant(_up(x), _up(frames, np.int32), _dev_map(m, T), _up(s), None, order=Q - 1)[0].cpu().numpy()
        ref, parts = E.warp_formant(x, frames, m, A, S, s, None, parts=True)
        dv = 3 * U
        for b in range(B):
            v, c, en, e = parts[b]
            _, denv, de = _env_bounds(v, c, en, A, S, dv)
            menv, me = np.abs(en).max(1), np.abs(e).max(1)
            bound = (denv.max(1) + 3 * U * menv + de.max(1) + 3 * U * me + U * (menv + me))[:, None] * SLACK
            assert (np.abs(out[b] - ref[b]) <= bound).all(), (B, T, T_out, b)


# ---- 2. the exact tier ----
@pytest.mark.parametrize("W", [3, 65, 129, 513, 1025, 2049])
def test_order_one_is_bit_equal_on_exact_data(W):
    torch, _, prosody = _mods()
    rs = np.random.RandomState(W)
    B, T, T_out = 3, 19, 37
    x = (rs.randint(0, 256, size=(B, T, W)) / 256.0).astype(np.float32)
    frames = np.array([T, 11, 1])
    A, S = E.tables(W, 1)
    assert np.array_equal(S, np.ones((1, W), np.float32))
    env, cep = prosody.envelope(_up(x), _up(frames, np.int32), order=0, return_cepstrum=True)
    renv, rcep = E.envelope(x, frames, A, S, np.float32)
    r64 = E.envelope(x, frames, A, S, np.float64)
    assert np.array_equal(renv, r64[0]) and np.array_equal(rcep, r64[1])                             # the restatement met no rounding
    assert np.array_equal(_bits(env.cpu().numpy()), _bits(renv)) and np.array_equal(_bits(cep.cpu().numpy()), _bits(rcep))
    m = _rand_map(rs, B, T, T_out, frames, frac_step=1 << 12)
    assert len(set(m["frac"].ravel().tolist())) >= 8
    for ps, fs in ((rs.uniform(0.3, 2.5, B), rs.uniform(0.3, 2.5, B)), (None, rs.uniform(0.5, 1.5, B)), (rs.uniform(0.5, 1.5, B), None)):
        ps, fs = (None if s is None else s.astype(np.float32) for s in (ps, fs))
        out = prosody.warp_formant(_up(x), _up(frames, np.int32), _dev_map(m, T), _up(ps), _up(fs), order=0)[0].cpu().numpy()
        ref, parts = E.warp_formant(x, frames, m, A, S, ps, fs, dt=np.float32, parts=True)
        p64 = E.warp_formant(x, frames, m, A, S, ps, fs, dt=np.float64, parts=True)[1]
        for (v, c, en, e), (v6, c6, en6, e6) in zip(parts, p64):                                     # v, c, env, e met no rounding
            assert np.array_equal(v, v6) and np.array_equal(c, c6) and np.array_equal(en, en6) and np.array_equal(e, e6)
        assert np.array_equal(_bits(out), _bits(ref)), W


# ---- 3. a lifter of zeros: taco_spec_warp on the bits ----
@pytest.mark.parametrize("W,Q", [(17, 3), (130, 49), (1153, 128)])
def test_a_zero_lifter_is_the_plain_warp_on_the_bits(W, Q):
    torch, _, prosody = _mods()
    rs = np.random.RandomState(W)
    B, T, T_out = 3, 13, 29
    x = rs.standard_normal((B, T, W)).astype(np.float32)
    x[x == 0] = 1.0                                                                                   # no -0 (and no +0 that a sign could reach)
    frames = np.array([T, 6, 2])
    m = _rand_map(rs, B, T, T_out, frames)
    dm, dx, df = _dev_map(m, T), _up(x), _up(frames, np.int32)
    ps = np.array([0.8908987, 1.3, 0.5], np.float32)
    want = prosody.warp(dx, df, dm, _up(ps))[0].cpu().numpy()
    assert np.array_equal(_bits(want), _bits(R.warp32(x, frames, m, ps)))
    for fs in (None, np.array([1.1224620, 0.7, 2.0], np.float32)):
        got = prosody.warp_formant(dx, df, dm, _up(ps), _up(fs), lifter=np.zeros(Q))[0].cpu().numpy()
        assert np.array_equal(_bits(got), _bits(want)), (W, fs is None)
    env = prosody.envelope(dx, df, lifter=np.zeros(Q)).cpu().numpy()
    assert not _bits(env).any()                                                                       # +0 throughout


# ---- 4. equal scales: taco_spec_warp up to rounding ----
@pytest.mark.parametrize("W,Q", [(130, 49), (1025, 49), (2049, 128)])
def test_equal_scales_are_the_plain_warp_up_to_rounding(W, Q):
    """G is linear: G(env) + G(e) = G(env + e), and env + fl(v - env) = v + d with |d| <= u |e|.  Each of the three rounded gathers is off
    its exact formula by at most 3 u max|y| (test_gpu_warp.py), the addition by u (max|env| + max|e|):
    |out - warp| <= u (4 max|env| + 5 max|e| + 3 max|v|) per frame, the magnitudes the fp32 restatement's own."""
    torch, _, prosody = _mods()
    rs = np.random.RandomState(W + 1)
    B, T, T_out = 3, 9, 21
    x = rs.rand(B, T, W).astype(np.float32)
    frames = np.array([T, 5, 1])
    m = _rand_map(rs, B, T, T_out, frames)
    s = np.array([0.8908987, 1.1224620, 0.6], np.float32)
    dm, dx, df = _dev_map(m, T), _up(x), _up(frames, np.int32)
    plain = prosody.warp(dx, df, dm, _up(s))[0].cpu().numpy()
    out = prosody.warp_formant(dx, df, dm, _up(s), _up(s), order=Q - 1)[0].cpu().numpy()
    A, S = E.tables(W, Q)
    parts = E.warp_formant(x, frames, m, A, S, s, s, dt=np.float32, parts=True)[1]
    worst = 0.0
    for b in range(B):
        of = int(m["out_frames"][b])
        assert not _bits(out[b, of:]).any()
        if of == 0:
            continue
        v, c, en, e = (np.abs(a.astype(np.float64)) for a in parts[b])
        bound = U * (4 * en.max(1) + 5 * e.max(1) + 3 * v.max(1))[:, None] * SLACK
        err = np.abs(out[b, :of].astype(np.float64) - plain[b, :of])
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (W, b)
    print("W %d, Q %d: |warp_formant(s, s) - warp(s)| / bound %.3f" % (W, Q, worst))


# ---- 5. NaN and lengths ----
def test_nan_past_the_frames_changes_nothing_and_a_nan_frame_marks_its_readers_only():
    torch, _, prosody = _mods()
    rs = np.random.RandomState(5)
    B, T, T_out, W, Q = 3, 17, 40, 130, 49
    x = rs.rand(B, T, W).astype(np.float32)
    frames = np.array([T, 9, 3])
    m = _rand_map(rs, B, T, T_out, frames)
    ps, fs = np.array([0.9, 0.75, 1.0], np.float32), np.array([1.0, 0.6, 0.8], np.float32)         # at most 1: every output bin reads a source bin
    dm, df = _dev_map(m, T), _up(frames, np.int32)

    def run(a):
        env, cep = prosody.envelope(_up(a), df, order=Q - 1, return_cepstrum=True)
        env, cep = env.cpu().numpy(), cep.cpu().numpy()
        return env, cep, prosody.warp_formant(_up(a), df, dm, _up(ps), _up(fs), order=Q - 1)[0].cpu().numpy()

    clean = run(x)
    assert not any(np.isnan(a).any() for a in clean)
    planted = x.copy()
    for b, f in enumerate(frames):
        planted[b, f:] = np.nan
    for a, c in zip(run(planted), clean):
        assert np.array_equal(_bits(a), _bits(c))
    b0, t0 = 1, 4
    one = x.copy()
    one[b0, t0, 77] = np.nan
    env, cep, out = run(one)
    hit = np.zeros((B, T), bool)
    hit[b0, t0] = True
    for a, c in ((env, clean[0]), (cep, clean[1])):
        assert np.isnan(a[hit]).all() and np.array_equal(_bits(a[~hit]), _bits(c[~hit]))
    f = int(frames[b0])
    src = np.clip(m["src"][b0], 0, f - 1)
    reads = (src == t0) | ((m["frac"][b0] != 0) & (np.minimum(src + 1, f - 1) == t0))
    reads &= np.arange(T_out) < m["out_frames"][b0]
    assert reads.any() and not reads.all()
    hit = np.zeros((B, T_out), bool)
    hit[b0] = reads
    assert np.isnan(out[hit]).all() and np.array_equal(_bits(out[~hit]), _bits(clean[2][~hit]))


def test_lengths_are_clamped_and_null_means_all():
    torch, _, prosody = _mods()
    rs = np.random.RandomState(6)
    B, T, W, Q = 3, 10, 65, 33
    x = _up(rs.rand(B, T, W), np.float32)
    m = _rand_map(rs, B, T, 15, [T, T, 1])
    dm = _dev_map(m, T)
    s = _up([0.9, 1.1, 1.0], np.float32)
    want = [a.clone() for a in prosody.envelope(x, _up([T, T, 1], np.int32), order=Q - 1, return_cepstrum=True)]
    want.append(prosody.warp_formant(x, _up([T, T, 1], np.int32), dm, s, None, order=Q - 1)[0].clone())
    got = [a.clone() for a in prosody.envelope(x, _up([T + 5, 2 ** 31 - 1, 0], np.int32), order=Q - 1, return_cepstrum=True)]
    got.append(prosody.warp_formant(x, _up([T + 5, T, -3], np.int32), dm, s, None, order=Q - 1)[0].clone())
    for a, b in zip(got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not want[0][2, 1:].view(torch.int32).any() and want[0][2, 0].abs().max() > 0
    full = [a.clone() for a in prosody.envelope(x, None, order=Q - 1, return_cepstrum=True)]
    allT = [a.clone() for a in prosody.envelope(x, _up([T, T, T], np.int32), order=Q - 1, return_cepstrum=True)]
    for a, b in zip(full, allT):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    m2 = _rand_map(rs, B, T, 15, [T, T, T])
    a = prosody.warp_formant(x, None, _dev_map(m2, T), s, s, order=Q - 1)[0].clone()
    b = prosody.warp_formant(x, _up([T, T, T], np.int32), _dev_map(m2, T), s, s, order=Q - 1)[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 6. graph capture and replay ----
def test_second_call_and_graph_replay_give_the_same_bits():
    torch, _, prosody = _mods()
    rs = np.random.RandomState(11)
    B, T, T_out, W, Q = 3, 20, 45, 257, 49
    x = _up(rs.rand(B, T, W), np.float32)
    frames = _up([T, 12, 5], np.int32)
    dm = _dev_map(_rand_map(rs, B, T, T_out, [T, 12, 5]), T)
    ps, fs = _up([0.9, 1.0, 1.3], np.float32), _up([1.1, 0.8, 1.0], np.float32)

    def run():
        env, cep = prosody.envelope(x, frames, order=Q - 1, return_cepstrum=True)
        return env, cep, prosody.warp_formant(x, frames, dm, ps, fs, order=Q - 1)[0]

    first = [t.clone() for t in run()]                                                               # the handle's first call: outside capture
    outs = run()
    torch.cuda.synchronize()
    for a, b in zip(first, outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                                                        # one stream, one chain of two launches
        captured = run()
    for t in captured:
        t.fill_(-7)
    g.replay()
    torch.cuda.synchronize()
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(captured, outs))                         # the buffer set of the shape, not new memory
    for a, b in zip(first, captured):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert float(first[0].abs().max()) > 0 and float(first[2].abs().max()) > 0


# ---- 7. end to end: Synthesizer.synthesize_audio ----
def test_synthesize_audio_formant(tmp_path):
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

    plain = s.synthesize_audio(tokens=ids, seed=3)
    assert same(plain, s.synthesize_audio(tokens=ids, seed=3, formant=None)) and s.warped_frames is None
    end = np.asarray(s.spec_end_idx).copy()
    linear = s.model.linear_outputs.clone()
    T = linear.shape[1]
    order = prosody.default_order(1600)
    assert order == 3
    gl = s._griffin_lim()
    for kw, pitch, formant in ((dict(pitch=3, formant=0), 3.0, 0.0), (dict(formant=-2), 0.0, -2.0), (dict(formant=[1.0, -1.0], pitch=[0.0, 2.0]), [0.0, 2.0], [1.0, -1.0])):
        got = s.synthesize_audio(tokens=ids, seed=3, **kw)
        assert np.array_equal(s.spec_end_idx, end) and np.array_equal(s.warped_frames, np.clip(end, 1, T))      # the identity map
        frames = _up(end, np.int32)
        wmap = prosody.warp_map(frames, T, r, out_cap=prosody.out_frames_bound(T))
        ps = prosody.semitones_to_scale(np.broadcast_to(np.asarray(pitch, np.float64), (2,)))
        fs = prosody.semitones_to_scale(np.broadcast_to(np.asarray(formant, np.float64), (2,)))
        spec, of = prosody.warp_formant(linear, frames, wmap, ps, fs, order=order)
        wav, n = gl.inv_spectrogram_rows(spec, of, seed=3)
        pcm = gl.pcm16(wav, n).cpu().numpy()
        want = [a[:k] for a, k in zip(pcm, n.cpu().numpy())]
        assert same(got, want), kw
        assert not same(got, plain)
    # with a rate: the map of the rate, then the same chain; envelope_order is taken
    got = s.synthesize_audio(tokens=ids, seed=3, rate=0.8, pitch=2, formant=0, envelope_order=5, vocoder="tensorflow")
    frames = _up(end, np.int32)
    row = (1.0 / np.array([0.8, 0.8])).astype(np.float32)
    wmap = prosody.warp_map(frames, T, r, row_stretch=row, out_cap=prosody.out_frames_bound(T, row))
    spec, of = prosody.warp_formant(linear, frames, wmap, prosody.semitones_to_scale([2.0, 2.0]), prosody.semitones_to_scale([0.0, 0.0]), order=5)
    assert np.array_equal(s.warped_frames, of.cpu().numpy())
    tf = s._griffin_lim_tf()
    wav, n = tf.inv_spectrogram_tensorflow(spec, of)
    pcm = tf.pcm16(wav, n).cpu().numpy()
    assert same(got, [a[:k] for a, k in zip(pcm, n.cpu().numpy())])
    with pytest.raises(L.TacoError) as e:
        s.synthesize_audio(tokens=ids, vocoder="mel", formant=1.0)
    assert e.value.code == L.TACO_ERR_ARG
    s.close()
