"""NumPy restatement of taco_spec_warp_map / taco_spec_warp (include/taco_abi.h; kernels in csrc/taco_warp.h).  The map is in int64,
exactly as defined there; the interpolation is in float64 (warp64) and, operation for operation, in float32 (warp32).

The map of row b, with f = clamp(frames[b], 1, T):
  tok(s) = argmax over e of alignments[b, e, s]: the first maximum wins, a NaN counts as the maximum and the first NaN wins (np.argmax).
  Source frame t < f belongs to step t // r; its duration in units of 2^-16 output frame is
      d_t = clamp(lrint(fp32(row_stretch[b] * token_stretch[b, tok(t // r)]) * 65536), 2^12, 2^20),  2^12 for a NaN or a product <= 0.
  C_t = inclusive prefix sum of d_t in int64, C_-1 = 0.  out_frames[b] = clamp((C_{f-1} + 2^15) >> 16, 1, T_out).
  For j < out_frames[b], tau = j << 16: src[b, j] = the t with C_{t-1} <= tau < C_t; frac[b, j] = ((tau - C_{src-1}) << 16) // d_src.
  For j >= out_frames[b]: src = f - 1, frac = 0.
  token_frames[b, e] = the number of t < f with tok(t // r) == e.
The warp, time first, then frequency:
  t0 = src, t1 = min(t0 + 1, f - 1), w_t = frac * 2^-16; v(k) = x[t0, k] when frac == 0, else x[t0, k] + w_t * (x[t1, k] - x[t0, k]);
  v(k) = +0 for k >= W.  No scale: out[j, k] = v(k).  Scale c: q = fp32(k * c), k0 = (int)q, w_f = q - k0; out = v(k0) if w_f == 0, else
  v(k0) + w_f * (v(k0 + 1) - v(k0)); a q outside [0, W) gives +0.  Rows j >= out_frames[b] are +0."""
import numpy as np

D_MIN, D_MAX = 1 << 12, 1 << 20


def durations(product):
    """fp32 products -> int64 durations"""
    p = np.asarray(product, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.rint(np.minimum(p.astype(np.float64), 16.0) * 65536.0)            # exact scaling; rint rounds half to even, like lrint
        d = np.where(p > 0, np.clip(d, D_MIN, D_MAX), D_MIN)                      # NaN > 0 is False
    return d.astype(np.int64)


def tokens_of(alignments):
    """[B, T_in, n_steps] -> [B, n_steps]: np.argmax has the rule (first maximum; a NaN is the maximum, the first NaN wins)"""
    return np.argmax(np.asarray(alignments, np.float32), axis=1)


def warp_map(frames, T, r, T_out, alignments=None, row_stretch=None, token_stretch=None, B=None):
    """-> dict(src, frac [B, T_out] int32, out_frames [B] int32, token_frames [B, T_in] int32 or None, C: per row the int64 prefix sums, f [B])"""
    if alignments is not None:
        alignments = np.asarray(alignments, np.float32)
        B, T_in, n_steps = alignments.shape
        assert T == n_steps * r
        tok = tokens_of(alignments)
    else:
        assert token_stretch is None
        B = B if B is not None else len(frames if frames is not None else row_stretch)
        tok = None
    fs = np.full(B, T, np.int64) if frames is None else np.clip(np.asarray(frames, np.int64), 1, T)
    rs = np.ones(B, np.float32) if row_stretch is None else np.broadcast_to(np.asarray(row_stretch, np.float32), (B,))
    src, frac = np.zeros((B, T_out), np.int32), np.zeros((B, T_out), np.int32)
    out_frames = np.zeros(B, np.int32)
    token_frames = None if tok is None else np.zeros((B, alignments.shape[1]), np.int32)
    Cs = []
    for b in range(B):
        f = int(fs[b])
        t = np.arange(f)
        if token_stretch is not None:
            with np.errstate(invalid="ignore", over="ignore"):
                prod = rs[b] * np.asarray(token_stretch, np.float32)[b, tok[b, t // r]]       # one fp32 product
        else:
            prod = np.full(f, rs[b], np.float32)                                              # times 1 is exact
        d = durations(prod)
        C = np.cumsum(d, dtype=np.int64)
        Cs.append(C)
        of = int(min(max((int(C[-1]) + (1 << 15)) >> 16, 1), T_out))
        out_frames[b] = of
        tau = np.arange(of, dtype=np.int64) << 16
        s = np.searchsorted(C, tau, side="right")                                             # the smallest t with C_t > tau
        assert (s < f).all()
        prev = np.where(s > 0, C[np.maximum(s - 1, 0)], 0)
        src[b, :of] = s
        frac[b, :of] = ((tau - prev) << 16) // d[s]
        src[b, of:] = f - 1
        if tok is not None:
            token_frames[b] = np.bincount(tok[b, t // r], minlength=alignments.shape[1])
    return dict(src=src, frac=frac, out_frames=out_frames, token_frames=token_frames, C=Cs, f=fs.astype(np.int32))


def _warp(spec, frames, m, freq_scale, dt):
    x = np.asarray(spec, np.float32).astype(dt)
    B, T, W = x.shape
    T_out = m["src"].shape[1]
    fs = np.full(B, T, np.int64) if frames is None else np.clip(np.asarray(frames, np.int64), 1, T)
    out = np.zeros((B, T_out, W), dt)
    k = np.arange(W)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            f, of = int(fs[b]), int(m["out_frames"][b])
            t0 = np.clip(m["src"][b, :of].astype(np.int64), 0, f - 1)
            t1 = np.minimum(t0 + 1, f - 1)
            fr = m["frac"][b, :of]
            wt = (fr.astype(np.float32) * np.float32(2.0 ** -16)).astype(dt)[:, None]         # exact in fp32
            a, c = x[b, t0], x[b, t1]
            v = np.where((fr == 0)[:, None], a, a + wt * (c - a))                             # [of, W]: each operation rounded in dt; a copied row takes nothing from next door
            if freq_scale is None:
                out[b, :of] = v
                continue
            q = k.astype(np.float32) * np.float32(np.broadcast_to(np.asarray(freq_scale, np.float32), (B,))[b])      # fp32(k * c), for both precisions
            ok = (q >= 0) & (q < W)
            k0 = np.where(ok, q, 0).astype(np.int64)
            wf = (np.where(ok, q, 0) - k0.astype(np.float32)).astype(dt)[None, :]
            vp = np.concatenate([v, np.zeros((of, 1), dt)], axis=1)                           # v(W) = +0
            v0, v1 = vp[:, k0], vp[:, k0 + 1]
            res = np.where(wf == 0, v0, v0 + wf * (v1 - v0))
            out[b, :of] = np.where(ok[None, :], res, dt(0))
    return out


def warp64(spec, frames, m, freq_scale=None):
    return _warp(spec, frames, m, freq_scale, np.float64)


def warp32(spec, frames, m, freq_scale=None):
    return _warp(spec, frames, m, freq_scale, np.float32)
