"""NumPy restatement of taco_envelope_create / taco_spec_envelope / taco_spec_warp_formant (include/taco_abi.h; kernels in
csrc/taco_envelope.h), in float64 and, operation for operation where the order is fixed, in float32.

W >= 3 bins, M = W - 1, Q coefficients kept.  basis[n, k] = cos(pi n k / M) and the lifter l[n] are float64.  The two fp32 tables:
    A[n, k] = fp32((w_k * basis[n, k]) / M),  w_0 = w_M = 0.5, else 1;      S[n, k] = fp32((a_n * l[n]) * basis[n, k]),  a_0 = 1, else 2.
For a frame v:  c_n = sum_k A[n, k] v_k;  env_k = sum_n S[n, k] c_n;  e_k = v_k - env_k.  The order of the two sums is the kernel's, so the
float32 versions here (NumPy's own order) match the device on the bits only where every sum is exact; otherwise the float64 versions and a
derived bound are the yardstick.  Both precisions use the SAME fp32 tables.
taco_spec_warp_formant: v = taco_spec_warp's time interpolation (tests/warp_reference.py), then
    out[j, k] = G(env, formant_scale)[k] + G(e, pitch_scale)[k],   G(y, s): q = fp32(k * s), k0 = (int)q, w_f = q - k0, y(k0) if w_f == 0 else
    y(k0) + w_f * (y(k0 + 1) - y(k0)); y(k >= W) = +0; q outside [0, W) gives +0; no scale: y[k].
Rows j >= out_frames[b] are +0; frames t >= f of taco_spec_envelope's outputs are +0."""
import numpy as np


def cosine_basis(W, Q):
    """[Q, W] float64: cos(pi n k / M)"""
    n, k = np.arange(Q, dtype=np.float64)[:, None], np.arange(W, dtype=np.float64)[None, :]
    return np.cos(np.pi * n * k / (W - 1))


def tables64(W, Q, lifter=None, basis=None):
    """The two tables before the rounding, float64 [Q, W] each, in the order of operations the header states"""
    b = cosine_basis(W, Q) if basis is None else np.asarray(basis, np.float64)
    M = float(W - 1)
    w = np.ones(W)
    w[0] = w[-1] = 0.5
    a = np.full(Q, 2.0)
    a[0] = 1.0
    l = np.ones(Q) if lifter is None else np.asarray(lifter, np.float64)
    return (w[None, :] * b) / M, (a * l)[:, None] * b


def tables(W, Q, lifter=None, basis=None):
    A, S = tables64(W, Q, lifter, basis)
    return A.astype(np.float32), S.astype(np.float32)


def _clamped(frames, B, T):
    return np.full(B, T, np.int64) if frames is None else np.clip(np.asarray(frames, np.int64), 1, T)


def separate(v, A, S, dt):
    """v [..., W] -> (c [..., Q], env, e) in dt; the fp32 tables enter as they are"""
    v = np.asarray(v, np.float32).astype(dt) if np.asarray(v).dtype != dt else v
    with np.errstate(invalid="ignore", over="ignore"):
        c = v @ A.astype(dt).T
        env = c @ S.astype(dt)
        return c, env, v - env


def envelope(spec, frames, A, S, dt=np.float64):
    """taco_spec_envelope -> (env [B, T, W], cep [B, T, Q]); frames t >= f are +0 and are not read"""
    x = np.asarray(spec, np.float32)
    B, T, W = x.shape
    fs = _clamped(frames, B, T)
    env, cep = np.zeros((B, T, W), dt), np.zeros((B, T, A.shape[0]), dt)
    for b in range(B):
        f = int(fs[b])
        c, e, _ = separate(x[b, :f].astype(dt), A, S, dt)
        env[b, :f], cep[b, :f] = e, c
    return env, cep


def time_interp(spec, frames, m, dt):
    """taco_spec_warp's v per row: a list of [out_frames[b], W] arrays in dt, every operation rounded in dt"""
    x = np.asarray(spec, np.float32).astype(dt)
    B, T, W = x.shape
    fs = _clamped(frames, B, T)
    rows = []
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(B):
            f, of = int(fs[b]), int(min(max(m["out_frames"][b], 0), m["src"].shape[1]))
            t0 = np.clip(m["src"][b, :of].astype(np.int64), 0, f - 1)
            t1 = np.minimum(t0 + 1, f - 1)
            fr = np.clip(m["frac"][b, :of].astype(np.int64), 0, 65535)
            wt = (fr.astype(np.float32) * np.float32(2.0 ** -16)).astype(dt)[:, None]
            a, c = x[b, t0], x[b, t1]
            rows.append(np.where((fr == 0)[:, None], a, a + wt * (c - a)))
    return rows


def gather(y, scale, dt):
    """G(y, s) on rows y [n, W]; scale None: y itself"""
    if scale is None:
        return y
    n, W = y.shape
    k = np.arange(W)
    with np.errstate(invalid="ignore", over="ignore"):
        q = k.astype(np.float32) * np.float32(scale)
        ok = (q >= 0) & (q < W)
        k0 = np.where(ok, q, 0).astype(np.int64)
        wf = (np.where(ok, q, 0) - k0.astype(np.float32)).astype(dt)[None, :]
        yp = np.concatenate([y, np.zeros((n, 1), dt)], axis=1)
        y0, y1 = yp[:, k0], yp[:, k0 + 1]
        res = np.where(wf == 0, y0, y0 + wf * (y1 - y0))
        return np.where(ok[None, :], res, dt(0))


def warp_formant(spec, frames, m, A, S, pitch_scale=None, formant_scale=None, dt=np.float64, parts=False):
    """taco_spec_warp_formant -> out [B, T_out, W] in dt (parts: also per row v, c, env, e)"""
    B, T, W = np.asarray(spec).shape
    T_out = m["src"].shape[1]
    out = np.zeros((B, T_out, W), dt)
    ps = None if pitch_scale is None else np.broadcast_to(np.asarray(pitch_scale, np.float32), (B,))
    fs = None if formant_scale is None else np.broadcast_to(np.asarray(formant_scale, np.float32), (B,))
    kept = []
    for b, v in enumerate(time_interp(spec, frames, m, dt)):
        c, env, e = separate(v, A, S, dt)
        with np.errstate(invalid="ignore", over="ignore"):
            out[b, :len(v)] = gather(env, None if fs is None else fs[b], dt) + gather(e, None if ps is None else ps[b], dt)
        kept.append((v, c, env, e))
    return (out, kept) if parts else out
