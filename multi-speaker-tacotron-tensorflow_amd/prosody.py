"""Control over how a sentence is spoken -- overall rate, the length of single tokens, pitch -- applied to the spectrogram the forward
produced, before any vocoder runs.  Not in the reference: its synthesizer says a sentence at the speed and pitch the model chose.  The
forward gives a magnitude spectrogram and Griffin-Lim invents the phase afterwards, so speed is a resampling of the frame axis and pitch
a resampling of the bin axis, and the alignments say which token every decoder step belongs to, so the stretch can differ per token
(taco_spec_warp_map, taco_spec_warp: csrc/taco_warp.h; the definition is in include/taco_abi.h and, as NumPy, in tests/warp_reference.py).

The time map is defined in integers.  For row b with f = clamp(frames[b], 1, T): tok(s) = argmax over e of alignments[b, e, s] (the first
maximum wins, a NaN counts as the maximum and the first NaN wins); source frame t < f belongs to step t / r and lasts
    d_t = clamp(lrint(fp32(row_stretch[b] * token_stretch[b, tok(t / r)]) * 65536), 2^12, 2^20)
units of 2^-16 output frame (2^12 for a NaN or a non-positive product); C_t is the inclusive prefix sum of d_t in int64, C_-1 = 0;
out_frames[b] = clamp((C_{f-1} + 2^15) >> 16, 1, T_out); output frame j < out_frames[b] sits at tau = j << 16, src[b, j] is the t with
C_{t-1} <= tau < C_t and frac[b, j] = ((tau - C_{src-1}) << 16) / d_src, an integer division, in [0, 65536); for j >= out_frames[b],
src = f - 1 and frac = 0.

Pitch and formants apart (taco_spec_envelope, taco_spec_warp_formant: csrc/taco_envelope.h; tests/envelope_reference.py): the linear output
is normalised dB, affine in log|D|, so the low-quefrency part of a frame's real cepstrum -- a cosine transform of the frame, Q coefficients
kept -- is its spectral envelope, the formants, and the rest the excitation, the harmonics.  warp_formant scales the two along the bin axis
by different factors: the pitch moves and the voice stays, or the other way round."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._device import STREAM, Handle, buffers, call, device_of, lengths, tensor

D_MIN, D_MAX = 1 << 12, 1 << 20      # the shortest and the longest duration of a source frame, in 2^-16 output frame

# the result tensors (and the workspace) of every shape a call was made with; the next call of that shape reuses them:
# (device, "map", B, T, T_out, T_in), (device, "warp", B, T, W, T_out), (device, "envelope", B, T, W, Q) and (device, "formant", B, T, W, T_out)
_BUFFERS = {}
_ENVELOPES = {}                      # (device, W, Q, lifter bytes) -> Envelope


class WarpMap(object):
    """What warp_map returns and warp takes: src, frac [B, T_out] and out_frames [B] (int32, on the device), token_frames [B, T_in] or
    None, and the sizes T (source frames) and T_out (capacity) they were made for."""

    def __init__(self, src, frac, out_frames, token_frames, T, T_out):
        self.src, self.frac, self.out_frames, self.token_frames, self.T, self.T_out = src, frac, out_frames, token_frames, T, T_out


def semitones_to_scale(p):
    """The bin-axis scale that raises the pitch by p semitones: float32(2 ** (-p / 12)); output bin k reads input bin k * scale."""
    return np.float32(2.0 ** (-np.asarray(p, np.float64) / 12.0))


def _host_max(x, what):
    """The largest value of a host-side stretch (None: 1)"""
    if x is None:
        return 1.0
    if torch.is_tensor(x) and x.is_cuda:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "%s is a device tensor: pass out_cap, its default is formed from host-side values only" % what)
    v = np.asarray(x.cpu() if torch.is_tensor(x) else x, np.float64)
    return float(np.nanmax(v)) if v.size and not np.isnan(v).all() else 1.0


def out_frames_bound(T, row_stretch=None, token_stretch=None):
    """The largest out_frames any row of T source frames can reach under host-side stretches, exactly: every duration is at most
    dmax = clamp(lrint(fp32(max row stretch * max token stretch) * 65536), 2^12, 2^20), so C_{f-1} <= T * dmax."""
    p = np.float32(_host_max(row_stretch, "row_stretch")) * np.float32(_host_max(token_stretch, "token_stretch"))
    dmax = D_MIN if not p > 0 else int(min(max(np.rint(min(float(p), 16.0) * 65536.0), D_MIN), D_MAX))
    return max(1, (int(T) * dmax + (1 << 15)) >> 16)


def warp_map(frames, T, reduction_factor, alignments=None, row_stretch=None, token_stretch=None, out_cap=None, return_token_frames=False,
             device=None):
    """The integer time map of the module's header (taco_spec_warp_map), one launch.  frames: int32 [B] -- Synthesizer's trim output as it
    stands, on the device or not -- or None for T; alignments [B, T_in, n_steps] with T == n_steps * reduction_factor, or None;
    row_stretch a scalar or [B], token_stretch [B, T_in] (it needs alignments), None meaning 1.  out_cap, the capacity T_out of the
    map, defaults to ceil(T * max row stretch * max token stretch) + 1 from the host-side values the caller passed: no device read (a
    stretch that is a device tensor therefore needs an explicit out_cap).  A row that would be longer than out_cap is cut there.
    return_token_frames: the map's token_frames is [B, T_in], the source frames t < f attributed to each token (it needs alignments).
    Returns a WarpMap whose tensors belong to a buffer set kept per shape: the next call of the same shape overwrites them (clone to
    keep), which is what lets the call be captured in a graph and replayed.  Nothing is downloaded and nothing waits."""
    lib = _lib.load_library()
    dev = torch.device(device) if device is not None else device_of(alignments, frames, row_stretch, token_stretch)
    T, r = int(T), int(reduction_factor)
    al = None if alignments is None else tensor(alignments, dev, torch.float32, "alignments", ("B", "T_in", "n_steps"))
    if al is not None:
        B, T_in, n_steps = al.shape
    else:
        T_in = n_steps = 0
        first = next((x for x in (frames, row_stretch, token_stretch) if x is not None and (x.dim() if torch.is_tensor(x) else np.ndim(x)) >= 1), None)
        B = 1 if first is None else len(first)
    if out_cap is None:
        p = _host_max(row_stretch, "row_stretch") * _host_max(token_stretch, "token_stretch")
        out_cap = int(math.ceil(T * min(max(p, 1.0 / 16.0), 16.0))) + 1       # (the product as the kernel clamps it: a frame lasts 1/16 .. 16)
    T_out = int(out_cap)
    if B < 1 or T < 1 or T_out < 1:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "B, T and out_cap must be >= 1, got %d, %d, %d" % (B, T, T_out))
    fr = lengths(frames, dev, B, "frames")
    rs = None
    if row_stretch is not None:
        rs = torch.as_tensor(np.asarray(row_stretch, np.float32)) if not torch.is_tensor(row_stretch) else row_stretch
        rs = tensor(rs.expand(B) if rs.dim() == 0 else rs, dev, torch.float32, "row_stretch", (("B", B),))
    ts = None if token_stretch is None else tensor(token_stretch, dev, torch.float32, "token_stretch", (("B", B), ("T_in", T_in)))
    specs = {"src": ((B, T_out), torch.int32), "frac": ((B, T_out), torch.int32), "out_frames": ((B,), torch.int32),
             "ws": ((int(lib.taco_spec_warp_workspace_bytes(B, T)),), torch.uint8)}
    if return_token_frames:
        specs["token_frames"] = ((B, max(T_in, 1)), torch.int32)
    buf = buffers(_BUFFERS, (str(dev), "map", B, T, T_out, T_in), **specs)
    tf = buf["token_frames"] if return_token_frames else None
    call(dev, lib.taco_spec_warp_map, STREAM, al, fr, rs, ts, B, T_in, n_steps, r, T, T_out, buf["src"], buf["frac"], buf["out_frames"], tf,
         buf["ws"], buf["ws"].numel())
    return WarpMap(buf["src"], buf["frac"], buf["out_frames"], tf, T, T_out)


def warp(spec, frames, map, freq_scale=None):
    """The gather and the interpolation (taco_spec_warp), one launch: spec [B, T, W] (the linear outputs, or the mel outputs) with the
    frames the map was made with -> (out [B, T_out, W], out_frames [B]).  Per output element the time interpolation comes first, then the
    frequency interpolation, every operation rounded on its own:
        t0 = src, t1 = min(t0 + 1, f - 1), w_t = frac * 2^-16;  v(k) = x[t0, k] when frac == 0 (the bits are copied), otherwise
        x[t0, k] + w_t * (x[t1, k] - x[t0, k]);  v(k) = +0 for k >= W
        no freq_scale: out[j, k] = v(k);  with c = freq_scale[b] (a scalar or [B]; semitones_to_scale): q = fp32(k * c), k0 = (int)q,
        w_f = q - k0; out = v(k0) if w_f == 0, otherwise v(k0) + w_f * (v(k0 + 1) - v(k0))
    Rows j >= out_frames[b] are +0; nothing at frames >= f of spec is read.  The bin-axis scale moves the formants with the pitch, as a
    resampling-based shift does.  out belongs to a buffer set kept per shape, like the map."""
    lib = _lib.load_library()
    if not (torch.is_tensor(spec) and spec.is_cuda):
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "spec must be a device tensor (the model's linear_outputs or mel_outputs)")
    dev = spec.device
    x = tensor(spec, dev, torch.float32, "spec", ("B", ("T", map.T), "W"))
    B, T, W = x.shape
    if tuple(map.src.shape) != (B, map.T_out):
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "the map is [%d, %d], spec has %d rows" % (tuple(map.src.shape) + (B,)))
    fr = lengths(frames, dev, B, "frames")
    fs = None
    if freq_scale is not None:
        fs = torch.as_tensor(np.asarray(freq_scale, np.float32)) if not torch.is_tensor(freq_scale) else freq_scale
        fs = tensor(fs.expand(B) if fs.dim() == 0 else fs, dev, torch.float32, "freq_scale", (("B", B),))
    out = buffers(_BUFFERS, (str(dev), "warp", B, T, W, map.T_out), out=((B, map.T_out, W), torch.float32))["out"]
    call(dev, lib.taco_spec_warp, STREAM, x, fr, map.src, map.frac, map.out_frames, fs, B, T, W, map.T_out, out)
    return out, map.out_frames


def token_frames(alignments, frames, reduction_factor):
    """The model's own durations: [B, T_in] int32 on the device, the number of source frames t < frames[b] (None: all) whose decoder step
    t / reduction_factor attends most to each token.  Every row sums to its clamped frame count."""
    n_steps = alignments.shape[2]
    return warp_map(frames, n_steps * int(reduction_factor), reduction_factor, alignments=alignments, out_cap=1, return_token_frames=True).token_frames


def cosine_basis(W, Q):
    """basis[n, k] = cos(pi * n * k / (W - 1)) as float64 [Q, W]: what taco_envelope_create takes (the library calls no libm)"""
    n, k = np.arange(int(Q), dtype=np.float64)[:, None], np.arange(int(W), dtype=np.float64)[None, :]
    return np.cos(np.pi * n * k / (int(W) - 1))


def default_order(sample_rate):
    """The highest quefrency the envelope keeps, in samples: 2 ms, the period of 500 Hz, so the cepstral peak of any speaking pitch stays in
    the excitation.  The envelope then has Q = default_order + 1 coefficients (48 and 49 at 24 kHz)."""
    return int(sample_rate * 0.002)


class Envelope(Handle):
    """A taco_envelope handle: the two fp32 tables for frames of W bins and Q cepstral coefficients under a lifter (None: all ones), made
    on the host; the first device call uploads them (it allocates: make it outside graph capture)."""
    _destroy = "taco_envelope_destroy"

    def __init__(self, W, Q, lifter=None, device=None):
        self._lib = _lib.load_library()
        self._h = None
        self.device = torch.device(device if device is not None else "cuda:0")
        self.W, self.Q = int(W), int(Q)
        if self.W < 3 or self.Q < 1 or self.Q > self.W - 1:                  # (before the basis is formed: a negative size is no NumPy error here)
            raise _lib.TacoError(_lib.TACO_ERR_ARG, "W >= 3 and 1 <= Q <= W - 1 are required, got W = %d, Q = %d" % (self.W, self.Q))
        basis = np.ascontiguousarray(cosine_basis(self.W, self.Q))
        lift = None if lifter is None else np.ascontiguousarray(np.asarray(lifter, np.float64))
        if lift is not None and lift.shape != (self.Q,):
            raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "the lifter must be [Q = %d], got shape %s" % (self.Q, lift.shape))
        h = C.c_void_p()
        _lib.check(self._lib.taco_envelope_create(self.W, self.Q, basis.ctypes.data_as(C.c_void_p),
                                                  None if lift is None else lift.ctypes.data_as(C.c_void_p), self.device.index or 0, C.byref(h)))
        self._h = h

    def tables(self):
        """(A, S), float32 [Q, W] each, as the library rounded them"""
        A, S = np.empty((self.Q, self.W), np.float32), np.empty((self.Q, self.W), np.float32)
        _lib.check(self._lib.taco_envelope_tables(self._h, A.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p)))
        return A, S


def _envelope_for(dev, W, order, lifter):
    """The cached handle for frames of W bins on dev.  order: the highest quefrency kept, so Q = order + 1; None: as many as the lifter
    has entries, else Q = min(49, W - 1) -- default_order at 24 kHz."""
    if order is not None:
        Q = int(order) + 1
    elif lifter is not None:
        Q = len(lifter)
    else:
        Q = min(49, W - 1)
    lift = None if lifter is None else np.ascontiguousarray(np.asarray(lifter, np.float64))
    key = (str(dev), W, Q, None if lift is None else lift.tobytes())
    if key not in _ENVELOPES:
        _ENVELOPES[key] = Envelope(W, Q, lift, dev)
    return _ENVELOPES[key]


def _spec(spec, T=None):
    if not (torch.is_tensor(spec) and spec.is_cuda):
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "spec must be a device tensor (the model's linear_outputs)")
    return tensor(spec, spec.device, torch.float32, "spec", ("B", "T" if T is None else ("T", T), "W"))


def _per_row(v, dev, B, what):
    if v is None:
        return None
    v = torch.as_tensor(np.asarray(v, np.float32)) if not torch.is_tensor(v) else v
    return tensor(v.expand(B) if v.dim() == 0 else v, dev, torch.float32, what, (("B", B),))


def envelope(spec, frames=None, order=None, lifter=None, return_cepstrum=False):
    """The spectral envelope of every frame (taco_spec_envelope), one launch: spec [B, T, W], a log-magnitude spectrogram such as the
    model's linear outputs -> env [B, T, W], with return_cepstrum (env, cep [B, T, Q]).  order: the highest quefrency kept in samples
    (Q = order + 1 coefficients; default_order(sample_rate)); lifter [Q] float64 weights on the coefficients, None for all ones.
        c_n = sum_k A[n, k] v_k,  env_k = sum_n S[n, k] c_n  -- fp32 sums against the two tables of taco_envelope_create
    Frames t >= clamp(frames[b], 1, T) are +0 and are not read.  The results belong to a buffer set kept per shape, like warp's."""
    lib = _lib.load_library()
    x = _spec(spec)
    dev = x.device
    B, T, W = x.shape
    h = _envelope_for(dev, W, order, lifter)
    fr = lengths(frames, dev, B, "frames")
    specs = {"env": ((B, T, W), torch.float32)}
    if return_cepstrum:
        specs["cep"] = ((B, T, h.Q), torch.float32)
    buf = buffers(_BUFFERS, (str(dev), "envelope", B, T, W, h.Q), **specs)
    call(dev, lib.taco_spec_envelope, h._h, STREAM, x, fr, B, T, buf["env"], buf["cep"] if return_cepstrum else None)
    return (buf["env"], buf["cep"]) if return_cepstrum else buf["env"]


def warp_formant(spec, frames, map, pitch_scale=None, formant_scale=None, order=None, lifter=None):
    """warp with the pitch and the formants scaled apart (taco_spec_warp_formant), one launch: spec [B, T, W] and a WarpMap ->
    (out [B, T_out, W], out_frames [B]).  Per output frame: v = warp's time interpolation, to the bit; c, env as in envelope, e = v - env;
        out[k] = G(env, formant_scale[b])[k] + G(e, pitch_scale[b])[k]
    with G warp's frequency gather (a scalar or [B] each, semitones_to_scale; None: no scaling of that part).  Equal scales are warp's
    freq_scale up to rounding.  order, lifter: as in envelope.  out belongs to a buffer set kept per shape."""
    lib = _lib.load_library()
    x = _spec(spec, map.T)
    dev = x.device
    B, T, W = x.shape
    if tuple(map.src.shape) != (B, map.T_out):
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "the map is [%d, %d], spec has %d rows" % (tuple(map.src.shape) + (B,)))
    h = _envelope_for(dev, W, order, lifter)
    fr = lengths(frames, dev, B, "frames")
    ps, fs = _per_row(pitch_scale, dev, B, "pitch_scale"), _per_row(formant_scale, dev, B, "formant_scale")
    out = buffers(_BUFFERS, (str(dev), "formant", B, T, W, map.T_out), out=((B, map.T_out, W), torch.float32))["out"]
    call(dev, lib.taco_spec_warp_formant, h._h, STREAM, x, fr, map.src, map.frac, map.out_frames, ps, fs, B, T, map.T_out, out)
    return out, map.out_frames
