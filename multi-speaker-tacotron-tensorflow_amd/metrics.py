"""Distances between feature sequences that are not aligned in time, on the device.  Not in the reference: its test loss
(train.py:158-168) compares output frame t with target frame t, which for a decoder fed its own frames mostly measures the drift in
time; people judge the dumped plots and wavs instead.  Dynamic time warping takes the drift out: the cost of the cheapest monotone
alignment of the two sequences, normalised by their lengths (taco_dtw, csrc/taco_dtw.h; the definition is in include/taco_abi.h and,
as float64 NumPy, in tests/dtw_reference.py).

That distance, on cepstra, measures the spectral envelope.  The source is measured beside it: YIN F0 tracks of a waveform on the
spectrogram's frame grid (f0_track: taco_f0_yin, csrc/taco_f0.h) and, along the warping path, the F0 RMSE in cents and the
voiced/unvoiced error (f0_errors: taco_f0_path_stats); prosody_distance gives all three numbers for two waveform batches."""
import math

import numpy as np
import torch

from . import _lib
from ._device import STREAM, buffers, call, device_of, tensor

COSTS = {"l1": 0, "l2": 1}       # cost_kind of taco_dtw: mean absolute difference per frame / Euclidean distance per frame

# the result tensors (and the workspace) of every shape a call was made with; the next call of that shape reuses them:
# (device, "dtw", B, Ta, Tb, D), (device, "f0", B, L, hop) and (device, "f0_stats", B, Fa, Fb, cap)
_BUFFERS = {}


def dtw_distance(a, b, len_a=None, len_b=None, cost="l1", return_total=False, return_path=False, device=None):
    """Dynamic time warping of a[p, :len_a[p]] onto b[p, :len_b[p]] for every pair p: a [B, Ta, D] and b [B, Tb, D] (device tensors,
    or arrays, which are uploaded), lengths int32 [B] or None for full rows (clamped to [1, T] on the device, never read on the host).
    cost 'l1': c(i, j) = mean_d |a_id - b_jd|; 'l2': sqrt(sum_d (a_id - b_jd)^2).  Steps (i-1,j-1) at weight 2, (i-1,j) and (i,j-1) at
    weight 1; dist = G(n-1, m-1) / (n + m), so for n == m it is at most the mean of c(i, i).  A pair with a NaN or an infinity inside
    its lengths gives NaN; what lies past the lengths is never read.

    Returns dist [B] (float32, on the device; nothing is downloaded and nothing waits).  With return_total also total [B] =
    G(n-1, m-1); with return_path also (path [B, Ta+Tb-1, 2] int32 rows (i, j) from (0, 0) to (n-1, m-1), -1 past path_len; path_len
    [B]).  The result tensors belong to a buffer set kept per shape: the next call of the same shape overwrites them (clone to keep),
    which is also what lets the call be captured in a graph and replayed."""
    lib = _lib.load_library()
    if cost not in COSTS:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "cost must be one of %s, got %r" % (sorted(COSTS), cost))
    dev = torch.device(device) if device is not None else device_of(a, b)
    a, b = tensor(a, dev, torch.float32, "a"), tensor(b, dev, torch.float32, "b")
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "a and b must be [B, Ta, D] and [B, Tb, D], got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    B, Ta, D = a.shape
    Tb = b.shape[1]
    la = None if len_a is None else tensor(len_a, dev, torch.int32, "len_a")
    lb = None if len_b is None else tensor(len_b, dev, torch.int32, "len_b")
    for l in (la, lb):
        if l is not None and tuple(l.shape) != (B,):
            raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "lengths must be [B] = (%d,), got %s" % (B, tuple(l.shape)))
    specs = {"dist": ((B,), torch.float32), "total": ((B,), torch.float32), "ws": ((int(lib.taco_dtw_workspace_bytes(B, Ta, Tb, D)),), torch.uint8)}
    if return_path:
        specs.update(dir=((B, Ta, Tb), torch.uint8), path=((B, Ta + Tb - 1, 2), torch.int32), path_len=((B,), torch.int32))
    buf = buffers(_BUFFERS, (str(dev), "dtw", B, Ta, Tb, D), **specs)
    ws = buf["ws"]            # of no bytes where one strip holds a pair: its pointer is null then
    call(dev, lib.taco_dtw, STREAM, a, la, b, lb, B, Ta, Tb, D, COSTS[cost], buf["dist"], buf["total"], buf["dir"] if return_path else None,
         ws, ws.numel())
    if return_path:
        call(dev, lib.taco_dtw_path, STREAM, buf["dir"], la, lb, B, Ta, Tb, buf["path"], buf["path_len"])
    out = (buf["dist"],)
    if return_total:
        out += (buf["total"],)
    if return_path:
        out += ((buf["path"], buf["path_len"]),)
    return out[0] if len(out) == 1 else out


def mcd_constant():
    """(10 / ln 10) * sqrt(2): decibels per unit of Euclidean cepstral distance"""
    return 10.0 / math.log(10.0) * math.sqrt(2.0)


def mel_cepstra(mel, hparams=None, n_cepstra=13):
    """Normalised mel spectrograms [B, T, M] as the model emits them -> cepstra [B, T, n_cepstra] (float32, on the device
    the input is on):
    L = (clip(x, 0, 1) * -min_level_db + min_level_db) * ln 10 / 20 (the natural log of the mel amplitude that audio/__init__.py's
    _normalize encoded), c_k = sqrt(2/M) * sum_m L_m cos(pi k (m + 1/2) / M) for k = 1 .. n_cepstra (a DCT-II without its k = 0 term,
    which is the level)."""
    from .hparams import hparams as default_hparams
    hp = hparams if hparams is not None else default_hparams
    x = (mel if torch.is_tensor(mel) else torch.as_tensor(np.asarray(mel))).to(torch.float32)      # stays where it is: plumbing
    M = x.shape[-1]
    if not 1 <= n_cepstra < M:
        raise ValueError("n_cepstra must be in [1, %d), got %d" % (M, n_cepstra))
    mdb = float(hp.min_level_db)
    L = (x.clamp(0.0, 1.0) * -mdb + mdb) * (math.log(10.0) / 20.0)
    k = np.arange(1, n_cepstra + 1, dtype=np.float64)[None, :]
    mm = np.arange(M, dtype=np.float64)[:, None]
    basis = torch.as_tensor((math.sqrt(2.0 / M) * np.cos(np.pi * k * (mm + 0.5) / M)).astype(np.float32)).to(x.device)     # [M, n_cepstra]
    return torch.matmul(L, basis).contiguous()


def mel_cepstral_distortion(mel_a, mel_b, len_a=None, len_b=None, hparams=None, n_cepstra=13):
    """Mel-cepstral distortion in dB of two normalised mel spectrograms [B, Ta, M] and [B, Tb, M] as the model emits them, aligned by
    dynamic time warping; returns [B] on the device.

        L_m  = (clip(x_m, 0, 1) * -min_level_db + min_level_db) * ln 10 / 20
        c_k  = sqrt(2 / M) * sum_m L_m cos(pi k (m + 1/2) / M),   k = 1 .. n_cepstra
        MCD  = (10 / ln 10) * sqrt(2) * dtw_distance(c_a, c_b, cost='l2')

    so the number is the mean over the warping path (diagonal steps counted twice, divided by n + m) of the usual per-frame
    (10 / ln 10) sqrt(2 sum_k (c_k - c'_k)^2).  This is this project's own definition, UNPINNED on any MCD package: the cepstra come from
    the model's 80 mel bands and not from a mel-generalised cepstral analysis, and packages differ in the warping steps and in what
    they average over; compare numbers made by this function with each other only.  hparams supplies min_level_db (default: the
    package's hparams)."""
    ca = mel_cepstra(mel_a, hparams, n_cepstra)
    cb = mel_cepstra(mel_b, hparams, n_cepstra)
    return dtw_distance(ca, cb, len_a, len_b, cost="l2") * mcd_constant()


# ---- pitch: YIN F0 tracks, F0 RMSE and V/UV error along a warping path (taco_f0_yin, taco_f0_path_stats: csrc/taco_f0.h) ----
_SPEC = {}                       # (device, the audio hparams' values) -> the audio.Spectrogram handle prosody_distance makes its mels with


def framing(hparams=None):
    """(sample_rate, hop, frame length in samples) as audio.c_audio_hparams reads them and the library's spectrogram frames with"""
    from . import audio
    from .hparams import hparams as default_hparams
    hp = audio.c_audio_hparams(hparams if hparams is not None else default_hparams)
    return int(hp.sample_rate), int(hp.frame_shift_ms / 1000.0 * hp.sample_rate), int(hp.frame_length_ms / 1000.0 * hp.sample_rate)


def f0_track(wav, num_samples=None, hparams=None, fmin=60.0, fmax=500.0, threshold=0.1, window=None, return_aperiodicity=False,
             return_lag=False, device=None):
    """YIN pitch tracks of wav [B, L] (a device tensor, or an array, which is uploaded), row b using its first num_samples[b] samples
    (int32 [B], clamped to [0, L] on the device and never read on the host; None: L).  hop and the default window (the frame length)
    come from hparams as audio.c_audio_hparams reads them, so column t is the frame the spectrogram's column t is centred on:
    F = 1 + L // hop columns, row b owning 1 + n_b // hop of them, exact zeros after.

    This project's own definition, UNPINNED on any pitch-tracking package (include/taco_abi.h; tests/yin_reference.py is it in NumPy):
    with tau_min = floor(sr / fmax), tau_max = ceil(sr / fmin), W = window and x~ the row, zero outside [0, n), frame t reads
    x~[s0 .. s0 + W + tau_max], s0 = t * hop - (W + tau_max) // 2;
        d(tau)  = sum_{j < W} (x~[s0 + j] - x~[s0 + j + tau])^2,           tau = 0 .. tau_max + 1
        d'(tau) = d(tau) * tau / sum_{k = 1 .. tau} d(k),   d'(0) = 1, and 1 where the sum is 0
        tau*    = the first tau in [tau_min, tau_max] with d'(tau) < threshold, walked on to tau + 1 while d' falls: voiced;
                  no such tau: unvoiced, tau* = the first argmin of d' over the range
        f0      = sr / (tau* + delta) when voiced, delta the vertex of the parabola through d'(tau* - 1 .. tau* + 1) clamped to
                  +-0.5 (0 where it opens downwards); exactly 0 when unvoiced.
    A frame that reads a NaN or an infinity gives NaN (lag -1); other frames are not affected.

    Returns f0 [B, F] (float32, on the device; nothing is downloaded and nothing waits); with return_aperiodicity also d'(tau*) [B, F],
    with return_lag also tau* [B, F] int32.  The tensors belong to a buffer set kept per shape: the next call of the same shape overwrites
    them (clone to keep), which is what lets the call be captured in a graph and replayed."""
    lib = _lib.load_library()
    dev = torch.device(device) if device is not None else device_of(wav)
    x = tensor(wav, dev, torch.float32, "wav")
    if x.dim() != 2:
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "wav must be [B, L], got %s" % (tuple(x.shape),))
    B, L = x.shape
    ns = None if num_samples is None else tensor(num_samples, dev, torch.int32, "num_samples")
    if ns is not None and tuple(ns.shape) != (B,):
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "num_samples must be [B] = (%d,), got %s" % (B, tuple(ns.shape)))
    sr, hop, frame = framing(hparams)
    W = frame if window is None else int(window)
    if B < 1 or L < 1 or hop < 1:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "wav [%d, %d] at hop %d: every one must be >= 1" % (B, L, hop))
    F = 1 + L // hop
    specs = {"f0": ((B, F), torch.float32)}
    if return_aperiodicity:
        specs["aper"] = ((B, F), torch.float32)
    if return_lag:
        specs["lag"] = ((B, F), torch.int32)
    buf = buffers(_BUFFERS, (str(dev), "f0", B, L, hop), **specs)
    call(dev, lib.taco_f0_yin, STREAM, x, ns, B, L, sr, hop, W, float(fmin), float(fmax), float(threshold), buf["f0"],
         buf["aper"] if return_aperiodicity else None, buf["lag"] if return_lag else None)
    out = (buf["f0"],)
    if return_aperiodicity:
        out += (buf["aper"],)
    if return_lag:
        out += (buf["lag"],)
    return out[0] if len(out) == 1 else out


def f0_path_stats(f0_a, f0_b, path, path_len):
    """The four sums behind f0_errors, [B, 4] float32 on the device (taco_f0_path_stats): sum of squared cents over the path entries voiced
    on both sides, their number, the entries voiced on one side only, the entries used.  Kept per shape like every result here."""
    lib = _lib.load_library()
    if not (torch.is_tensor(f0_a) and f0_a.is_cuda):
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "f0_a must be a device tensor (f0_track returns one)")
    dev = f0_a.device
    a, b = tensor(f0_a, dev, torch.float32, "f0_a"), tensor(f0_b, dev, torch.float32, "f0_b")
    pth, pl = tensor(path, dev, torch.int32, "path"), tensor(path_len, dev, torch.int32, "path_len")
    if a.dim() != 2 or b.dim() != 2 or pth.dim() != 3 or pth.shape[2] != 2 or not (a.shape[0] == b.shape[0] == pth.shape[0]) or \
            tuple(pl.shape) != (a.shape[0],):
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "f0_a [B, Fa], f0_b [B, Fb], path [B, cap, 2], path_len [B]; got %s, %s, %s, %s"
                             % (tuple(a.shape), tuple(b.shape), tuple(pth.shape), tuple(pl.shape)))
    B, Fa = a.shape
    Fb, cap = b.shape[1], pth.shape[1]
    stats = buffers(_BUFFERS, (str(dev), "f0_stats", B, Fa, Fb, cap), stats=((B, 4), torch.float32))["stats"]
    call(dev, lib.taco_f0_path_stats, STREAM, a, Fa, b, Fb, pth, pl, B, cap, stats)
    return stats


def f0_errors(f0_a, f0_b, path, path_len):
    """F0 RMSE in cents and voiced/unvoiced error of two F0 tracks [B, Fa] and [B, Fb] (f0_track's: 0 = unvoiced) along a warping
    path [B, cap, 2] with path_len [B], as dtw_distance(return_path=True) returns them.  This project's own definition, UNPINNED on
    any evaluation package: over the path entries (i, j) inside both tracks,
        rmse_cents    = sqrt(mean of (1200 * log2(f0_a[i] / f0_b[j]))^2 over the entries voiced on both sides), NaN where there is none;
        vuv_error     = entries voiced on exactly one side / entries used;
        voiced_frames = entries voiced on both sides.
    A NaN in a track at a used entry makes that pair's rmse NaN.  Returns (rmse_cents, vuv_error, voiced_frames), each [B] float32 on
    the device; the sums are taco_f0_path_stats's, the three divisions and the root are torch plumbing.  Nothing is downloaded."""
    s = f0_path_stats(f0_a, f0_b, path, path_len)
    return torch.sqrt(s[:, 0] / s[:, 1]), s[:, 2] / s[:, 3], s[:, 1].clone()


def _spectrogram(hparams, dev):
    from . import audio
    from .hparams import hparams as default_hparams
    h = hparams if hparams is not None else default_hparams
    hp = audio.c_audio_hparams(h)
    key = (str(dev), int(getattr(h, "num_mels", 80))) + tuple(getattr(hp, f) for f, _ in hp._fields_)
    if key not in _SPEC:
        _SPEC[key] = audio.Spectrogram(h, device=dev)
    return _SPEC[key]


def prosody_distance(wav_a, wav_b, num_a=None, num_b=None, hparams=None, **f0_kw):
    """The three objective numbers for two batches of waveforms [B, La] and [B, Lb] (num_a, num_b: samples per row, None = all) in one
    call: mel targets of both by audio.Spectrogram, mel_cepstra of both, dtw_distance(cost='l2', return_path=True) on the cepstra, f0_track
    of both (f0_kw goes to it: fmin, fmax, threshold, window) and f0_errors along the path -- the F0 columns are the spectrogram's frames,
    so the path indexes them directly.  Each piece is this project's own definition, UNPINNED on any package (see mel_cepstral_distortion,
    f0_track, f0_errors).  Returns a dict of [B] device tensors: mcd (dB), f0_rmse_cents, vuv_error, voiced_frames.  Nothing is
    downloaded and nothing waits; the spectrogram handle and every buffer set are kept for the next call."""
    extra = sorted(set(f0_kw) - {"fmin", "fmax", "threshold", "window"})
    if extra:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "prosody_distance passes fmin, fmax, threshold and window on to f0_track, not %s" % ", ".join(extra))
    dev = device_of(wav_a, wav_b)
    a, b = tensor(wav_a, dev, torch.float32, "wav_a"), tensor(wav_b, dev, torch.float32, "wav_b")
    if a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0]:
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "wav_a and wav_b must be [B, La] and [B, Lb], got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    na = None if num_a is None else tensor(num_a, dev, torch.int32, "num_a")
    nb = None if num_b is None else tensor(num_b, dev, torch.int32, "num_b")
    spec = _spectrogram(hparams, dev)
    _, mel_a, frames_a = spec.targets(a, na)
    _, mel_b, frames_b = spec.targets(b, nb)
    ca, cb = mel_cepstra(mel_a, hparams), mel_cepstra(mel_b, hparams)
    dist, (path, path_len) = dtw_distance(ca, cb, frames_a, frames_b, cost="l2", return_path=True)
    mcd = dist * mcd_constant()
    # the two tracks differ in shape or are taken one after the other: the first is cloned out of the buffer set the second may share
    f0_a = f0_track(a, na, hparams, device=dev, **f0_kw).clone()
    f0_b = f0_track(b, nb, hparams, device=dev, **f0_kw)
    rmse, vuv, voiced = f0_errors(f0_a, f0_b, path, path_len)
    return {"mcd": mcd, "f0_rmse_cents": rmse, "vuv_error": vuv, "voiced_frames": voiced}
