"""Distances between feature sequences that are not aligned in time, on the device.  Not in the reference: its test loss
(train.py:158-168) compares output frame t with target frame t, which for a decoder fed its own frames mostly measures the drift in
time; people judge the dumped plots and wavs instead.  Dynamic time warping takes the drift out: the cost of the cheapest monotone
alignment of the two sequences, normalised by their lengths (taco_dtw, csrc/taco_dtw.h; the definition is in include/taco_abi.h and,
as float64 NumPy, in tests/dtw_reference.py)."""
import ctypes as C
import math

import numpy as np

COSTS = {"l1": 0, "l2": 1}       # cost_kind of taco_dtw: mean absolute difference per frame / Euclidean distance per frame

_BUFFERS = {}                    # (device, B, Ta, Tb, D) -> the outputs and workspace of that shape; a call reuses them


def _dev_tensor(x, dtype, device):
    import torch
    if not torch.is_tensor(x):
        x = torch.as_tensor(np.asarray(x))
    return x.to(device=device, dtype=dtype).contiguous()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


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
    import torch
    from . import _lib
    lib = _lib.load_library()
    if cost not in COSTS:
        raise _lib.TacoError(_lib.TACO_ERR_ARG, "cost must be one of %s, got %r" % (sorted(COSTS), cost))
    if device is None:
        device = a.device if torch.is_tensor(a) and a.is_cuda else (b.device if torch.is_tensor(b) and b.is_cuda else
                                                                    torch.device("cuda:%d" % torch.cuda.current_device()))
    dev = torch.device(device)
    a, b = _dev_tensor(a, torch.float32, dev), _dev_tensor(b, torch.float32, dev)
    if a.dim() != 3 or b.dim() != 3 or a.shape[0] != b.shape[0] or a.shape[2] != b.shape[2]:
        raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "a and b must be [B, Ta, D] and [B, Tb, D], got %s and %s" % (tuple(a.shape), tuple(b.shape)))
    B, Ta, D = a.shape
    Tb = b.shape[1]
    la = None if len_a is None else _dev_tensor(len_a, torch.int32, dev)
    lb = None if len_b is None else _dev_tensor(len_b, torch.int32, dev)
    for l in (la, lb):
        if l is not None and tuple(l.shape) != (B,):
            raise _lib.TacoError(_lib.TACO_ERR_SHAPE, "lengths must be [B] = (%d,), got %s" % (B, tuple(l.shape)))
    key = (str(dev), B, Ta, Tb, D)
    buf = _BUFFERS.get(key)
    if buf is None:
        nws = int(lib.taco_dtw_workspace_bytes(B, Ta, Tb, D))
        buf = _BUFFERS[key] = {"dist": torch.empty(B, dtype=torch.float32, device=dev),
                               "total": torch.empty(B, dtype=torch.float32, device=dev),
                               "ws": torch.empty(nws, dtype=torch.uint8, device=dev) if nws else None}
    if return_path and "dir" not in buf:
        buf["dir"] = torch.empty((B, Ta, Tb), dtype=torch.uint8, device=dev)
        buf["path"] = torch.empty((B, Ta + Tb - 1, 2), dtype=torch.int32, device=dev)
        buf["path_len"] = torch.empty(B, dtype=torch.int32, device=dev)
    ws = buf["ws"]
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(lib.taco_dtw(stream, _ptr(a), _ptr(la), _ptr(b), _ptr(lb), B, Ta, Tb, D, COSTS[cost], _ptr(buf["dist"]), _ptr(buf["total"]),
                                _ptr(buf["dir"]) if return_path else None, _ptr(ws), ws.numel() if ws is not None else 0))
        if return_path:
            _lib.check(lib.taco_dtw_path(stream, _ptr(buf["dir"]), _ptr(la), _ptr(lb), B, Ta, Tb, _ptr(buf["path"]), _ptr(buf["path_len"])))
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
    import torch
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
