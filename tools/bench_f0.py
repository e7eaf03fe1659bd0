#!/usr/bin/env python
"""Times pitch tracking on the device (taco_f0_yin / taco_f0_path_stats, csrc/taco_f0.h) at the shape it is for: the C2 output, 32 rows x
512 frames of 24 kHz audio at the model's framing (hop 300, frame 1200; fmin 60 Hz -> 402 lags, 482 400 multiply-adds a frame):

  * k_yin, the register-blocked kernel (taco_f0_yin), and the plain one-lag-per-thread form (taco_debug_f0_yin_plain), alternating in the
    same windows; their outputs are compared (lags and voicing equal, F0 within 1e-3 relative: the two sum in different orders);
  * taco_f0_path_stats on a warping path of the same tracks;
  * metrics.prosody_distance whole (two spectrograms, cepstra, DTW with its path, two F0 tracks, the statistics);
  * a device copy of the waveform as yardstick (the least any pass over the data costs);
  * on the host, one thread: the float64 restatement (tests/yin_reference.py) on a few frames, multiplied up and labelled extrapolated.

The figure to read the kernel against is arithmetic, not bytes (the waveform is 19.6 MB): a pair (j, tau) costs two vector instructions, a
subtraction and an fmaf, so the chip's least time is pairs * 2 / (256 CUs * 4 SIMDs * 32 lanes a clock * clock).  The LDS's least time is
words read per pair / (256 CUs * 32 words a clock (ds_read_b32) * clock): 2 words a pair for the plain form, 40 / 144 for the blocked
one.  Both are printed with the share of each the kernel reaches at the nominal 2.4 GHz, and which of the two is the larger
(`larger_floor`: computed from these counts at that assumed clock, not a measured stall reason; the clock held under load is not measured).

    python tools/bench_f0.py [--windows 5] [--calls 50] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

B, FRAMES, FMIN, FMAX, THR = 32, 512, 60.0, 500.0, 0.1
CLOCK, CUS = 2.4e9, 256


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import taco_amd
    from taco_amd import _lib, metrics
    import yin_reference as R
    if not torch.cuda.is_available():
        sys.exit("bench_f0.py needs a GPU: nothing here is timed on the host in its place")
    lib = _lib.load_library()
    hp = taco_amd.hparams
    sr, hop, W = metrics.framing(hp)
    L = (FRAMES - 1) * hop
    tau_min, tau_max = R.lag_range(sr, FMIN, FMAX)
    info = (C.c_int * 7)()
    _lib.check(lib.taco_debug_f0_info(info, 7))
    plan = (C.c_int * 5)()
    _lib.check(lib.taco_debug_f0_plan(W, tau_max, hop, plan))
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    med = lambda v: float(np.median(v))
    st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # voiced-speech-like rows: a harmonic tone with vibrato, different per row, on a noise floor, with a noise-only stretch
    g = torch.Generator(device="cuda").manual_seed(1)
    t = torch.arange(L, device="cuda", dtype=torch.float64) / sr
    f = torch.linspace(90.0, 320.0, B, device="cuda", dtype=torch.float64)[:, None]
    ph = 2 * np.pi * torch.cumsum(f * (1 + 0.03 * torch.sin(2 * np.pi * 5.0 * t)[None, :]), 1) / sr
    wav = (0.2 * (torch.sin(ph) + 0.5 * torch.sin(2 * ph + 1.0) + 0.25 * torch.sin(3 * ph + 2.0))).float()
    wav += 0.003 * torch.randn((B, L), device="cuda", generator=g)
    wav[:, L // 3:L // 3 + L // 8] = 0.1 * torch.randn((B, L // 8), device="cuda", generator=g)
    wav_b = torch.roll(wav, 1, 0).contiguous()
    F = 1 + L // hop
    assert F == FRAMES
    outs = {k: (torch.empty((B, F), device="cuda"), torch.empty((B, F), device="cuda"), torch.empty((B, F), dtype=torch.int32, device="cuda"))
            for k in ("blocked", "plain")}

    def yin(kind):
        f0, aper, lag = outs[kind]
        fn = lib.taco_f0_yin if kind == "blocked" else lib.taco_debug_f0_yin_plain
        _lib.check(fn(st(), P(wav), None, B, L, sr, hop, W, FMIN, FMAX, THR, P(f0), P(aper), P(lag)))

    def timed(fns, calls):
        """the functions alternate window by window: [per-call ms of every window] per function"""
        for fn in fns:
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        out = [[] for _ in fns]
        for _ in range(a.windows):
            for i, fn in enumerate(fns):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                out[i].append(e0.elapsed_time(e1) / calls)
        return out

    t_blocked, t_plain = timed([lambda: yin("blocked"), lambda: yin("plain")], a.calls)
    torch.cuda.synchronize()
    fb, fp = outs["blocked"][0], outs["plain"][0]
    lag_equal = float((outs["blocked"][2] == outs["plain"][2]).float().mean())
    voiced = fb > 0
    both = voiced & (fp > 0)
    rel = float(((fb - fp).abs()[both] / fb[both]).max()) if bool(both.any()) else 0.0
    assert lag_equal > 0.999 and float((voiced == (fp > 0)).float().mean()) > 0.999 and rel < 1e-3, (lag_equal, rel)

    # a warping path of the tracks: the mel DTW of the two batches (row b against row b - 1), as prosody_distance makes it
    res = {k: v.clone() for k, v in metrics.prosody_distance(wav, wav_b, None, None, hp, fmin=FMIN, fmax=FMAX, threshold=THR).items()}
    spec = metrics._spectrogram(hp, wav.device)
    _, ma, na = spec.targets(wav, None)
    _, mb, nb = spec.targets(wav_b, None)
    _, (path, plen) = metrics.dtw_distance(metrics.mel_cepstra(ma, hp), metrics.mel_cepstra(mb, hp), na, nb, cost="l2", return_path=True)
    path, plen = path.clone(), plen.clone()
    f0_b = torch.roll(fb, 1, 0).contiguous()
    stats = torch.empty((B, 4), device="cuda")
    wav2 = torch.empty_like(wav)

    def path_stats():
        _lib.check(lib.taco_f0_path_stats(st(), P(fb), F, P(f0_b), F, P(path), P(plen), B, path.shape[1], P(stats)))

    t_stats, t_copy = timed([path_stats, lambda: wav2.copy_(wav)], a.calls)
    (t_whole,) = timed([lambda: metrics.prosody_distance(wav, wav_b, None, None, hp, fmin=FMIN, fmax=FMAX, threshold=THR)], max(1, a.calls // 2))

    # the float64 restatement on the host: a few frames of row 0, multiplied up
    x0 = wav[0].cpu().numpy()
    n_host = 8 * hop                                                              # 9 frames
    t0 = time.perf_counter()
    ref = R.yin64(x0[None, :n_host], None, sr, hop, W, FMIN, FMAX, THR)
    one = (time.perf_counter() - t0) / int(ref["frames"][0])
    s0 = lambda t_: t_ * hop - (W + tau_max) // 2
    assert s0(4) + W + tau_max < n_host                                           # frames 0 .. 4 read nothing at or past n_host
    dev_lag = outs["blocked"][2][0, :5].cpu().numpy()
    assert np.array_equal(dev_lag, ref["lag"][0, :5]), (dev_lag, ref["lag"][0, :5])

    pairs = float(B) * F * W * (tau_max + 2)
    valu_s = pairs * 2 / (CUS * 4 * 32 * CLOCK)
    lds_words = {"blocked": float(info[2] + info[2] + info[1] - 1) / (info[2] * info[1]), "plain": 2.0}
    kern = {}
    for name, tw in (("blocked", t_blocked), ("plain", t_plain)):
        ms = med(tw)
        lds_s = pairs * lds_words[name] / (CUS * 32 * CLOCK)
        kern[name] = {"ms": ms, "ms_windows": tw, "multiply_adds_per_s": pairs / (ms * 1e-3), "valu_floor_ms": valu_s * 1e3,
                      "lds_floor_ms": lds_s * 1e3, "lds_words_per_pair": lds_words[name], "share_of_valu_floor": valu_s * 1e3 / ms,
                      "share_of_lds_floor": lds_s * 1e3 / ms, "larger_floor": "LDS reads (ds_read_b32)" if lds_s > valu_s else "fp32 vector issue"}
    line = {"metric": "taco_f0_yin (k_yin: %d frames of a row a workgroup, %d lags x %d j a register block) against the plain one-lag-per-thread "
                      "form, taco_f0_path_stats, prosody_distance whole, a device copy of the waveform" % (plan[3], info[1], info[2]),
            "shape": {"rows": B, "frames": F, "samples_per_row": L, "sample_rate": sr, "hop": hop, "window": W, "tau_min": tau_min, "tau_max": tau_max,
                      "multiply_adds": pairs, "lag_blocks": plan[0], "j_parts": plan[1], "j_per_part": plan[2], "lds_floats": plan[4]},
            "k_yin": kern["blocked"], "k_yin_plain": kern["plain"], "blocked_over_plain": med(t_plain) / med(t_blocked),
            "blocked_vs_plain": {"lags_equal_share": lag_equal, "max_relative_f0_difference": rel},
            "path_stats_ms": med(t_stats), "path_stats_ms_windows": t_stats, "path_len_mean": float(plen.float().mean()),
            "prosody_distance_ms": med(t_whole), "prosody_distance_ms_windows": t_whole,
            "copy_waveform_ms": med(t_copy), "copy_waveform_ms_windows": t_copy, "waveform_bytes": int(wav.numel()) * 4,
            "voiced_share": float(voiced.float().mean()),
            "result_means": {k: float(v[torch.isfinite(v)].mean()) for k, v in res.items()},
            "host": {"float64_numpy_one_frame_ms": one * 1e3, "float64_numpy_all_frames_ms_extrapolated": one * 1e3 * B * F,
                     "note": "tests/yin_reference.py yin64 on %d frames of row 0, times %d frames: extrapolated, not run" % (int(ref["frames"][0]), B * F)},
            "clock_assumed_hz": CLOCK,
            "windows": "%d windows of %d calls per kernel after 2 warm-up calls, the two forms alternating window by window, device events around "
                       "each window; medians" % (a.windows, a.calls),
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f_:
            f_.write(s + "\n")


if __name__ == "__main__":
    main()
