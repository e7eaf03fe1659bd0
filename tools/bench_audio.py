#!/usr/bin/env python
"""Spectrogram -> waveform (Griffin-Lim, 60 iterations) at the C2 output shape: B=32 utterances x 512 frames x 1025 bins.
Prints one JSON line: audio seconds produced per second, with the NumPy oracle (FFT-based, one utterance) timed beside it.
"rows" holds the per-utterance-length entry point (GriffinLim.inv_spectrogram_rows) timed in the same run, alternating with the
existing one: all rows full (must cost what the existing entry point costs, within that entry point's own window-to-window spread)
and a seeded spread of lengths uniform in [T/4, T], followed by the PCM16 kernel.
`--analysis` measures the other direction, waveform -> linear and mel training targets (Spectrogram.targets) at the C2 target shape --
32 rows x 512 frames = 153 300 samples each: the whole call, k_spec_targets alone (through taco_debug_spec_epilogue on the same number
of frame rows) with the bytes it moves over its time, and the difference of the two medians (k_spec_prepare + the windowed-DFT product; a
difference, not a measurement).  It runs with `--analysis` only, INSTEAD of the synthesis arms, and prints its own JSON line."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch, taco_amd
import audio_oracle as A
B, T, F = 32, 512, 1025
hp = taco_amd.hparams


def analysis():
    import ctypes as C
    sp = taco_amd.Spectrogram(hp)
    M = sp.num_mels
    n_fft = (hp.num_freq - 1) * 2; hop = int(hp.frame_shift_ms / 1000 * hp.sample_rate); win = int(hp.frame_length_ms / 1000 * hp.sample_rate)
    Tr = T + -(-n_fft // hop)                                    # frame rows per utterance slot the product runs over (gl_rows)
    L = 153300                                                   # hop * (T - 1): the samples of a 512-frame C2 target
    assert sp.num_frames(L) == T
    rs = np.random.RandomState(2)
    wav = torch.from_numpy((0.1 * rs.randn(B, L)).astype(np.float32)).cuda()
    ragged = torch.from_numpy(rs.randint(L // 4, L + 1, B).astype(np.int32)).cuda()
    est = torch.from_numpy(rs.randn(1, 2 * F).astype(np.float32)).cuda().repeat(B * T, 1).contiguous()
    lin = torch.empty((B * T, F), dtype=torch.float32, device="cuda"); mel = torch.empty((B * T, M), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    epi = lambda: taco_amd._lib.check(sp._lib.taco_debug_spec_epilogue(sp._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(est), B * T, p(lin), p(mel)))
    arms = {"targets": lambda: sp.targets(wav), "targets_ragged": lambda: sp.targets(wav, ragged), "epilogue": epi}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(5):
        for k, f in arms.items():
            e0.record()
            for _ in range(10):
                f()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 10)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    a, b = sp.targets(wav), sp.targets(wav)
    nbytes = B * T * (2 * F + F + M) * 4                         # est read, linear and mel written
    out = {"metric": "audio seconds analysed per second (waveform -> linear + mel targets)", "value": B * L / hp.sample_rate / (med["targets"] / 1e3),
           "unit": "x realtime", "batch": "B=%d x %d samples -> %d frames x (%d + %d)" % (B, L, T, F, M), "windows": "5 windows of 10 calls per arm, alternating",
           "targets_ms": ms["targets"], "targets_ragged_ms": ms["targets_ragged"], "k_spec_targets_ms": ms["epilogue"],
           "targets_median_minus_k_spec_targets_median_ms": med["targets"] - med["epilogue"], "k_spec_targets_bytes": nbytes,
           "k_spec_targets_GBps": nbytes / (med["epilogue"] / 1e3) / 1e9, "dft_gemm_GFLOP": 2.0 * B * Tr * win * 2 * F / 1e9,
           "identical_bits_on_two_calls": bool(all(torch.equal(x, y) for x, y in zip(a, b))), "finite": bool(torch.isfinite(a[0]).all() and torch.isfinite(a[1]).all())}
    sp.close()
    return out


if "--analysis" in sys.argv:
    print(json.dumps(analysis()))
    sys.exit(0)
gl = taco_amd.GriffinLim(hp)
rs = np.random.RandomState(0)
spec = torch.from_numpy(rs.rand(B, T, F).astype(np.float32)).cuda()
full = torch.full((B,), T, dtype=torch.int32, device="cuda")
ragged = torch.from_numpy(np.random.RandomState(1).randint(T // 4, T + 1, B).astype(np.int32)).cuda()
arms = {"existing": lambda: gl.inv_spectrogram(spec), "rows_full": lambda: gl.inv_spectrogram_rows(spec, full)[0],
        "rows_ragged": lambda: gl.inv_spectrogram_rows(spec, ragged)[0]}
for f in arms.values():
    for _ in range(2):
        f()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 10
def window(f):
    e0.record()
    for _ in range(n):
        out = f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n, out
times = {k: [] for k in arms}
for _ in range(4):                                             # existing, rows_full, existing, rows_ragged: the versions alternate
    for k in ("existing", "rows_full", "existing", "rows_ragged"):
        times[k].append(window(arms[k])[0])
ms, wav = window(arms["existing"]); times["existing"].append(ms)
ms = float(np.median(times["existing"]))
same = bool(torch.equal(arms["rows_full"](), wav))
rw, rn = gl.inv_spectrogram_rows(spec, ragged)
pcm_ms = window(lambda: gl.pcm16(rw, rn))[0]
L = wav.shape[1]; audio_s = B * L / hp.sample_rate
gflop = 2.0 * 2 * (B * (T + 7)) * 1200 * 2050 * 61 / 1e9      # two windowed-DFT products per iteration (+1 synthesis)
ahp = A.AudioHParams()
t0 = time.perf_counter(); A.inv_spectrogram(spec[0].cpu().numpy().astype(np.float64).T, ahp, rs.rand(F, T)); cpu_s = time.perf_counter() - t0
print(json.dumps({"metric": "audio seconds synthesised per second (Griffin-Lim, 60 iterations)", "value": audio_s / (ms / 1e3), "unit": "x realtime",
                  "ms_per_batch": ms, "batch": "B=%d x T=%d frames x %d bins -> %d samples each (%.1f s of audio at %d Hz)" % (B, T, F, L, L / hp.sample_rate, hp.sample_rate),
                  "dft_gemm_TFLOPs_equiv": gflop / ms, "finite": bool(torch.isfinite(wav).all()),
                  "rows": {"windows": "%d calls each, alternating" % n, "existing_ms": times["existing"],
                           "existing_spread_ms": max(times["existing"]) - min(times["existing"]), "rows_full_ms": times["rows_full"],
                           "rows_full_minus_existing_ms": float(np.median(times["rows_full"])) - ms, "rows_full_equals_existing": same,
                           "rows_ragged_ms": times["rows_ragged"], "ragged_frames": "seeded, uniform in [%d, %d], mean %.0f" % (T // 4, T, float(ragged.float().mean())),
                           "ragged_audio_s": float(rn.sum()) / hp.sample_rate, "pcm16_ms": pcm_ms},
                  "cpu_baseline": {"kind": "port", "sample": "oracle/audio_oracle.py (NumPy FFT, float64), 1 utterance", "seconds_per_utterance": cpu_s,
                                   "value": (L / hp.sample_rate) / cpu_s, "unit": "x realtime", "cores": 1}}))
