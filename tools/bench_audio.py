#!/usr/bin/env python
"""Spectrogram -> waveform (Griffin-Lim, 60 iterations) at the C2 output shape: B=32 utterances x 512 frames x 1025 bins.
Prints one JSON line: audio seconds produced per second, with the NumPy oracle (FFT-based, one utterance) timed beside it.
"rows" holds the per-utterance-length entry point (GriffinLim.inv_spectrogram_rows) timed in the same run, alternating with the
existing one: all rows full (must cost what the existing entry point costs, within that entry point's own window-to-window spread)
and a seeded spread of lengths uniform in [T/4, T], followed by the PCM16 kernel.
`--analysis` measures the other direction, waveform -> linear and mel training targets (Spectrogram.targets) at the C2 target shape --
32 rows x 512 frames = 153 300 samples each: the whole call, k_spec_targets alone (through taco_debug_spec_epilogue on the same number
of frame rows) with the bytes it moves over its time, and the difference of the two medians (k_spec_prepare + the windowed-DFT product; a
difference, not a measurement).  It runs with `--analysis` only, INSTEAD of the synthesis arms, and prints its own JSON line.
`--trim` measures the silence trim of librosa_trim=True (GriffinLim.trim at 5120 / 256 / 50 dB, synthesizer.py:266-269) on a batch of the C2
output shape -- 32 rows x 153 300 samples with the seeded per-utterance lengths of the synthesis arms, each row noise with a quiet last
fifth: the trim alone, the tail of synthesize_audio (pcm16 alone = flag off; trim + end column + pcm16 = flag on), and the float64
restatement tests/trim_reference.py on the CPU for the same batch, whose indices the device must reproduce.  Its own JSON line, `--trim` only.
`--split` measures splitting a recording on silence (audio/silence.py:33-76) on a synthetic recording of three minutes at 24 kHz -- seeded
utterances of 2-9 s, each loud phrases with quieter breaths between short pauses, separated by 0.5-1.5 s of noise floor: the split alone
(GriffinLim.split at 1024 / 256 / 40 dB, one row), the whole taco_amd.split_on_silence (two splits, the intervals gathered, remove_breath at
128 / 32, scattered back, intervals downloaded), and the float64 restatement tests/split_reference.py on the CPU, whose segments the device
must reproduce.  Its own JSON line, `--split` only.
`--resample` measures resampling to the model's rate (audio.Resampler, kaiser_best) on three minutes at 44100 -> 24000 Hz: mono float32
and stereo 16-bit PCM, the call alone (input and outputs on the device), as output samples per second and as the bytes of the stream it
moves (input once, output once) over its time; beside it the vectorised float64 restatement tests/resample_reference.py on the CPU for
the same mono input, whose values bound the device's error; and three minutes at 16000 -> 24000 Hz, mono float32, the up-sampling shape.  Its own JSON line, `--resample` only.
`--vocoders` times the reference's three vocoders in one run at the C2 output shape (32 x 512 frames, 60 iterations), windows alternating: the
existing inv_spectrogram, inv_spectrogram_tensorflow (GriffinLim(flavor="tensorflow")) and inv_melspectrogram (80 mels), plus
k_gl_mel_magnitude alone (GriffinLim.mel_to_linear on the same batch: the kernel without its ^power) -- each arm's ms, the TF arm relative
to the existing one, and k_gl_mel_magnitude relative to one Griffin-Lim iteration of the same run (the existing arm at 60 and at 0 iterations,
their difference over 60).  Its own JSON line, `--vocoders` only.
`--pydub` measures the reference's other way of splitting (audio/silence.py:81-117) and app.py's amplify on three minutes of seeded
speech-like bursts at 44100 Hz, stereo, 16-bit PCM: GriffinLim.nonsilent alone (100 ms / -40 dBFS, the recording on the device), the whole
silence.split_on_silence_pydub and the whole silence.amplify (upload, kernels, tables and results downloaded), windows alternating; the
energy pass alone (k_pcm_energy through taco_debug_pcm_energy: the only launch that reads the samples) with the bytes of the recording
over its time, beside a device copy of the same buffer (which reads and writes those bytes); and on the host the restatement tests/pydub_reference.py: its
fast form on the whole recording and its literal audioop form on the first ten seconds ("literal, 10 s": not extrapolated).  Its own JSON
line, `--pydub` only.
`--momentum` measures Fast Griffin-Lim (GriffinLim.set_momentum) at the C2 output shape on a CONSISTENT spectrogram -- the STFT
magnitudes of 32 seeded multi-tone signals of 153 300 samples (Spectrogram.targets on the device, re-encoded so that the vocoder's
magnitudes are exactly those), not noise: momentum 0 and 0.99 at 10, 20, 30 and 60 iterations, five windows of four calls per cell with
the two settings alternating, and for each cell the mean and the worst spectral convergence of the batch as the device reports it
(GriffinLim.convergence).  From them: the smallest iteration count at which 0.99 is at or below the plain loop's 60-iteration
convergence, and its time over the plain loop's 60-iteration call of the same run; the cost of one iteration of either loop (the 60-
and the 10-iteration medians, their difference over 50); k_gl_project_fast against k_gl_project alone (taco_debug_gl_project on the
loop's own number of frame rows) with the bytes each moves over its time; and the convergence call alone.  Its own JSON line,
`--momentum` only."""
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


def trim():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import trim_reference as R
    gl = taco_amd.GriffinLim(hp)
    L = gl.num_samples(T)
    frames = np.random.RandomState(1).randint(T // 4, T + 1, B)
    ns = np.array([gl.num_samples(int(f)) for f in frames], np.int32)
    rs = np.random.RandomState(3)
    x = np.zeros((B, L), np.float32)
    for b, n in enumerate(ns):
        x[b, :n] = 1e-4 * rs.randn(n)
        x[b, :4 * n // 5] = 0.1 * rs.randn(4 * n // 5)
    wav, dn = torch.from_numpy(x).cuda(), torch.from_numpy(ns).cuda()
    kw = dict(top_db=50, frame_length=5120, hop_length=256)
    tail_on = lambda: gl.pcm16(wav, gl.trim(wav, dn, **kw)[:, 1].contiguous())
    arms = {"trim": lambda: gl.trim(wav, dn, **kw), "tail_flag_off": lambda: gl.pcm16(wav, dn), "tail_flag_on": tail_on}
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
    index, db = gl.trim(wav, dn, return_db=True, **kw)
    again = gl.trim(wav, dn, return_db=True, **kw)
    index = index.cpu().numpy()
    t0 = time.perf_counter(); ref = [R.trim(x[b, :n], 50, 5120, 256, "spectral") for b, n in enumerate(ns)]; cpu_s = time.perf_counter() - t0
    ddb = max(float(np.abs(db[b, :len(r[1])].cpu().numpy() - r[1]).max()) for b, r in enumerate(ref))
    out = {"metric": "silence trim (librosa.effects.trim at 5120/256/50 dB) of a C2-shaped batch", "value": med["trim"], "unit": "ms",
           "batch": "B=%d x %d samples, lengths %d..%d (%.1f s of audio at %d Hz)" % (B, L, ns.min(), ns.max(), float(ns.sum()) / hp.sample_rate, hp.sample_rate),
           "windows": "5 windows of 10 calls per arm, alternating", "trim_ms": ms["trim"], "tail_flag_off_ms": ms["tail_flag_off"],
           "tail_flag_on_ms": ms["tail_flag_on"], "tail_flag_on_minus_off_median_ms": med["tail_flag_on"] - med["tail_flag_off"],
           "share_of_a_55_ms_griffin_lim_call": med["trim"] / 55.0, "cpu_restatement_float64_s": cpu_s,
           "indices_equal_to_the_restatement": int(sum(index[b].tolist() == r[0].tolist() for b, r in enumerate(ref))), "rows": B,
           "smallest_margin_db": min(r[2] for r in ref), "max_abs_db_difference": ddb,
           "samples_cut": int((ns - index[:, 1]).sum()), "identical_bits_on_two_calls": bool(torch.equal(again[0].cpu(), torch.from_numpy(index)) and torch.equal(again[1], db))}
    gl.close()
    return out


def split_recording(seconds=180, seed=5):
    """float32 [seconds * sample_rate]: noise floor 1e-5; utterances of 2-9 s made of phrases (0.15-0.3) of 0.4-1.2 s, pauses of 15-30 ms at 1e-4 (shorter than the 1024-sample frame, longer than the 128-sample one)
    and now and then a breath (0.01-0.03) of 0.2-0.4 s between two pauses."""
    sr = hp.sample_rate
    rs = np.random.RandomState(seed)
    n = seconds * sr
    x = 1e-5 * rs.randn(n)
    t = int(0.5 * sr)
    while True:
        end = t + int(rs.uniform(2.0, 9.0) * sr)
        if end >= n - sr:
            break
        while t < end:
            m = min(end - t, int(rs.uniform(0.4, 1.2) * sr))
            x[t:t + m] = rs.uniform(0.15, 0.3) * rs.randn(m); t += m
            m = min(end - t, int(rs.uniform(0.015, 0.03) * sr))
            x[t:t + m] = 1e-4 * rs.randn(m); t += m
            if rs.rand() < 0.4 and t < end:
                m = min(end - t, int(rs.uniform(0.2, 0.4) * sr))
                x[t:t + m] = rs.uniform(0.01, 0.03) * rs.randn(m); t += m
                m = min(end - t, int(rs.uniform(0.015, 0.03) * sr))
                x[t:t + m] = 1e-4 * rs.randn(m); t += m
        t = end + int(rs.uniform(0.5, 1.5) * sr)
    return x.astype(np.float32)


def split():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import split_reference as R
    x = split_recording()
    dev = taco_amd.silence.SilenceDevice(hp)
    gl = dev.gl
    wav = dev.upload(x)
    kw = dict(top_db=40, frame_length=1024, hop_length=256)
    arms = {"split": (lambda: gl.split(wav, None, **kw), 10), "split_on_silence": (lambda: taco_amd.split_on_silence(x, hp, device=dev), 2)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f, _ in arms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(5):
        for k, (f, reps) in arms.items():
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    no_breath, segments = taco_amd.split_on_silence(x, hp, device=dev)
    again = taco_amd.split_on_silence(x, hp, device=dev)
    first = dev.split(wav, 40, 1024, 256)
    t0 = time.perf_counter(); ref = R.split_on_silence(x, hp.sample_rate); cpu_s = time.perf_counter() - t0
    out = {"metric": "split on silence (audio/silence.py:33-76: split at 1024/256/40 dB, remove_breath at 128/32, second split) of one recording",
           "value": med["split_on_silence"], "unit": "ms", "recording": "%.0f s at %d Hz, %d samples" % (len(x) / hp.sample_rate, hp.sample_rate, len(x)),
           "windows": "5 windows per arm, alternating: 10 calls of the split, 2 of split_on_silence", "split_ms": ms["split"],
           "split_on_silence_ms": ms["split_on_silence"], "split_median_ms": med["split"], "x_realtime": len(x) / hp.sample_rate / (med["split_on_silence"] / 1e3),
           "cpu_restatement_float64_s": cpu_s, "intervals_first_split": int(len(first)), "intervals_second_split": int(len(ref["second"])),
           "segments_kept": len(segments), "samples_muted": int(((no_breath == 0) & (x != 0)).sum()),
           "first_split_equals_the_restatement": bool(np.array_equal(first, ref["first"])),
           "segments_equal_to_the_restatement": bool([s[:3] for s in segments] == ref["kept"]),
           "no_breath_equals_the_restatement": bool(np.array_equal(no_breath, ref["no_breath"].astype(np.float32))),
           "restatement_db_margin": ref["db_margin"], "restatement_decision_margin": ref["decision_margin"],
           "identical_bits_on_two_calls": bool(np.array_equal(again[0], no_breath) and [s[:3] for s in again[1]] == [s[:3] for s in segments])}
    dev.close()
    return out


def resample():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import resample_reference as R
    so, sn, seconds = 44100, 24000, 180
    n = so * seconds
    rs_ = np.random.RandomState(9)
    x = R.chirp_rows(n, [n], 9)[0].astype(np.float32)
    q2 = np.stack([np.round(x * 8000), np.round(4000 * rs_.randn(n))], axis=1).astype(np.int16).reshape(1, n, 2)
    rs = taco_amd.Resampler(so, sn)
    mono, pcm = torch.from_numpy(x.reshape(1, n)).cuda(), torch.from_numpy(q2).cuda()
    up = taco_amd.Resampler(16000, sn)                             # the up-sampling shape of the same kernel: 3 phases x 127 taps
    mono16 = mono[:, :16000 * seconds].contiguous()
    arms = {"mono_f32": lambda: rs.resample(mono), "stereo_pcm16": lambda: rs.resample(pcm, channels=2), "up_16000_mono_f32": lambda: up.resample(mono16)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(5):
        for k, f in arms.items():
            e0.record()
            for _ in range(20):
                f()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / 20)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    y, yn = rs.resample(mono)
    again = rs.resample(mono)
    n_out = int(yn[0])
    half = taco_amd.audio.kaiser_window()
    t0 = time.perf_counter(); ref, A = R.resample_bank(x.astype(np.float64), so, sn, half, 512); cpu_s = time.perf_counter() - t0
    ratio = np.abs(y[0, :len(ref)].cpu().numpy().astype(np.float64) - ref) / ((rs.taps + 4) * 2.0 ** -24 * A + 4 * 2.0 ** -149)
    nbytes = {"mono_f32": n * 4 + n_out * 4, "stereo_pcm16": n * 4 + n_out * 4}
    out = {"metric": "resampling 44100 -> 24000 Hz (kaiser_best, %d phases x %d taps) of three minutes of audio" % (rs.phases, rs.taps),
           "value": n_out / (med["mono_f32"] / 1e3), "unit": "output samples per second (mono float32)",
           "recording": "%d s at %d Hz, %d samples -> %d" % (seconds, so, n, n_out), "windows": "5 windows of 20 calls per arm, alternating",
           "mono_f32_ms": ms["mono_f32"], "stereo_pcm16_ms": ms["stereo_pcm16"], "mono_f32_median_ms": med["mono_f32"], "stereo_pcm16_median_ms": med["stereo_pcm16"],
           "stereo_pcm16_output_samples_per_s": n_out / (med["stereo_pcm16"] / 1e3), "x_realtime_mono": seconds / (med["mono_f32"] / 1e3),
           "up_16000_24000_mono_f32_ms": ms["up_16000_mono_f32"], "up_16000_24000_median_ms": med["up_16000_mono_f32"],
           "up_16000_24000_output_samples_per_s": n_out / (med["up_16000_mono_f32"] / 1e3), "up_16000_24000_filter": "%d phases x %d taps" % (up.phases, up.taps),
           "stream_bytes": nbytes, "stream_GBps": {k: nbytes[k] / (med[k] / 1e3) / 1e9 for k in nbytes},
           "GFLOPs_mono": 2.0 * n_out * rs.taps / (med["mono_f32"] / 1e3) / 1e9,
           "cpu_restatement_float64_s": cpu_s, "cpu_restatement_output_samples_per_s": n_out / cpu_s,
           "largest_error_over_the_derived_bound": float(ratio.max()), "identical_bits_on_two_calls": bool(torch.equal(again[0], y) and torch.equal(again[1], yn))}
    rs.close(); up.close()
    return out


def vocoders():
    gl, tf = taco_amd.GriffinLim(hp), taco_amd.GriffinLim(hp, flavor="tensorflow")
    gl.set_inv_mel_basis()
    M = int(hp.num_mels)
    rs = np.random.RandomState(0)
    spec = torch.from_numpy(rs.rand(B, T, F).astype(np.float32)).cuda()
    mel = torch.from_numpy(rs.rand(B, T, M).astype(np.float32)).cuda()
    arms = {"inv_spectrogram": (lambda: gl.inv_spectrogram(spec), 4), "inv_spectrogram_0_iters": (lambda: gl.inv_spectrogram(spec, iters=0), 20),
            "inv_spectrogram_tensorflow": (lambda: tf.inv_spectrogram_tensorflow(spec)[0], 4),
            "inv_melspectrogram": (lambda: gl.inv_melspectrogram(mel)[0], 4), "k_gl_mel_magnitude": (lambda: gl.mel_to_linear(mel), 50)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f, _ in arms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(5):
        for k, (f, reps) in arms.items():
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    a, b = tf.inv_spectrogram_tensorflow(spec), tf.inv_spectrogram_tensorflow(spec)
    w = gl.inv_melspectrogram(mel)[0]
    iteration = (med["inv_spectrogram"] - med["inv_spectrogram_0_iters"]) / hp.griffin_lim_iters
    nbytes = B * T * (M + F) * 4                                 # mel read, magnitudes written (the basis stays in cache)
    out = {"metric": "the three vocoders at the C2 output shape (Griffin-Lim, %d iterations)" % hp.griffin_lim_iters, "value": med["inv_spectrogram_tensorflow"],
           "unit": "ms (inv_spectrogram_tensorflow)", "batch": "B=%d x T=%d frames x %d bins (%d mels)" % (B, T, F, M),
           "windows": "5 windows per arm, alternating: 4 calls of a vocoder, 20 of the 0-iteration call, 50 of k_gl_mel_magnitude",
           "inv_spectrogram_ms": ms["inv_spectrogram"], "inv_spectrogram_tensorflow_ms": ms["inv_spectrogram_tensorflow"],
           "inv_melspectrogram_ms": ms["inv_melspectrogram"], "inv_spectrogram_0_iters_ms": ms["inv_spectrogram_0_iters"],
           "k_gl_mel_magnitude_ms": ms["k_gl_mel_magnitude"], "median_ms": med,
           "tensorflow_over_existing": med["inv_spectrogram_tensorflow"] / med["inv_spectrogram"],
           "mel_over_existing": med["inv_melspectrogram"] / med["inv_spectrogram"],
           "one_iteration_ms": iteration, "k_gl_mel_magnitude_over_one_iteration": med["k_gl_mel_magnitude"] / iteration,
           "k_gl_mel_magnitude_bytes": nbytes, "k_gl_mel_magnitude_GBps": nbytes / (med["k_gl_mel_magnitude"] / 1e3) / 1e9,
           "k_gl_mel_magnitude_GFLOPs": 2.0 * B * T * M * F / (med["k_gl_mel_magnitude"] / 1e3) / 1e9,
           "tensorflow_identical_bits_on_two_calls": bool(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])),
           "finite": bool(torch.isfinite(a[0]).all() and torch.isfinite(w).all())}
    gl.close(); tf.close()
    return out


def pydub_recording(seconds=180, sr=44100, seed=7):
    """int16 [seconds * sr, 2]: a floor of +-3; utterances of 1-6 s made of phrases (uniform in +-3000..9000) of 0.3-1.0 s with pauses of
    20-80 ms at +-20 between them, separated by 0.3-1.2 s of floor."""
    rs = np.random.RandomState(seed)
    n = seconds * sr
    x = rs.randint(-3, 4, size=(n, 2))
    t = int(0.4 * sr)
    while True:
        end = t + int(rs.uniform(1.0, 6.0) * sr)
        if end >= n - sr:
            break
        while t < end:
            m = min(end - t, int(rs.uniform(0.3, 1.0) * sr)); a = int(rs.uniform(3000, 9000))
            x[t:t + m] = rs.randint(-a, a + 1, size=(m, 2)); t += m
            m = min(end - t, int(rs.uniform(0.02, 0.08) * sr))
            x[t:t + m] = rs.randint(-20, 21, size=(m, 2)); t += m
        t = end + int(rs.uniform(0.3, 1.2) * sr)
    return x.astype(np.int16)


def pydub():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pydub_reference as R
    from taco_amd import silence
    sr, seconds = 44100, 180
    x = pydub_recording(seconds, sr)
    dev = silence.PcmDevice(hp)
    gl = dev.gl
    pcm = dev.upload(x)["pcm"]
    import ctypes as C
    energy = torch.empty((1, R.len_ms(len(x), sr)), dtype=torch.int64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    energy_pass = lambda: taco_amd._lib.check(gl._lib.taco_debug_pcm_energy(C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(pcm), None, 1, len(x), 2, sr, ptr(energy)))
    arms = {"nonsilent": (lambda: gl.nonsilent(pcm, None, sr, 100, -40), 20), "energy_pass": (energy_pass, 20), "device_copy": (lambda: pcm.clone(), 20),
            "split_on_silence_pydub": (lambda: silence.split_on_silence_pydub(x, sr, device=dev), 2), "amplify": (lambda: silence.amplify(x, sr, device=dev), 2)}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for f, _ in arms.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(5):
        for k, (f, reps) in arms.items():
            e0.record()
            for _ in range(reps):
                f()
            e1.record(); torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / reps)
    med = {k: float(np.median(v)) for k, v in ms.items()}
    a, b = gl.nonsilent(pcm, None, sr, 100, -40), gl.nonsilent(pcm, None, sr, 100, -40)
    ranges = a[0][0, :int(a[1][0])].cpu().numpy().tolist()
    segments = silence.split_on_silence_pydub(x, sr, device=dev)
    loud = silence.amplify(x, sr, device=dev)
    t0 = time.perf_counter(); ref_ranges, M = R.detect_nonsilent(x, sr, 100, -40); fast_s = time.perf_counter() - t0
    ref_segments = R.split_on_silence_with_pydub(x, sr)
    t0 = time.perf_counter(); ref_loud = R.amplify(x, sr); fast_amplify_s = time.perf_counter() - t0
    literal_s = None
    if R.HAVE_AUDIOOP:
        head = x[:10 * sr]
        t0 = time.perf_counter(); lit = R.detect_nonsilent_literal(R.Segment.of(head, sr), 100, -40); literal_s = time.perf_counter() - t0
        assert lit == R.detect_nonsilent(head, sr, 100, -40)[0]
    nbytes = x.nbytes
    out = {"metric": "pydub method (audio/silence.py:81-117: detect_nonsilent at 100 ms / -40 dBFS, merge, keep_silence) of one recording",
           "value": med["split_on_silence_pydub"], "unit": "ms", "recording": "%d s at %d Hz, stereo PCM16, %d frames, %d ms" % (seconds, sr, len(x), M),
           "windows": "5 windows per arm, alternating: 20 calls of nonsilent, of the energy pass and of the copy, 2 of split_on_silence_pydub and of amplify",
           "nonsilent_ms": ms["nonsilent"], "split_on_silence_pydub_ms": ms["split_on_silence_pydub"], "amplify_ms": ms["amplify"],
           "device_copy_ms": ms["device_copy"], "median_ms": med, "x_realtime": seconds / (med["split_on_silence_pydub"] / 1e3),
           "energy_pass_ms": ms["energy_pass"], "recording_bytes": nbytes, "energy_pass_read_GBps": nbytes / (med["energy_pass"] / 1e3) / 1e9,
           "device_copy_read_GBps": nbytes / (med["device_copy"] / 1e3) / 1e9, "device_copy_read_plus_write_GBps": 2 * nbytes / (med["device_copy"] / 1e3) / 1e9,
           "cpu_restatement_fast_form_s": fast_s, "cpu_restatement_fast_form_amplify_s": fast_amplify_s,
           "cpu_restatement_literal_audioop_s": literal_s, "cpu_restatement_literal_audioop_label": "literal, 10 s",
           "nonsilent_ranges": len(ranges), "segments": len(segments), "amplified_frames": int(len(loud)),
           "ranges_equal_to_the_restatement": bool(ranges == ref_ranges),
           "segments_equal_to_the_restatement": bool([g[:3] for g in segments] == [r[:3] for r in ref_segments] and all(np.array_equal(g[3], r[3]) for g, r in zip(segments, ref_segments))),
           "amplify_equals_the_restatement": bool(np.array_equal(loud, ref_loud)),
           "identical_bits_on_two_calls": bool(all(torch.equal(u, v) for u, v in zip(a, b)))}
    dev.close()
    return out


def multitone(rows=B, n=153300, seed=11):
    """float32 [rows, n]: per row six tones of seeded frequency (80 Hz - 9 kHz), amplitude, vibrato and slow tremolo"""
    rs = np.random.RandomState(seed)
    t = np.arange(n) / float(hp.sample_rate)
    x = np.zeros((rows, n))
    for b in range(rows):
        for _ in range(6):
            f0, a = np.exp(rs.uniform(np.log(80.0), np.log(9000.0))), rs.uniform(0.005, 0.03)
            vib, trem = rs.uniform(0.0, 0.01) * f0 / 5.0, rs.uniform(0.2, 3.0)
            x[b] += a * (0.6 + 0.4 * np.sin(2 * np.pi * trem * t + rs.uniform(0, 6.28))) * np.sin(2 * np.pi * f0 * t + vib * np.sin(2 * np.pi * 5.0 * t) + rs.uniform(0, 6.28))
    return x.astype(np.float32)


def momentum():
    import ctypes as C
    ITERS, MOMENTA, WINDOWS, CALLS = (10, 20, 30, 60), (0.0, 0.99), 5, 4
    sp, gl = taco_amd.Spectrogram(hp), taco_amd.GriffinLim(hp)
    L = gl.num_samples(T)
    lin = sp.targets(torch.from_numpy(multitone(B, L)).cuda(), mel=False)[0]                      # normalised 20 log10 |stft(p)| - ref_level_db
    assert tuple(lin.shape) == (B, T, F)
    # the vocoder raises the amplitude it decodes to `power`: encode |stft(p)|^(1/power), so that its magnitudes are |stft(p)| itself
    db = lin * -hp.min_level_db + hp.min_level_db + hp.ref_level_db
    spec = ((db / hp.power - hp.ref_level_db - hp.min_level_db) / -hp.min_level_db).clamp_(0.0, 1.0).contiguous()
    sp.close()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(f, calls):
        e0.record()
        for _ in range(calls):
            out = f()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls, out

    cells = [(it, m) for it in ITERS for m in MOMENTA]
    for it, m in cells:                                       # warm: both workspace sizes, every launch shape
        gl.inv_spectrogram(spec, iters=it, momentum=m)
    torch.cuda.synchronize()
    ms, sc = {c: [] for c in cells}, {}
    for _ in range(WINDOWS):
        for it, m in cells:                                   # the two settings alternate at every iteration count
            t, wav = window(lambda: gl.inv_spectrogram(spec, iters=it, momentum=m), CALLS)
            ms[(it, m)].append(t)
            sc[(it, m)] = gl.convergence(spec, wav).cpu().numpy()
    wav = gl.inv_spectrogram(spec, iters=60, momentum=0.99)
    same = bool(torch.equal(wav, gl.inv_spectrogram(spec, iters=60, momentum=0.99)))
    conv_ms = [window(lambda: gl.convergence(spec, wav), 20)[0] for _ in range(WINDOWS)]
    med = {c: float(np.median(v)) for c, v in ms.items()}
    mean = {c: float(v.mean()) for c, v in sc.items()}
    reach = [it for it in ITERS if mean[(it, 0.99)] <= mean[(60, 0.0)]]
    per_it = {m: (med[(60, m)] - med[(10, m)]) / 50.0 for m in MOMENTA}
    # the projection kernels alone, on the loop's own frame rows
    n_fft, hop = (F - 1) * 2, int(hp.frame_shift_ms / 1000 * hp.sample_rate)
    R = B * (T + -(-n_fft // hop))
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    est, prev = (torch.randn((R, 2 * F), device="cuda", generator=g) for _ in range(2))
    S, X = torch.rand((R, F), device="cuda", generator=g), torch.empty((R, 2 * F), device="cuda")
    p = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    proj = lambda pv: taco_amd._lib.check(gl._lib.taco_debug_gl_project(gl._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), p(est), p(pv), p(S), p(X),
                                                                        C.c_float(0.99 / 1.99), R))
    kern = {"k_gl_project": lambda: proj(None), "k_gl_project_fast": lambda: proj(prev)}
    for f in kern.values():
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    kms = {k: [] for k in kern}
    for _ in range(WINDOWS):
        for k, f in kern.items():
            kms[k].append(window(f, 50)[0])
    kmed = {k: float(np.median(v)) for k, v in kms.items()}
    kbytes = {"k_gl_project": R * F * 20, "k_gl_project_fast": R * F * 28}
    key = lambda c: "%d_iters_momentum_%g" % c
    out = {"metric": "Fast Griffin-Lim at the C2 output shape: time of the smallest iteration count at which momentum 0.99 reaches the plain loop's 60-iteration spectral convergence, over the plain loop's 60-iteration call",
           "value": med[(reach[0], 0.99)] / med[(60, 0.0)] if reach else None, "unit": "x the plain loop's 60-iteration call",
           "batch": "B=%d x T=%d frames x %d bins, the STFT magnitudes of seeded six-tone signals (%d samples each)" % (B, T, F, L),
           "windows": "%d windows of %d calls per cell, momentum 0 and 0.99 alternating; 50 calls per window for a kernel alone, 20 for the convergence call" % (WINDOWS, CALLS),
           "ms": {key(c): v for c, v in ms.items()}, "median_ms": {key(c): v for c, v in med.items()},
           "convergence_mean": {key(c): v for c, v in mean.items()}, "convergence_worst": {key(c): float(v.max()) for c, v in sc.items()},
           "plain_60_iterations_ms": med[(60, 0.0)], "plain_60_iterations_convergence_mean": mean[(60, 0.0)],
           "smallest_iterations_at_or_below_plain_60": reach[0] if reach else None,
           "ms_at_that_count": med[(reach[0], 0.99)] if reach else None,
           "one_iteration_ms": {"momentum_0": per_it[0.0], "momentum_0.99": per_it[0.99]}, "one_iteration_fast_over_plain": per_it[0.99] / per_it[0.0],
           "same_count_fast_over_plain": {str(it): med[(it, 0.99)] / med[(it, 0.0)] for it in ITERS},
           "kernel_ms": kms, "kernel_median_ms": kmed, "kernel_bytes": kbytes, "kernel_GBps": {k: kbytes[k] / (kmed[k] / 1e3) / 1e9 for k in kern},
           "k_gl_project_fast_over_k_gl_project": kmed["k_gl_project_fast"] / kmed["k_gl_project"],
           "convergence_call_ms": conv_ms, "identical_bits_on_two_calls": same, "finite": bool(torch.isfinite(wav).all())}
    gl.close()
    return out


if "--momentum" in sys.argv:
    print(json.dumps(momentum()))
    sys.exit(0)
if "--pydub" in sys.argv:
    print(json.dumps(pydub()))
    sys.exit(0)
if "--vocoders" in sys.argv:
    print(json.dumps(vocoders()))
    sys.exit(0)
if "--resample" in sys.argv:
    print(json.dumps(resample()))
    sys.exit(0)
if "--split" in sys.argv:
    print(json.dumps(split()))
    sys.exit(0)
if "--trim" in sys.argv:
    print(json.dumps(trim()))
    sys.exit(0)
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
