#!/usr/bin/env python
"""Times the spectral envelope and the pitch / formant shift (taco_spec_envelope / taco_spec_warp_formant, csrc/taco_envelope.h) at the
shape they are for: the C2 output, 32 rows x 512 frames x 1025 bins, Q = 49 cepstral coefficients:

  * the envelope alone (k_spec_envelope);
  * the shift (k_spec_warp_formant) at rate 0.8 with the pitch up 2 semitones and the formants kept;
  * beside them the plain warp (k_spec_warp) with the same pitch scale on the same map, and a device copy of the same output bytes;
  * Synthesizer.synthesize_audio at C2 with and without formant=0.

The kernels are timed as 20 calls back to back in one captured graph, the variants alternating window by window, device events around
each replay; medians.  The two figures to read the new kernels against are computed, not measured: the matrix work, 2 * 2 * frames * W * Q
flop at the fp32 matrix rate (157.3 Tflop/s), and the bytes -- the output written once, every used source frame read once -- at 5 TB/s; the two
tables (2 * QP * WP * 4 bytes) are read once per workgroup of 16 frames through L2, and that traffic is reported beside them.  No time is a pass condition.

    python tools/bench_formant.py [--windows 5] [--calls 20] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

B, T_IN, N_STEPS, W, Q = 32, 128, 128, 1025, 49
RATE, PITCH = 0.8, 2.0
FP32_MATRIX_FLOPS, HBM_BYTES_PER_S = 157.3e12, 5.0e12


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20, help="calls per captured graph")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import taco_amd
    from taco_amd import prosody
    if not torch.cuda.is_available():
        sys.exit("bench_formant.py needs a GPU: nothing here is timed on the host in its place")
    hp = taco_amd.hparams.copy(max_iters=N_STEPS)
    r = hp.reduction_factor
    T = N_STEPS * r
    med = lambda v: float(np.median(v))
    rs = np.random.RandomState(1)
    up = lambda x: torch.as_tensor(x).cuda()
    row_host = np.full(B, 1.0 / RATE, np.float32)
    frames_host = rs.randint(T - 40, T + 1, size=B).astype(np.int32)
    T_out = prosody.out_frames_bound(T, row_host)
    spec = torch.rand((B, T, W), device="cuda")
    d_row, d_frames = up(row_host), up(frames_host)
    d_pitch = up(np.full(B, prosody.semitones_to_scale(PITCH), np.float32))
    d_formant = up(np.full(B, prosody.semitones_to_scale(0.0), np.float32))
    m = prosody.warp_map(d_frames, T, r, None, d_row, out_cap=T_out)
    out, of = prosody.warp_formant(spec, d_frames, m, d_pitch, d_formant, order=Q - 1)     # the handle's first call: outside capture
    prosody.envelope(spec, d_frames, order=Q - 1)
    torch.cuda.synchronize()
    out_frames = of.cpu().numpy()
    copy_dst = torch.empty_like(out)
    fns = {"envelope": lambda: prosody.envelope(spec, d_frames, order=Q - 1),
           "warp_formant": lambda: prosody.warp_formant(spec, d_frames, m, d_pitch, d_formant, order=Q - 1),
           "warp": lambda: prosody.warp(spec, d_frames, m, d_pitch), "copy": lambda: copy_dst.copy_(out)}
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in fns.items():
        fn(); fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(a.calls):
                fn()
        g.replay()
        graphs[name] = g
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(a.windows):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.calls)

    used = int(np.clip(frames_host, 1, T).sum())
    written = int(out_frames.sum())
    wp, qp = -(-W // 16) * 16, -(-Q // 16) * 16
    table_bytes = 2 * qp * wp * 4

    def floors(n_frames, io_bytes):
        flop = 4 * n_frames * W * Q
        return {"frames": n_frames, "flop": flop, "matrix_floor_us": flop / FP32_MATRIX_FLOPS * 1e6, "bytes": io_bytes,
                "bytes_floor_us": io_bytes / HBM_BYTES_PER_S * 1e6, "table_bytes_through_L2": -(-n_frames // 16) * table_bytes}

    env_floor = floors(used, (used + B * T) * W * 4)                       # the used frames read, every frame of the output written
    wf_floor = floors(written, used * W * 4 + int(out.numel()) * 4)

    # synthesize_audio at C2 with and without formant=0 (random weights; the trim is off so that every row keeps its 512 frames)
    s = taco_amd.Synthesizer()
    s.hparams, s.num_speakers = hp, 1
    s.model = taco_amd.create_model(hp)
    s.model.load_weights(taco_amd.weights.random_weights(hp, 1, seed=1))
    s.model.initialize(None, None, 1, None)
    ids = rs.randint(2, 80, size=(B, T_IN)).astype(np.int32)
    ids[:, -1] = 1
    kw = dict(tokens=ids, attention_trim=False, seed=1)
    variants = {"plain": lambda: s.synthesize_audio(**kw), "pitch_2": lambda: s.synthesize_audio(pitch=PITCH, **kw),
                "formant_0": lambda: s.synthesize_audio(formant=0.0, **kw), "pitch_2_formant_0": lambda: s.synthesize_audio(pitch=PITCH, formant=0.0, **kw)}
    synth = {k: [] for k in variants}
    for fn in variants.values():
        fn()
    for _ in range(3):
        for name, fn in variants.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                              # ends in the download of the audio: a synchronise
            synth[name].append((time.perf_counter() - t0) * 1e3)
    s.close()

    line = {"metric": "taco_spec_envelope and taco_spec_warp_formant (rate %.2f, pitch %+g semitones, formants kept, Q = %d) at the C2 output next "
                      "to taco_spec_warp with the same pitch scale and a device copy of the same output bytes; synthesize_audio with and without "
                      "formant=0" % (RATE, PITCH, Q),
            "shape": {"rows": B, "frames": T, "bins": W, "Q": Q, "T_out": T_out, "used_frames": used, "written_rows": written},
            "envelope_ms": med(times["envelope"]), "envelope_ms_windows": times["envelope"],
            "warp_formant_ms": med(times["warp_formant"]), "warp_formant_ms_windows": times["warp_formant"],
            "warp_ms": med(times["warp"]), "warp_ms_windows": times["warp"],
            "copy_ms": med(times["copy"]), "copy_ms_windows": times["copy"],
            "envelope_floors": env_floor, "warp_formant_floors": wf_floor, "table_bytes": table_bytes,
            "warp_formant_over_warp_time": med(times["warp_formant"]) / med(times["warp"]),
            "synthesize_audio_ms": {k: med(v) for k, v in synth.items()}, "synthesize_audio_ms_runs": synth,
            "windows": "%d windows of one replay of %d captured calls per variant after two warm-up calls, the variants alternating window by "
                       "window, device events around each replay; medians.  synthesize_audio: host clock around the call (it ends in the audio's "
                       "download), 3 runs alternating, medians.  The floors are computed: flop at %.1f Tflop/s, bytes at %.1f TB/s"
                       % (a.windows, a.calls, FP32_MATRIX_FLOPS / 1e12, HBM_BYTES_PER_S / 1e12),
            "device": torch.cuda.get_device_name(0)}
    txt = json.dumps(line)
    print(txt)
    if a.out:
        with open(a.out, "w") as f_:
            f_.write(txt + "\n")


if __name__ == "__main__":
    main()
