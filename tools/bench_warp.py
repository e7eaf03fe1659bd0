#!/usr/bin/env python
"""Times rate, duration and pitch control on the spectrogram (taco_spec_warp_map / taco_spec_warp, csrc/taco_warp.h) at the shape it is
for: the C2 output, 32 rows x 512 frames x 1025 bins, at rate 0.8 with a per-token stretch and a pitch:

  * the map alone (k_warp_map), the warp alone (k_spec_warp: with the frequency scale, its gather from the row staged in LDS and -- through
    taco_debug_spec_warp_direct -- straight from the cache; and without the scale), and both;
  * a device copy of the same output bytes as yardstick (the least any pass that writes the output costs);
  * Synthesizer.synthesize_audio at C2 with and without the keywords.

The kernels are timed as 20 calls back to back in one captured graph (the launch path from Python would otherwise be what the map's
time measures), the variants alternating window by window, device events around each replay; medians.  The figure to read the warp
against is bytes: it writes the output once and reads every source frame it uses at least once (its second reader is served by the
caches), so bytes = output bytes + used input bytes, next to the copy's 2 x output bytes.

    python tools/bench_warp.py [--windows 5] [--calls 20] [--out FILE]

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

B, T_IN, N_STEPS, W = 32, 128, 128, 1025
RATE, PITCH = 0.8, 2.0


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
        sys.exit("bench_warp.py needs a GPU: nothing here is timed on the host in its place")
    hp = taco_amd.hparams.copy(max_iters=N_STEPS)
    r = hp.reduction_factor
    T = N_STEPS * r
    med = lambda v: float(np.median(v))
    rs = np.random.RandomState(1)

    # a monotone attention with some noise, stretches a listener would ask for, the trim's frame counts near the end
    al = rs.rand(B, T_IN, N_STEPS).astype(np.float32) * 0.3
    for b in range(B):
        al[b, np.minimum((np.arange(N_STEPS) * (0.7 + 0.3 * rs.rand())).astype(int), T_IN - 1), np.arange(N_STEPS)] += 1.0
    tok_host = rs.choice([0.75, 1.0, 1.0, 1.25, 1.5], size=(B, T_IN)).astype(np.float32)
    row_host = np.full(B, 1.0 / RATE, np.float32)
    frames_host = rs.randint(T - 40, T + 1, size=B).astype(np.int32)
    T_out = prosody.out_frames_bound(T, row_host, tok_host)
    up = lambda x: torch.as_tensor(x).cuda()
    spec = torch.rand((B, T, W), device="cuda")
    d_al, d_tok, d_row, d_frames = up(al), up(tok_host), up(row_host), up(frames_host)
    d_scale = up(np.full(B, prosody.semitones_to_scale(PITCH), np.float32))

    def do_map():
        return prosody.warp_map(d_frames, T, r, d_al, d_row, d_tok, out_cap=T_out)

    m = do_map()
    out, of = prosody.warp(spec, d_frames, m, d_scale)
    torch.cuda.synchronize()
    out_frames = of.cpu().numpy()
    copy_dst = torch.empty_like(out)
    from taco_amd import _device, _lib
    direct_out = torch.empty_like(out)

    def warp_direct():
        _device.call(spec.device, _lib.load_library().taco_debug_spec_warp_direct, _device.STREAM, spec, d_frames, m.src, m.frac, m.out_frames,
                     d_scale, B, T, W, T_out, direct_out)

    warp_direct()
    torch.cuda.synchronize()
    assert torch.equal(direct_out.view(torch.int32), out.view(torch.int32))      # the two forms of the frequency gather: the same bits
    fns = {"map": do_map, "warp": lambda: prosody.warp(spec, d_frames, m, d_scale), "warp_direct": warp_direct,
           "warp_no_pitch": lambda: prosody.warp(spec, d_frames, m),
           "both": lambda: prosody.warp(spec, d_frames, do_map(), d_scale), "copy": lambda: copy_dst.copy_(out)}
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

    out_bytes = int(out.numel()) * 4
    used_in_bytes = int(np.clip(frames_host, 1, T).sum()) * W * 4
    written_rows = int(out_frames.sum())
    warp_bytes = out_bytes + used_in_bytes
    gbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e9

    # synthesize_audio at C2 with and without the keywords (random weights; the trim is off so that every row keeps its 512 frames)
    s = taco_amd.Synthesizer()
    s.hparams, s.num_speakers = hp, 1
    s.model = taco_amd.create_model(hp)
    s.model.load_weights(taco_amd.weights.random_weights(hp, 1, seed=1))
    s.model.initialize(None, None, 1, None)
    ids = rs.randint(2, 80, size=(B, T_IN)).astype(np.int32)
    ids[:, -1] = 1
    stretch = [list(map(float, row_)) for row_ in tok_host]
    kw = dict(tokens=ids, attention_trim=False, seed=1)
    plain = lambda: s.synthesize_audio(**kw)
    unit = lambda: s.synthesize_audio(rate=1.0, **kw)
    full = lambda: s.synthesize_audio(rate=RATE, token_stretch=stretch, pitch=PITCH, **kw)
    import time
    synth = {"plain": [], "rate_1": [], "rate_stretch_pitch": []}
    for fn in (plain, unit, full):
        fn()
    for _ in range(3):
        for name, fn in zip(synth, (plain, unit, full)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()                                                              # ends in the download of the audio: a synchronise
            synth[name].append((time.perf_counter() - t0) * 1e3)
    warped = [int(v) for v in s.warped_frames]
    s.close()

    line = {"metric": "taco_spec_warp_map + taco_spec_warp at the C2 output (rate %.2f, a per-token stretch, pitch %+g semitones) next to a device "
                      "copy of the same output bytes; synthesize_audio with and without the keywords" % (RATE, PITCH),
            "shape": {"rows": B, "frames": T, "bins": W, "T_in": T_IN, "n_steps": N_STEPS, "reduction_factor": r, "T_out": T_out,
                      "out_frames_mean": float(out_frames.mean()), "out_frames_max": int(out_frames.max()), "written_rows": written_rows},
            "map_ms": med(times["map"]), "map_ms_windows": times["map"],
            "warp_ms": med(times["warp"]), "warp_ms_windows": times["warp"],
            "warp_direct_ms": med(times["warp_direct"]), "warp_direct_ms_windows": times["warp_direct"],
            "warp_no_pitch_ms": med(times["warp_no_pitch"]), "warp_no_pitch_ms_windows": times["warp_no_pitch"],
            "both_ms": med(times["both"]), "both_ms_windows": times["both"],
            "copy_ms": med(times["copy"]), "copy_ms_windows": times["copy"],
            "output_bytes": out_bytes, "used_input_bytes": used_in_bytes, "warp_bytes": warp_bytes, "copy_bytes": 2 * out_bytes,
            "warp_GBps": gbs(warp_bytes, med(times["warp"])), "warp_no_pitch_GBps": gbs(warp_bytes, med(times["warp_no_pitch"])),
            "copy_GBps": gbs(2 * out_bytes, med(times["copy"])), "warp_over_copy_time": med(times["warp"]) / med(times["copy"]),
            "warp_no_pitch_over_copy_time": med(times["warp_no_pitch"]) / med(times["copy"]),
            "synthesize_audio_ms": {k: med(v) for k, v in synth.items()}, "synthesize_audio_ms_runs": synth, "synthesize_audio_warped_frames": warped[:4],
            "windows": "%d windows of one replay of %d captured calls per variant after two warm-up calls, the variants alternating window by "
                       "window, device events around each replay; medians.  synthesize_audio: host clock around the call (it ends in the audio's "
                       "download), 3 runs alternating, medians" % (a.windows, a.calls),
            "device": torch.cuda.get_device_name(0)}
    txt = json.dumps(line)
    print(txt)
    if a.out:
        with open(a.out, "w") as f_:
            f_.write(txt + "\n")


if __name__ == "__main__":
    main()
