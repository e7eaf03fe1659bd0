#!/usr/bin/env python
"""Times dynamic time warping on the device (taco_dtw / taco_dtw_path, csrc/taco_dtw.h) at the shapes it is for:

  * c4_mel:      32 pairs, 512 x 512 frames, D = 80, mean-absolute cost -- a C4 shard's mel outputs against their targets (Tacotron.mel_dtw);
  * c4_cepstra:  the same frames at 13 cepstra, Euclidean cost -- mel_cepstral_distortion;
  * c5_mel:      8 pairs, 4000 x 4000 frames, D = 80 -- one C5-sized pair set;

each with and without the direction map, taco_dtw_path alone on the map of the run before, and a device copy of both inputs as a
yardstick (the least any pass over the data costs).  On the host, one thread: the float64 restatement (tests/dtw_reference.py) on ONE
pair of c4_mel, multiplied by the pair count and labelled as extrapolated.  The figure to read a time against is the dependent chain:
a strip of columns takes n + (its width) - 1 anti-diagonal steps, one after the other, so `us_per_step` = time / steps of one pair
(all pairs run side by side, one workgroup each).

    python tools/bench_dtw.py [--windows 5] [--calls 10] [--out FILE]

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

SHAPES = (("c4_mel", 32, 512, 512, 80, 0), ("c4_cepstra", 32, 512, 512, 13, 1), ("c5_mel", 8, 4000, 4000, 80, 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10, help="calls per timed window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    from taco_amd import _lib
    import dtw_reference as R
    if not torch.cuda.is_available():
        sys.exit("bench_dtw.py needs a GPU: nothing here is timed on the host in its place")
    lib = _lib.load_library()
    info = (C.c_int * 6)()
    _lib.check(lib.taco_debug_dtw_info(info, 6))
    strip = int(info[0])
    P = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    med = lambda v: float(np.median(v))

    def timed(fn, calls):
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(a.windows):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) / calls)
        return out

    shapes = {}
    host = None
    for name, B, Ta, Tb, D, kind in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(1)
        A = torch.rand((B, Ta, D), device="cuda", generator=g)
        Bm = torch.rand((B, Tb, D), device="cuda", generator=g)
        dist, total = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
        dr = torch.empty((B, Ta, Tb), dtype=torch.uint8, device="cuda")
        path = torch.empty((B, Ta + Tb - 1, 2), dtype=torch.int32, device="cuda")
        plen = torch.empty(B, dtype=torch.int32, device="cuda")
        nws = int(lib.taco_dtw_workspace_bytes(B, Ta, Tb, D))
        ws = torch.empty(max(nws, 1), dtype=torch.uint8, device="cuda")
        A2, B2 = torch.empty_like(A), torch.empty_like(Bm)
        st = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def dtw(with_dir):
            _lib.check(lib.taco_dtw(st(), P(A), None, P(Bm), None, B, Ta, Tb, D, kind, P(dist), P(total), P(dr) if with_dir else None,
                                    P(ws) if nws else None, nws))

        def walk():
            _lib.check(lib.taco_dtw_path(st(), P(dr), None, None, B, Ta, Tb, P(path), P(plen)))

        def copy():
            A2.copy_(A)
            B2.copy_(Bm)

        calls = a.calls if Ta * Tb <= 1 << 20 else max(1, a.calls // 5)
        t_plain, t_dir = timed(lambda: dtw(False), calls), timed(lambda: dtw(True), calls)
        without = total.clone()
        dtw(True)
        torch.cuda.synchronize()
        assert torch.equal(without.view(torch.int32), total.view(torch.int32)) and bool(torch.isfinite(total).all())
        t_walk, t_copy = timed(walk, calls), timed(copy, calls)
        n_strips = -(-Tb // strip)
        steps = sum(Ta + min(strip, Tb - k * strip) - 1 for k in range(n_strips))
        shapes[name] = {"pairs": B, "Ta": Ta, "Tb": Tb, "D": D, "cost_kind": kind, "strips": n_strips, "steps_per_pair": steps,
                        "dtw_ms": med(t_plain), "dtw_ms_windows": t_plain, "us_per_step": med(t_plain) * 1e3 / steps,
                        "dtw_with_dir_ms": med(t_dir), "dtw_with_dir_ms_windows": t_dir, "us_per_step_with_dir": med(t_dir) * 1e3 / steps,
                        "path_ms": med(t_walk), "path_ms_windows": t_walk, "path_len_mean": float(plen.float().mean()),
                        "us_per_path_entry": med(t_walk) * 1e3 / float(plen.max()),
                        "copy_inputs_ms": med(t_copy), "copy_inputs_ms_windows": t_copy, "input_bytes": int(A.numel() + Bm.numel()) * 4,
                        "calls_per_window": calls, "mean_dist": float((total / (Ta + Tb)).mean())}
        if name == "c4_mel":
            a0, b0 = A[0].cpu().numpy(), Bm[0].cpu().numpy()
            t0 = time.perf_counter()
            ref_total = R.dtw(a0, b0, kind)[0]
            one = time.perf_counter() - t0
            gamma = (Ta + Tb + D + 4) * 2.0 ** -24
            assert abs(float(total[0]) - ref_total) <= gamma / (1 - gamma) * ref_total
            host = {"float64_numpy_one_pair_ms": one * 1e3, "float64_numpy_all_pairs_ms_extrapolated": one * 1e3 * B,
                    "note": "tests/dtw_reference.py dtw (anti-diagonals in NumPy, one thread) on pair 0 of c4_mel, times %d pairs: extrapolated, not run" % B}
        del A, Bm, dr, path, A2, B2
        torch.cuda.empty_cache()

    line = {"metric": "taco_dtw (k_dtw: one workgroup per pair, anti-diagonal steps) with and without the direction map, taco_dtw_path, and a device copy of the inputs",
            "strip_columns": strip, "rows_staged": int(info[1]), "shapes": shapes, "host": host,
            "windows": "%d windows of `calls_per_window` calls per kernel after 2 warm-up calls, device events around each window; medians"
                       % a.windows,
            "device": torch.cuda.get_device_name(0)}
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
