#!/usr/bin/env python
"""Feeding the training step at the C4-shard shape (32 rows, targets of 380-508 frames, 100 tokens, r = 4; seeded):

  (a) the host path: np.load of 32 `.npz` files + feeder.collate + upload of the batch;
  (b) DeviceCorpus.collate, kind "targets": one taco_collate launch out of a corpus of --corpus examples (larger than the 256 MiB
      Infinity Cache, so the reads come from HBM), eager per batch and as 16 launches replayed from one graph (device time);
  (c) the same with kind "waveform": taco_collate of the samples + Spectrogram.targets;
  (d) a torch device-to-device copy of as many bytes as (b) writes, source rotating over more than the cache: the yardstick for
      (b)'s bytes over time (the copy moves at least as many bytes: it reads what it writes, (b) reads only the rows' own frames);
  (e) training steps per second: Trainer.train_step fed by (a) and by (b) over the same 20 batches, next to the step alone on a
      fixed batch.

Warm-up, then --windows timed windows per arm; medians with [min, max].  Device work is timed with events around a window that ends
in a synchronise, host work with perf_counter.  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse, json, os, shutil, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(xs):
    xs = sorted(float(x) for x in xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1], "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=100)
    ap.add_argument("--frames", type=int, nargs=2, default=[380, 508])
    ap.add_argument("--corpus", type=int, default=256, help="examples held on the device (32 distinct ones, repeated)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--launches", type=int, default=400, help="eager collates per timed window")
    ap.add_argument("--replays", type=int, default=40, help="replays of the 16-launch graph per timed window")
    ap.add_argument("--train-batches", type=int, default=20)
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    import numpy as np, torch, taco_amd
    from taco_amd import feeder as F
    assert torch.cuda.is_available(), "bench_feed needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    hp = taco_amd.hparams.copy(max_iters=200)
    r, B, hop = hp.reduction_factor, args.batch, F.hop_length(hp)
    rs = np.random.RandomState(1234)
    base = []
    for j in range(B):
        T = int(rs.randint(args.frames[0], args.frames[1] + 1))
        tok = rs.randint(2, 80, size=args.tokens).astype(np.int32); tok[-1] = 1
        base.append(F.Example(tok, np.float32(1), rs.rand(T, hp.num_mels).astype(np.float32), rs.rand(T, hp.num_freq).astype(np.float32)))
    tmp = tempfile.mkdtemp(prefix="bench_feed_")
    try:
        paths = []
        for j, e in enumerate(base):
            paths.append(os.path.join(tmp, "ex%03d.npz" % j))
            np.savez(paths[-1], tokens=e.tokens, mel=e.mel, linear=e.linear, loss_coeff=e.loss_coeff)
        ev = lambda: torch.cuda.Event(enable_timing=True)

        # ---- (a) host path ----
        def host_batch():
            t0 = time.perf_counter()
            ex = []
            for p in paths:
                z = np.load(p)
                ex.append(F.Example(z["tokens"], z["loss_coeff"], z["mel"], z["linear"]))
            t1 = time.perf_counter()
            b = F.collate(ex, r)
            t2 = time.perf_counter()
            d = [torch.from_numpy(x).to(dev) for x in b[:5]]
            torch.cuda.synchronize()
            return b, d, (t1 - t0, t2 - t1, time.perf_counter() - t2)
        host_batch()
        ta = [host_batch()[2] for _ in range(args.windows)]
        want, _, _ = host_batch()
        arm_a = {"np_load_ms": stats(t[0] * 1e3 for t in ta), "collate_ms": stats(t[1] * 1e3 for t in ta), "upload_ms": stats(t[2] * 1e3 for t in ta),
                 "total_ms": stats(sum(t) * 1e3 for t in ta), "upload_bytes": int(sum(x.nbytes for x in want[:5]))}

        # ---- (b) device corpus, targets ----
        reps = max(1, args.corpus // B)
        N = reps * B
        draws = [rs.permutation(N)[:B].astype(np.int32) for _ in range(16)]
        draws[0] = np.arange(B, dtype=np.int32)                     # the batch arm (a) builds: checked to the bit below
        T_out = F.padded_length(args.frames[1], r)                   # static rectangles sized for the longest example possible
        static = F.Batch(torch.empty((B, args.tokens), dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                         torch.empty(B, dtype=torch.float32, device=dev), torch.empty((B, T_out, hp.num_mels), dtype=torch.float32, device=dev),
                         torch.empty((B, T_out, hp.num_freq), dtype=torch.float32, device=dev), None)
        d_draws = [torch.from_numpy(d).to(dev) for d in draws]
        bytes_written = sum(t.numel() * t.element_size() for t in static[:5])

        def time_collate(corpus):
            got = corpus.collate(draws[0], r)
            same = all(np.array_equal(getattr(got, n).cpu().numpy().view(np.uint32), np.ascontiguousarray(getattr(want, n)).view(np.uint32))
                       for n in ("inputs", "input_lengths", "loss_coeff", "mel_targets", "linear_targets")) if corpus.kind == "targets" else None
            for d in d_draws:
                corpus.collate(d, r, out=static)
            torch.cuda.synchronize()
            eager = []
            for _ in range(args.windows):
                e0, e1 = ev(), ev()
                e0.record()
                for k in range(args.launches):
                    corpus.collate(d_draws[k % 16], r, out=static)
                e1.record(); torch.cuda.synchronize()
                eager.append(e0.elapsed_time(e1) / args.launches)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for d in d_draws:
                    corpus.collate(d, r, out=static)
            g.replay(); torch.cuda.synchronize()
            dev_ms = []
            for _ in range(args.windows):
                e0, e1 = ev(), ev()
                e0.record()
                for _k in range(args.replays):
                    g.replay()
                e1.record(); torch.cuda.synchronize()
                dev_ms.append(e0.elapsed_time(e1) / (16 * args.replays))
            return same, eager, dev_ms

        frames_mean = float(np.mean([len(e.mel) for e in base]))
        bytes_read = int(B * (frames_mean * (hp.num_mels + hp.num_freq) + args.tokens + 1) * 4)
        arm_b, corpus = {}, None
        for align in (4, 1):                                         # the unpadded corpus comes last and feeds arm (e)
            c = F.DeviceCorpus(hp, str(dev), "targets", item_align=align)
            for _ in range(reps):
                for e in base:
                    c.add(e.tokens, e.loss_coeff, mel=e.mel, linear=e.linear)
            c.finalize()
            same, eager, dev_ms = time_collate(c)
            k = "item_align_%d" % align
            arm_b[k] = {"equals_host_collate_bitwise": same, "corpus_bytes": c.nbytes, "per_batch_eager_ms": stats(eager),
                        "per_batch_device_ms_graph_of_16": stats(dev_ms)}
            m = arm_b[k]["per_batch_device_ms_graph_of_16"]["median"]
            arm_b[k]["bytes_read_plus_written_mean"] = bytes_read + bytes_written
            arm_b[k]["TB_per_s_read_plus_written"] = (bytes_read + bytes_written) / (m * 1e-3) / 1e12
            corpus = c

        # ---- (d) the copy yardstick ----
        n_src = max(2, int(600e6 // bytes_written) + 1)
        srcs = [torch.rand(bytes_written // 4, dtype=torch.float32, device=dev) for _ in range(n_src)]
        dst = torch.empty(bytes_written // 4, dtype=torch.float32, device=dev)
        for s in srcs:
            dst.copy_(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for k in range(16):
                dst.copy_(srcs[k % n_src])
        g.replay(); torch.cuda.synchronize()
        td = []
        for _ in range(args.windows):
            e0, e1 = ev(), ev()
            e0.record()
            for _k in range(args.replays):
                g.replay()
            e1.record(); torch.cuda.synchronize()
            td.append(e0.elapsed_time(e1) / (16 * args.replays))
        arm_d = {"bytes_copied": bytes_written, "per_copy_ms_graph_of_16": stats(td),
                 "TB_per_s_read_plus_written": 2 * bytes_written / (stats(td)["median"] * 1e-3) / 1e12}
        del srcs, dst, g

        # ---- (c) device corpus, waveform ----
        wc = F.DeviceCorpus(hp, str(dev), "waveform")
        for _ in range(reps):
            for e in base:
                n = (len(e.mel) - 1) * hop + int(rs.randint(0, hop))
                wc.add(e.tokens, e.loss_coeff, wav=(rs.rand(n).astype(np.float32) - 0.5))
        wc.finalize()
        args_launches = args.launches
        args.launches = max(20, args.launches // 4)
        _, eager_c, dev_c = time_collate(wc)
        args.launches = args_launches
        arm_c = {"corpus_bytes": wc.nbytes, "per_batch_eager_ms": stats(eager_c), "per_batch_device_ms_graph_of_16": stats(dev_c)}
        del wc

        # ---- (e) training steps per second ----
        arm_e = "not measured (--skip-train)"
        if not args.skip_train:
            tr = taco_amd.Trainer(hp, taco_amd.weights.random_weights(hp, 1, seed=4321), device=str(dev))
            tb = [np.sort(rs.permutation(N)[:B]).astype(np.int32) for _ in range(args.train_batches)]
            fixed = corpus.collate(tb[0], r)

            def host_fed(k):
                ex = []
                for i in tb[k]:
                    z = np.load(paths[int(i) % B])
                    ex.append(F.Example(z["tokens"], z["loss_coeff"], z["mel"], z["linear"]))
                b = F.collate(ex, r)
                return tr.train_step(b.inputs, b.input_lengths, b.mel_targets, b.linear_targets, b.loss_coeff)

            def device_fed(k):
                b = corpus.collate(tb[k], r)
                return tr.train_step(b.inputs, b.input_lengths, b.mel_targets, b.linear_targets, b.loss_coeff)

            def alone(k):
                return tr.train_step(fixed.inputs, fixed.input_lengths, fixed.mel_targets, fixed.linear_targets, fixed.loss_coeff)

            res = {}
            for _ in range(2):                                       # alternate the three feeds; the first round is the warm-up
                for name, fn in (("step_alone_fixed_batch", alone), ("fed_by_host_path", host_fed), ("fed_by_device_corpus", device_fed)):
                    for k in range(2):
                        fn(k)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for k in range(args.train_batches):
                        fn(k)
                    torch.cuda.synchronize()
                    res[name] = (time.perf_counter() - t0) / args.train_batches
            tr.check_device_errors()
            arm_e = {k: {"ms_per_step": v * 1e3, "steps_per_s": 1.0 / v} for k, v in res.items()}
            arm_e["batches"] = args.train_batches
            tr.close()

        step_ms = arm_e["step_alone_fixed_batch"]["ms_per_step"] if isinstance(arm_e, dict) else None
        rep = {"metric": "feeding the C4-shard train step", "shape": {"B": B, "tokens": args.tokens, "frames": args.frames, "r": r, "T_out_static": T_out,
                                                                         "corpus_examples": N},
               "a_host_path": arm_a, "b_device_targets": arm_b, "c_device_waveform": arm_c, "d_torch_copy": arm_d, "e_train": arm_e,
               "b_over_d_time": arm_b["item_align_1"]["per_batch_device_ms_graph_of_16"]["median"] / arm_d["per_copy_ms_graph_of_16"]["median"],
               "feeding_below_step": None if step_ms is None else {
                   "b_eager_ms": arm_b["item_align_1"]["per_batch_eager_ms"]["median"], "c_eager_ms": arm_c["per_batch_eager_ms"]["median"],
                   "step_alone_ms": step_ms, "holds": bool(arm_b["item_align_1"]["per_batch_eager_ms"]["median"] < step_ms and
                                                           arm_c["per_batch_eager_ms"]["median"] < step_ms)}}
        print(json.dumps(rep))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
