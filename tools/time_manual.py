#!/usr/bin/env python
"""Second pass of synthesize(manual_attention_mode=1) (synthesizer.py:171-205: the forward is run again with one-hot manual
alignments) against the first pass, at C2 shapes; and model type 'simple' against 'single'.  Both used to fall back to the
launch-per-stage decoder (43 us per step); they are modes of the persistent decoder now.

Then the whole two-pass call both ways: the second pass's alignments built on the host (the first pass's alignments downloaded,
manual_alignments_of, an upload: the route of the commits before k_manual_alignments, kept here for the comparison) and on the
device (run(manual_attention_mode=1)); and the kernel alone.

    python tools/time_manual.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch, taco_amd
from taco_amd.synthesizer import manual_alignments_of
B, T_in, n = 32, 128, 128


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for mt, ns in (("single", 1), ("simple", 4)):
    hp = taco_amd.hparams.copy(max_iters=n, model_type=mt)
    m = taco_amd.create_model(hp); m.load_weights(taco_amd.weights.random_weights(hp, ns, seed=1)); m.initialize(None, None, ns, None)
    rs = np.random.RandomState(1)
    ids = rs.randint(2, 80, size=(B, T_in)).astype(np.int32); ids[:, -1] = 1
    L = taco_amd.input_lengths_from_tokens(ids)
    spk = (np.arange(B) % ns).astype(np.int32) if ns > 1 else None
    lin, al = m.run(inputs=ids, input_lengths=L, speaker_id=spk, honor_stop=False)
    onehot = torch.zeros((B, n, T_in), device=al.device)
    onehot.scatter_(2, al.argmax(1).unsqueeze(2), 1.0)                     # [B, n, T_in] one-hot of the first pass's argmax
    t1 = timed(lambda: m.run(inputs=ids, input_lengths=L, speaker_id=spk, honor_stop=False))
    t2 = timed(lambda: m.run(inputs=ids, input_lengths=L, speaker_id=spk, manual_alignments=onehot, is_manual_attention=True, honor_stop=False))
    enc = m.encoder(ids, L, spk)
    d1 = timed(lambda: m.decoder(enc, n, spk))
    d2 = timed(lambda: m.decoder(enc, n, spk, manual_alignments=onehot))
    m.check_device_errors()
    print("%-7s forward %.3f ms, with manual alignments %.3f ms (x%.2f); decoder loop alone %.3f -> %.3f ms (%.2f -> %.2f us per step); engine %s"
          % (mt, t1, t2, t2 / t1, d1, d2, d1 * 1e3 / n, d2 * 1e3 / n, m.decoder_engine_info()))

    # ---- the two passes as one call: the second pass's alignments from the host, from the device ----
    def host_built(mode=1):
        _, a = m.run(inputs=ids, input_lengths=L, speaker_id=spk, honor_stop=False)
        return m.run(inputs=ids, input_lengths=L, speaker_id=spk, manual_alignments=manual_alignments_of(a.cpu().numpy(), mode),
                     is_manual_attention=True, honor_stop=False)

    def device_built(mode=1):
        return m.run(inputs=ids, input_lengths=L, speaker_id=spk, honor_stop=False, manual_attention_mode=mode)

    want = [t.clone() for t in host_built()]                               # both routes return the manual plan's own buffers
    same = all(torch.equal(x, y) for x, y in zip(want, device_built()))
    th, td = [], []
    for _ in range(3):                                                     # alternated: both see the same box in the same minute
        th.append(timed(host_built, reps=10)); td.append(timed(device_built, reps=10))
    first = m.first_pass_alignments.clone()
    buf = torch.empty((B, n, T_in), dtype=torch.float32, device=first.device)
    tk, tg = {}, {}
    for mode in (1, 3):
        call = lambda: m.manual_alignments_from(first, mode, out=buf)
        tk[mode] = min(timed(call, reps=200) for _ in range(3))            # one call at a time from Python: its launch path included
        g, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        with torch.cuda.graph(g, stream=side):                             # 100 calls back to back in one graph: the kernel itself
            for _ in range(100):
                call()
        tg[mode] = min(timed(g.replay, reps=5) for _ in range(3)) / 100
    m.check_device_errors()
    print("%-7s two passes, alignments built on the host %.3f ms (runs %s), on the device %.3f ms (runs %s): x%.2f, outputs bit-identical: %s; "
          "k_manual_alignments alone on [%d, %d, %d]: %.2f us (mode 1), %.2f us (mode 3) per call back to back in one graph (%.0f GB/s of "
          "its mode 3 traffic, one read for the argmax, one for the copy, one write); %.2f / %.2f us per call from Python"
          % (mt, min(th), " ".join("%.3f" % v for v in th), min(td), " ".join("%.3f" % v for v in td), min(td) / min(th), same,
             B, T_in, n, tg[1] * 1e3, tg[3] * 1e3, 3 * 4 * B * T_in * n / (tg[3] * 1e-3) / 1e9, tk[1] * 1e3, tk[3] * 1e3))
    m.close()
