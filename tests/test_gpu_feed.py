"""taco_collate (csrc/taco_feed.h) and feeder.DeviceCorpus on the GPU.  Every comparison is on the bits (arrays viewed as uint32):
the kernel against the NumPy restatement tests/feed_reference.py, DeviceCorpus.collate against the host feeder.collate on the same
examples, the waveform corpus against Spectrogram.targets on the host-collated rectangle, a device-fed train step against the
host-fed one.  Packs carry 1e3 in their slack and between items, outputs and counts are pre-filled with a poison pattern."""
import ctypes as C

import numpy as np
import pytest

import feed_reference as FR
from test_feed_host import _HP, _write_dirs

pytestmark = pytest.mark.gpu

POISON = 0xDEADBEEF
SLACK = np.float32(1.0e3)
FIELDS = ("inputs", "input_lengths", "loss_coeff", "mel_targets", "linear_targets", "speaker_id")


def _bits(t):
    return FR.words(t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t))


def _poisoned(shape, dtype, dev="cuda:0"):
    import torch
    return torch.full(shape, POISON - (1 << 32), dtype=torch.int32, device=dev).view(dtype)


def _ragged_stream(width, rows_out, rows, rs, dtype=np.float32, lead=0):
    """Items of `rows` rows laid out with 1e3-filled gaps of 0..3 words (item k starts `lead + ...` so that all four residues modulo 4
    words occur), the last item ending on the pack's last word."""
    start, parts, off = [], [], 0
    for k, n in enumerate(rows):
        gap = (lead + k) % 4 if k else lead
        parts.append(np.full(gap, SLACK, np.float32).view(np.uint32))
        off += gap
        start.append(off)
        item = (rs.rand(n * width).astype(np.float32) + 1).view(np.uint32) if dtype == np.float32 else rs.randint(1, 1 << 20, size=n * width).astype(np.int32).view(np.uint32)
        parts.append(item)
        off += n * width
    pack = np.concatenate(parts)
    assert start[-1] + rows[-1] * width == pack.size
    return dict(pack=pack.view(dtype), start=np.asarray(start, np.int64), rows=np.asarray(rows, np.int32), width=width, rows_out=rows_out)


def _launch(streams, index_dev, B, N, outs=None, with_counts=True):
    """Uploads the streams, runs ONE taco_collate on the current stream; returns (device outs, device counts, keep-alive list)."""
    import torch
    from taco_amd import _lib
    lib = _lib.load_library()
    keep, arr = [], (_lib.TacoCollateStream * len(streams))()
    outs_d, counts_d = [], []
    for k, (a, s) in enumerate(zip(arr, streams)):
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
        pack, start, rows = up(s["pack"]), up(s.get("start")), up(s.get("rows"))
        out = _poisoned((B, s["rows_out"], s["width"]), torch.int32) if outs is None else outs[k]
        cnt = _poisoned((B,), torch.int32) if with_counts else None
        keep += [pack, start, rows]
        a.pack, a.start, a.rows = pack.data_ptr(), None if start is None else start.data_ptr(), None if rows is None else rows.data_ptr()
        a.width, a.rows_out, a.out, a.counts = s["width"], s["rows_out"], out.data_ptr(), None if cnt is None else cnt.data_ptr()
        outs_d.append(out)
        counts_d.append(cnt)
    call = lambda: _lib.check(lib.taco_collate(C.c_void_p(torch.cuda.current_stream().cuda_stream), arr, len(streams), C.c_void_p(index_dev.data_ptr()), B, N))
    call()
    return outs_d, counts_d, keep + [arr], call


def _check(streams, index, N, outs_d, counts_d):
    for k, s in enumerate(streams):
        want, cw, _ = FR.collate_stream(s, index, N)
        got = _bits(outs_d[k]).reshape(len(index), -1)
        bad = np.argwhere(got != want)
        assert not len(bad), "stream %d (width %d, rows_out %d): first differing (row, word) %s of %d; got %#x want %#x" % (
            k, s["width"], s["rows_out"], bad[0].tolist(), len(bad), got[tuple(bad[0])], want[tuple(bad[0])])
        if counts_d[k] is not None:
            assert counts_d[k].cpu().numpy().tolist() == cw.tolist(), k


def _eight_streams(rs):
    """Widths 1, 5, 12, 65, 1025; rows_out * width both a multiple of 4 (12 x 5, 65 x 4) and not (1025 x 9: r = 5's odd rectangles; 5 x 7;
    1 x 3); rows 0, 1, exactly rows_out, more than rows_out (clamped) and in between; the 1025 x 9 row spans three workgroups, the 1 x 3
    row is smaller than one lane's access; two fixed-size streams (start and rows NULL)."""
    N = 6
    mk = lambda w, ro, lead, dt=np.float32: _ragged_stream(w, ro, [ro, 0, 1, ro + 3, max(ro - 2, 1), ro + 1], rs, dt, lead)
    streams = [mk(1, 3, 1, np.int32), mk(5, 7, 2), mk(12, 5, 3), mk(65, 4, 0), mk(1025, 9, 1), mk(1, 4100, 2),
               dict(pack=(rs.rand(N).astype(np.float32) + 1), start=None, rows=None, width=1, rows_out=1),
               dict(pack=rs.randint(1, 99, size=N * 3 * 5).astype(np.int32), start=None, rows=None, width=5, rows_out=3)]
    return streams, N


@pytest.mark.parametrize("index", [[3], [2, 0, 2, -1, 6, 4, 1], [5, 3, 1, 0, 5, 3, 1, 0, 2]], ids=["B1", "B7_repeat_and_outside", "B9"])
def test_collate_kernel_equals_the_restatement(index):
    import torch
    streams, N = _eight_streams(np.random.RandomState(17))
    idx = torch.tensor(index, dtype=torch.int32, device="cuda")
    outs, counts, _keep, _ = _launch(streams, idx, len(index), N)
    torch.cuda.synchronize()
    _check(streams, index, N, outs, counts)


def test_collate_serves_every_alignment_of_source_and_destination():
    """Destination bases at all four residues modulo 16 bytes (a view into a larger poisoned buffer) against item starts at all four:
    the words around the output stay poison."""
    import torch
    rs = np.random.RandomState(23)
    index = [1, 3, 0, 2]
    for shift in range(4):
        s = _ragged_stream(5, 7, [7, 3, 9, 6], rs, lead=1)
        big = _poisoned((4 * 35 + 8,), torch.int32)
        out = big[shift:shift + 4 * 35].view(4, 7, 5)
        idx = torch.tensor(index, dtype=torch.int32, device="cuda")
        outs, counts, _keep, _ = _launch([s], idx, 4, 4, outs=[out])
        torch.cuda.synchronize()
        _check([s], index, 4, outs, counts)
        edge = _bits(big)
        assert (edge[:shift] == POISON).all() and (edge[shift + 140:] == POISON).all()


def test_collate_offsets_are_64_bit():
    """One item of 4096 words that starts beyond 2^31 words of the pack (the pack is uninitialised memory, only the item is written)."""
    import torch
    from taco_amd import _lib
    if torch.cuda.mem_get_info()[0] < 16e9:
        pytest.skip("needs 16 GB of free device memory")
    at = (1 << 31) + 5
    pack = torch.empty(at + 4096, dtype=torch.float32, device="cuda")
    item = torch.arange(1, 4097, dtype=torch.float32, device="cuda")
    pack[at:] = item
    start = torch.tensor([at], dtype=torch.int64, device="cuda")
    rows = torch.tensor([4096], dtype=torch.int32, device="cuda")
    out, cnt = _poisoned((1, 4100, 1), torch.float32), _poisoned((1,), torch.int32)
    idx = torch.zeros(1, dtype=torch.int32, device="cuda")
    a = (_lib.TacoCollateStream * 1)()
    a[0].pack, a[0].start, a[0].rows, a[0].width, a[0].rows_out, a[0].out, a[0].counts = pack.data_ptr(), start.data_ptr(), rows.data_ptr(), 1, 4100, out.data_ptr(), cnt.data_ptr()
    _lib.check(_lib.load_library().taco_collate(C.c_void_p(torch.cuda.current_stream().cuda_stream), a, 1, C.c_void_p(idx.data_ptr()), 1, 1))
    torch.cuda.synchronize()
    got = out.cpu().numpy().reshape(-1)
    assert np.array_equal(got[:4096], np.arange(1, 4097, dtype=np.float32)) and (_bits(got[4096:]) == 0).all() and int(cnt[0]) == 4096
    del pack


def test_collate_replayed_from_a_graph_follows_the_index_tensor():
    import torch
    streams, N = _eight_streams(np.random.RandomState(29))
    first, second = [0, 1, 2, 3, 4], [5, 2, 6, 0, 2]
    idx = torch.tensor(first, dtype=torch.int32, device="cuda")
    outs, counts, _keep, call = _launch(streams, idx, 5, N)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for o in outs + counts:
        o.view(torch.int32).fill_(POISON - (1 << 32))
    idx.copy_(torch.tensor(second, dtype=torch.int32))
    g.replay()
    torch.cuda.synchronize()
    _check(streams, second, N, outs, counts)


# ---- DeviceCorpus ----
def _examples(n=9, num_mels=12, num_freq=65, seed=41, speakers=True):
    from taco_amd import feeder as F
    rs = np.random.RandomState(seed)
    ex = []
    for j in range(n):
        T, nt = int(rs.randint(1, 23)), int(rs.randint(1, 11))
        ex.append(F.Example(rs.randint(2, 80, size=nt).astype(np.int32), np.float32(0.5 + 0.25 * j), rs.rand(T, num_mels).astype(np.float32),
                            rs.rand(T, num_freq).astype(np.float32), (j * 7) % 4 if speakers else None))
    return ex


def _corpus(ex, hp, **kw):
    from taco_amd import feeder as F
    c = F.DeviceCorpus(hp, "cuda:0", "targets", **kw)
    for e in ex:
        c.add(e.tokens, e.loss_coeff, mel=e.mel, linear=e.linear, speaker_id=e.speaker_id)
    return c.finalize()


def _same_batch(got, want):
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if w is None:
            assert g is None, name
            continue
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, w.dtype, g.shape, w.shape)
        assert np.array_equal(_bits(g), _bits(w)), name


def _poisoned_batch(want):
    import torch
    from taco_amd import feeder as F
    dt = {np.dtype(np.int32): torch.int32, np.dtype(np.float32): torch.float32}
    return F.Batch(*[None if getattr(want, n) is None else _poisoned(getattr(want, n).shape, dt[getattr(want, n).dtype]) for n in FIELDS])


@pytest.mark.parametrize("r", [4, 5])
@pytest.mark.parametrize("item_align", [1, 4])
def test_device_corpus_targets_equal_the_host_collate(tmp_path, r, item_align):
    import torch
    from taco_amd import feeder as F
    import taco_amd
    assert taco_amd.DeviceCorpus is F.DeviceCorpus
    hp = _HP()
    ex = _examples()
    c = _corpus(ex, hp, item_align=item_align)
    assert c.nbytes >= sum(e.mel.nbytes + e.linear.nbytes + e.tokens.nbytes for e in ex)
    for indices in ([4, 0, 8, 2, 2], [7], list(range(9))):
        want = F.collate([ex[i] for i in indices], r)
        _same_batch(c.collate(indices, r), want)
        out = _poisoned_batch(want)
        ret = c.collate(indices, r, out=out)
        assert all(getattr(ret, n) is getattr(out, n) for n in FIELDS)
        _same_batch(out, want)
        out = _poisoned_batch(want)                                  # a device index tensor: shapes come from out=
        c.collate(torch.tensor(indices, dtype=torch.int32, device="cuda"), r, out=out)
        _same_batch(out, want)
    c.save(str(tmp_path / "c.npz"))
    d = F.DeviceCorpus.load(str(tmp_path / "c.npz"), "cuda:0")
    assert d.refs() == c.refs() and d.nbytes == c.nbytes
    _same_batch(d.collate([4, 0, 8, 2, 2], r), F.collate([ex[i] for i in [4, 0, 8, 2, 2]], r))
    with pytest.raises(Exception, match="out.inputs"):
        c.collate([1, 2], r, out=_poisoned_batch(want))
    with pytest.raises(IndexError):
        c.collate([9], r)


def test_device_corpus_without_speakers_and_a_corpus_that_does_not_fit(monkeypatch):
    import torch
    from taco_amd import feeder as F
    hp = _HP()
    ex = _examples(5, seed=43, speakers=False)
    c = _corpus(ex, hp)
    got = c.collate([3, 1, 4], 4)
    assert got.speaker_id is None
    _same_batch(got, F.collate([ex[i] for i in (3, 1, 4)], 4))
    big = F.DeviceCorpus(hp, "cuda:0", "targets")
    for e in ex:
        big.add(e.tokens, e.loss_coeff, mel=e.mel, linear=e.linear)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1000, 288 << 30))
    with pytest.raises(Exception, match=r"needs \d+ bytes .* only 1000 are free"):
        big.finalize()


def test_device_corpus_waveform_equals_spectrogram_targets_on_the_host_collated_rectangle():
    import torch
    import taco_amd
    import spec_reference as R
    from taco_amd import feeder as F
    from test_gpu_spec import SMALL, _HP as SpecHP
    hp = SpecHP(SMALL["ahp"], SMALL["num_mels"])
    hp.num_freq = SMALL["ahp"].num_freq
    r = 4
    ns = [727, 460, 161, 65, 300]
    wavs = [R.test_signal(n, SMALL["ahp"].sample_rate, 200 + b).astype(np.float32) for b, n in enumerate(ns)]
    toks = [np.arange(2, 4 + b, dtype=np.int32) for b in range(5)]
    c = F.DeviceCorpus(hp, "cuda:0", "waveform")
    with pytest.raises(Exception, match="too short"):
        c.add(toks[0], wav=wavs[0][:64])
    for b in range(5):
        c.add(toks[b], 1 + b, wav=wavs[b])
    c.finalize()
    hop = F.hop_length(hp)
    assert hop == 20 and [x.n_frames for x in c.refs()] == [1 + n // hop for n in ns]
    spec = taco_amd.Spectrogram(hp)
    for indices in ([0, 1, 2, 3, 4], [3, 2, 4]):
        frames = [1 + ns[i] // hop for i in indices]
        t_out = F.padded_length(max(frames), r)
        lmax = (t_out - 1) * hop
        rect = np.zeros((len(indices), lmax), np.float32)
        for b, i in enumerate(indices):
            rect[b, :ns[i]] = wavs[i]
        lin, mel, nf = spec.targets(rect, np.asarray([ns[i] for i in indices], np.int32))
        got = c.collate(indices, r)
        again = c.collate(indices, r)
        assert tuple(got.linear_targets.shape) == (len(indices), t_out, 65) and tuple(got.mel_targets.shape) == (len(indices), t_out, 12)
        assert np.array_equal(_bits(got.linear_targets), _bits(lin)) and np.array_equal(_bits(got.mel_targets), _bits(mel))
        assert np.array_equal(_bits(got.linear_targets), _bits(again.linear_targets)) and np.array_equal(_bits(got.mel_targets), _bits(again.mel_targets))
        assert nf.cpu().numpy().tolist() == frames
        for b, f in enumerate(frames):
            assert (_bits(got.linear_targets[b, f:]) == 0).all() and (_bits(got.mel_targets[b, f:]) == 0).all()
            assert float(got.linear_targets[b, :f].abs().sum()) > 0
        assert got.input_lengths.cpu().numpy().tolist() == [len(toks[i]) for i in indices]
        assert got.loss_coeff.cpu().numpy().tolist() == [1.0 + i for i in indices]
        want_in = np.zeros((len(indices), max(len(toks[i]) for i in indices)), np.int32)
        for b, i in enumerate(indices):
            want_in[b, :len(toks[i])] = toks[i]
        assert np.array_equal(got.inputs.cpu().numpy(), want_in)
        out = F.Batch(_poisoned(want_in.shape, torch.int32), _poisoned((len(indices),), torch.int32), _poisoned((len(indices),), torch.float32),
                      _poisoned(tuple(mel.shape), torch.float32), _poisoned(tuple(lin.shape), torch.float32), None)
        c.collate(indices, r, out=out)
        assert np.array_equal(_bits(out.linear_targets), _bits(lin)) and np.array_equal(_bits(out.mel_targets), _bits(mel))
    spec.close()


def test_device_feeder_hands_out_the_host_feeders_batches(tmp_path):
    from taco_amd import feeder as F
    dirs = _write_dirs(tmp_path)
    hp = _HP(reduction_factor=5, max_iters=9, min_iters=1, min_tokens=3, initial_phase_step=1, initial_data_greedy=False)
    corpus = F.DeviceCorpus.from_data_dirs(dirs, hp, "cuda:0")
    host = F.open_data_dirs(dirs, 4, hp, batches_per_group=2, seed=5)
    dev = F.open_data_dirs(dirs, 4, hp, batches_per_group=2, seed=5, corpus=corpus)
    for _ in range(3):
        _same_batch(next(dev), next(host))


def test_train_step_on_a_device_collated_batch_equals_the_host_collated_one():
    """Same weights, same examples: the four losses and the whole gradient bucket to the bit (deterministic reductions)."""
    import torch
    import taco_amd
    import taco_oracle as O
    from taco_amd import feeder as F
    from util import tiny_hp, to_product_hp
    ohp = tiny_hp(attention_type="bah_mon")
    hp = to_product_hp(ohp)
    w = O.init_weights(ohp, 1, 5)
    rs = np.random.RandomState(9)
    ex = [F.Example(np.concatenate([rs.randint(2, 30, size=nt - 1), [1]]).astype(np.int32), np.float32(co), rs.rand(T, hp.num_mels).astype(np.float32),
                    rs.rand(T, hp.num_freq).astype(np.float32)) for nt, T, co in ((9, 11, 0.5), (4, 17, 1.0), (7, 6, 1.5))]
    want = F.collate(ex, hp.reduction_factor)
    c = F.DeviceCorpus(hp, "cuda:0", "targets")
    for e in ex:
        c.add(e.tokens, e.loss_coeff, mel=e.mel, linear=e.linear)
    got = c.finalize().collate([0, 1, 2], hp.reduction_factor)
    res = []
    for b in (want, got):
        tr = taco_amd.Trainer(hp, w)
        tr.set_deterministic(True)
        step, _ = tr.train_step(b.inputs, b.input_lengths, b.mel_targets, b.linear_targets, b.loss_coeff)
        torch.cuda.synchronize()
        tr.check_device_errors()
        res.append((step, tr.losses.cpu().numpy().copy(), tr.grads.cpu().numpy().copy()))
        tr.close()
    assert res[0][0] == res[1][0] == 1 and np.isfinite(res[0][1]).all()
    assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])) and np.array_equal(_bits(res[0][2]), _bits(res[1][2]))
