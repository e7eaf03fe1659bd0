"""Host side of the device-resident corpus (feeder.DeviceCorpus, taco_collate): everything that needs no GPU -- the waveform
rectangle's length identity, the draw parity of Ref sources with NpzSource, the unchanged defaults of bucket / GroupFeeder, the
exported symbol and its argument errors, and the restatement the GPU tests are held to."""
import ctypes as C
import os

import numpy as np
import pytest

import feed_reference as FR
from taco_amd import _lib
from taco_amd import feeder as F

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class _HP(object):
    def __init__(self, **kw):
        self.__dict__.update(dict(num_mels=12, num_freq=65, sample_rate=1600, frame_length_ms=50, frame_shift_ms=12.5, preemphasis=0.97,
                                  min_level_db=-100, ref_level_db=20, power=1.5, griffin_lim_iters=60, reduction_factor=4, max_iters=200))
        self.__dict__.update(kw)


def test_restatement_on_a_hand_made_case():
    """The yardstick itself: two items, a clamped one, an index outside the corpus, zero padding, counts."""
    pack = np.array([9, 1, 2, 3, 4, 5, 6, 9, 7, 8, 9], np.int32)
    s = dict(pack=pack, start=np.array([1, 8], np.int64), rows=np.array([3, 1], np.int32), width=2, rows_out=2)
    out, counts, read = FR.collate_stream(s, [1, 0, 2, -1], 2)
    assert out.tolist() == [[7, 8, 0, 0], [1, 2, 3, 4], [0, 0, 0, 0], [0, 0, 0, 0]] and counts.tolist() == [1, 2, 0, 0]
    assert read.tolist() == [False, True, True, True, True, False, False, False, True, True, False]
    fixed = dict(pack=np.arange(6, dtype=np.float32), start=None, rows=None, width=1, rows_out=2)
    out, counts, _ = FR.collate_stream(fixed, [2, 0], 3)
    assert np.array_equal(out.view(np.float32), [[4, 5], [0, 1]]) and counts.tolist() == [2, 2]


@pytest.mark.parametrize("hop,num_freq,sr,shift", [(20, 65, 1600, 12.5), (300, 1025, 24000, 12.5)])
def test_waveform_rectangle_length_identity(hop, num_freq, sr, shift):
    """Lmax = (T_out - 1) * hop: 1 + Lmax // hop == T_out, Lmax > the longest row and Lmax > n_fft / 2, for every longest length
    from n_fft/2 + 1 up and r in {1, 4, 5} -- what lets Spectrogram.targets write the training rectangles directly."""
    from taco_amd import audio
    hp = _HP(num_freq=num_freq, sample_rate=sr, frame_shift_ms=shift)
    assert F.hop_length(hp) == hop
    assert audio.num_frames(hp, 5 * hop + 1) == 6 and audio.num_frames(hp, 5 * hop - 1) == 5       # the library's hop is the same
    half = (num_freq - 1)
    for r in (1, 4, 5):
        for longest in range(half + 1, half + 1 + 3 * hop * r + 7):
            frames = 1 + longest // hop
            t_out = F.padded_length(frames, r)
            lmax = F.waveform_length(t_out, hop)
            assert 1 + lmax // hop == t_out and lmax > longest and lmax > half, (r, longest, t_out, lmax)
    assert audio.num_frames(hp, half + 1) == 1 + (half + 1) // hop


def _write_dirs(tmp_path, n_dirs=2, per_dir=14, num_mels=12, num_freq=65, seed=3):
    """Tiny `.npz` examples; the first token is a marker that identifies the file (dir * 1000 + j + 2)."""
    rs = np.random.RandomState(seed)
    dirs = []
    for d in range(n_dirs):
        p = tmp_path / ("data%d" % d)
        p.mkdir()
        for j in range(per_dir):
            T, nt = int(rs.randint(4, 40)), int(rs.randint(2, 9))
            tokens = np.concatenate([[d * 1000 + j + 2], rs.randint(2, 80, size=nt - 1), [1]]).astype(np.int32)
            kw = dict(tokens=tokens, mel=rs.rand(T, num_mels).astype(np.float32), linear=rs.rand(T, num_freq).astype(np.float32))
            if j % 3 == 0:
                kw["loss_coeff"] = np.float32(0.5 + j / 10.0)
            np.savez(str(p / ("ex%02d.npz" % j)), **kw)
        dirs.append(str(p))
    return dirs


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("skip_path_filter", [False, True])
def test_ref_sources_draw_what_npz_sources_draw(tmp_path, training, skip_path_filter):
    """Two directories of 14 files, batch_size 4: a GroupFeeder over the corpus's Ref sources hands out the same examples in the same
    rows of the same batches as open_data_dirs does today (examples identified by the marker token), through wraps and reshuffles."""
    dirs = _write_dirs(tmp_path)
    hp = _HP(reduction_factor=4, max_iters=9, min_iters=2, min_tokens=3, initial_phase_step=3, initial_data_greedy=False)
    dt = "train" if training else "test"
    host = F.open_data_dirs(dirs, 4, hp, data_type=dt, batches_per_group=4, seed=11, skip_path_filter=skip_path_filter)
    corpus = F.DeviceCorpus.from_data_dirs(dirs, hp, device=None, finalize=False)
    assert len(corpus) == 28 and [r.index for r in corpus.refs()] == list(range(28))
    marker = {r.index: int(np.load(p)["tokens"][0]) for p, r in ((p, corpus.ref_of(p)) for p in corpus._path_index)}
    seen = []
    dev = F.open_data_dirs(dirs, 4, hp, data_type=dt, batches_per_group=4, seed=11, skip_path_filter=skip_path_filter, corpus=corpus,
                           collate_fn=lambda refs, r: seen.append((r, list(refs))) or refs)
    assert all(isinstance(s, F.RefSource) and s.offset == 2 for s in dev.sources.values())
    for _ in range(10):                       # 40 draws per directory-pair phase: several wraps of the 10-path training lists
        want = next(host)
        got = next(dev)
        assert [int(row[0]) for row in want.inputs] == [marker[ref.index] for ref in got]
        assert want.input_lengths.tolist() == [ref.n_tokens for ref in got]
        assert want.speaker_id.tolist() == [ref.speaker_id for ref in got]
        assert want.mel_targets.shape[1] == F.padded_length(max(ref.n_frames for ref in got), 4)
    assert len(seen) == 10 and all(r == 4 for r, _ in seen)
    assert host.step == dev.step == 10


def test_defaults_still_reproduce_the_reference_vectors():
    """bucket / GroupFeeder with the new arguments at their defaults (and with the defaults spelled out) against
    tests/golden/feeder_vectors.npz, as tests/test_reference_vectors.py checks them."""
    import test_reference_vectors as TRV
    fv = np.load(os.path.join(GOLD, "feeder_vectors.npz"))
    TRV.test_group_logic_equals_enqueue_next_group(fv)
    TRV.test_prepare_batch_cases(fv)
    for gi, row in enumerate(fv["groups"].tolist()):
        bs, bpg, r, ndirs, step, phase, seed = row[:7]
        dirs = [str(d) for d in fv["group%d_dirs" % gi]]
        streams = {d: iter(TRV._examples(fv, "group%d_%s" % (gi, d), int(fv["group%d_%s_count" % (gi, d)]), ndirs > 1)) for d in dirs}
        feeder = F.GroupFeeder({d: (lambda d=d: next(streams[d])) for d in dirs}, bs, r, batches_per_group=bpg,
                               ratios=dict(zip(dirs, [x / 1000.0 for x in row[7:7 + ndirs]])), seed=seed, training=True,
                               initial_phase_step=phase, initial_data_greedy=bool(row[9]), step=step, collate_fn=F.collate,
                               length=lambda e: len(e.mel))
        for bi in range(int(fv["group%d_nbatches" % gi])):
            TRV._same(next(feeder), fv, "group%d_batch%d_" % (gi, bi), ndirs > 1)
    ex = [F.Example(np.arange(3), 1, np.zeros((t, 2)), np.zeros((t, 3))) for t in (5, 2, 9, 2, 7, 1)]
    a = F.bucket(list(ex), 2, np.random.RandomState(5))
    b = F.bucket(list(ex), 2, np.random.RandomState(5), length=lambda e: len(e.mel))
    assert [[id(e) for e in x] for x in a] == [[id(e) for e in x] for x in b]


def test_corpus_bookkeeping_without_a_device(tmp_path):
    """add / refs / source / save / load on the host: kinds, refusals, the tables a draw needs."""
    hp = _HP()
    c = F.DeviceCorpus(hp, None, "waveform")
    with pytest.raises(Exception, match="too short"):
        c.add([5, 1], wav=np.zeros(64, np.float32))               # n_fft / 2 = 64
    assert c.add([5, 6, 1], wav=np.zeros(65, np.float32)) == 0 and c.add([5, 1], 0.5, wav=np.zeros(161, np.float32)) == 1
    assert c.refs() == [F.Ref(0, 3, 4, None), F.Ref(1, 2, 9, None)]
    with pytest.raises(Exception, match="speaker_id"):
        c.add([5, 1], wav=np.zeros(99, np.float32), speaker_id=1)
    with pytest.raises(Exception, match="kind"):
        F.DeviceCorpus(hp, None, "mp3")
    t = F.DeviceCorpus(hp, None, "targets", item_align=4)
    with pytest.raises(Exception, match="mel must be"):
        t.add([5, 1], mel=np.zeros((3, 12)), linear=np.zeros((4, 65)))
    for j, T in enumerate((3, 5, 2)):
        t.add(np.arange(2, 4 + j), 1 + j, mel=np.full((T, 12), j + 1.0), linear=np.full((T, 65), j + 2.0), speaker_id=j % 2, path="p%d" % j)
    assert t.nbytes > 0
    t.save(str(tmp_path / "corpus.npz"))
    u = F.DeviceCorpus.load(str(tmp_path / "corpus.npz"), device=None)
    assert u.kind == "targets" and u.refs() == t.refs() and u.ref_of("p2") == F.Ref(2, 4, 2, 0) and u.nbytes == t.nbytes
    assert (u._packs["mel_start"] % 4 == 0).all() and u._packs["mel_start"].tolist() == [0, 36, 96]
    src = u.source(["p0", "gone", "p1", "p2"], None, np.random.RandomState(0), training=False)
    with pytest.raises(Exception, match="speaker_id"):
        src()                                                      # stored with speaker ids, drawn for a single-speaker source
    src = t.source([0, 2], 0, np.random.RandomState(0), training=False)
    assert [src().index for _ in range(3)] == [0, 2, 0]           # cursor starts past the end of a 2-item list: wraps at once
    with pytest.raises(Exception, match="finalize"):
        t.collate([0], 4)


def test_library_exports_taco_collate_and_refuses_bad_arguments():
    lib = _lib.load_library()
    assert hasattr(lib, "taco_collate") and "taco_collate" in _lib.PROTOTYPES
    assert C.sizeof(_lib.TacoCollateStream) == 48 and _lib.TACO_COLLATE_MAX_STREAMS == 8
    d_ok = 0x1000                                                  # never dereferenced: every case fails before any device call

    def call(n_streams=1, index=d_ok, B=1, N=1, streams=True, **kw):
        arr = (_lib.TacoCollateStream * 9)()
        for a in arr:
            a.pack, a.start, a.rows, a.width, a.rows_out, a.out, a.counts = d_ok, d_ok, d_ok, 1, 1, d_ok, None
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return lib.taco_collate(None, arr if streams else None, n_streams, index, B, N)

    assert call(streams=False) == _lib.TACO_ERR_ARG
    assert call(index=None) == _lib.TACO_ERR_ARG
    assert call(pack=None) == _lib.TACO_ERR_ARG and call(out=None) == _lib.TACO_ERR_ARG
    assert call(n_streams=0) == _lib.TACO_ERR_ARG and call(n_streams=9) == _lib.TACO_ERR_ARG
    assert call(width=0) == _lib.TACO_ERR_ARG and call(rows_out=0) == _lib.TACO_ERR_ARG
    assert call(B=0) == _lib.TACO_ERR_ARG and call(N=0) == _lib.TACO_ERR_ARG
    assert call(start=None) == _lib.TACO_ERR_ARG                   # rows without start
    assert b"taco_collate" in lib.taco_last_error()
