"""Training-side batcher: the contract the reference's DataFeeder hands to `train.py` (datasets/datafeeder.py:210-243,289-328),
as plain host code with its own shape.

* `Example`   one utterance: token ids (EOS included), loss coefficient, mel [T, num_mels], linear [T, num_freq], speaker id.
* `collate`   a list of examples -> one `Batch` of dense arrays.  Inputs are zero-padded to the longest token row; targets are
              zero-padded to the next multiple of the reduction factor ABOVE the longest target (at least one padding frame, so
              the model always sees an end of utterance); `input_lengths` counts the tokens including the EOS -- the feeder's
              convention (the synthesizer instead uses the index of the EOS, synthesizer.py:120).
* `bucket`    length bucketing of one GROUP of examples (batch_size x batches_per_group of them): sort by target length, cut into
              consecutive batches (each batch then pads little), shuffle the ORDER of the batches, and -- for training data -- the
              rows inside each batch.
* `GroupFeeder`  iterator over batches that draws group after group from one or several example sources, with the reference's
              per-dataset draw ratios.
* `NpzSource`  one data directory of the reference's own training examples -- `*.npz` with `tokens`, `mel`, `linear` and optionally
              `loss_coeff`, the files its preprocessing writes -- drawn as DataFeeder._get_next_example draws them
              (datafeeder.py:245-287); `frame_limits` / `filter_items` / `split_paths` / `data_ratios` are the path bookkeeping of
              get_path_dict (:26-76) and DataFeeder.__init__ (:104-121).
* `DeviceCorpus`  the same examples held ON THE DEVICE (precomputed targets, or waveforms that become targets per batch), collated
              by one kernel launch (taco_collate, csrc/taco_feed.h).  The host keeps only what the draw logic needs -- a `Ref`
              (index, token count, frame count, speaker) per example -- and `RefSource` / `GroupFeeder(collate_fn=...)` draw, bucket
              and batch those exactly as `NpzSource` / `GroupFeeder` do the examples themselves."""
import os
import collections

import numpy as np
import torch

from . import _lib
from ._device import STREAM, call, pointer

Example = collections.namedtuple("Example", "tokens loss_coeff mel linear speaker_id")
Example.__new__.__defaults__ = (None,)
Batch = collections.namedtuple("Batch", "inputs input_lengths loss_coeff mel_targets linear_targets speaker_id")


def padded_length(longest, reduction_factor):
    """Frames a target batch is padded to: the smallest multiple of r that is > longest... unless longest + 1 already is one."""
    return -(-(longest + 1) // reduction_factor) * reduction_factor


def _stack_rows(rows, length, dtype):
    first = np.asarray(rows[0])
    out = np.zeros((len(rows), length) + first.shape[1:], dtype)
    for i, r in enumerate(rows):
        r = np.asarray(r)
        out[i, :len(r)] = r
    return out


def collate(examples, reduction_factor):
    ex = [e if isinstance(e, Example) else Example(*e) for e in examples]
    t_in = max(len(e.tokens) for e in ex)
    t_out = padded_length(max(len(e.mel) for e in ex), reduction_factor)
    spk = None
    if ex[0].speaker_id is not None:
        spk = np.asarray([e.speaker_id for e in ex], np.int32)
    return Batch(_stack_rows([e.tokens for e in ex], t_in, np.int32),
                 np.asarray([len(e.tokens) for e in ex], np.int32),
                 np.asarray([e.loss_coeff for e in ex], np.float32),
                 _stack_rows([e.mel for e in ex], t_out, np.float32),
                 _stack_rows([e.linear for e in ex], t_out, np.float32), spk)


def _target_length(e):
    return len(e.mel if isinstance(e, Example) else e[2])


def bucket(examples, batch_size, rng, shuffle_rows=True, length=None):
    """One group of examples -> list of lists (batches), bucketed by target length.  length: example -> target frames (default: the
    rows of its mel target; Ref sources pass the recorded frame count)."""
    length = _target_length if length is None else length
    order = sorted(range(len(examples)), key=lambda i: length(examples[i]))
    batches = [[examples[i] for i in order[k:k + batch_size]] for k in range(0, len(order), batch_size)]
    rng.shuffle(batches)
    if shuffle_rows:
        for b in batches:
            rng.shuffle(b)
    return batches


class GroupFeeder(object):
    """sources: {name: callable returning the next Example}; ratios: {name: share of a group} (equal shares when None).

    The reference's two phases (datafeeder.py:219-231): while `step` (batches handed out so far) is below `initial_phase_step` every
    source contributes batch_size * batches_per_group // len(sources) examples -- and with `initial_data_greedy` all of them come from
    the first source whose name contains "krbook", if there is one; from then on source d contributes
    int(batch_size * batches_per_group * ratios[d]).

    collate_fn(batch, reduction_factor) turns one bucketed batch into what the iterator hands out (default: `collate`), and `length`
    is `bucket`'s key; a DeviceCorpus feeder passes its own pair and Ref sources."""

    def __init__(self, sources, batch_size, reduction_factor, batches_per_group=32, ratios=None, seed=123, training=True,
                 initial_phase_step=0, initial_data_greedy=False, step=0, collate_fn=None, length=None):
        self.sources = dict(sources)
        self.collate_fn, self.length = (collate if collate_fn is None else collate_fn), length
        self.batch_size, self.r, self.bpg, self.training = batch_size, reduction_factor, batches_per_group, training
        n = len(self.sources)
        self.ratios = {k: (1.0 / n if ratios is None else ratios[k]) for k in self.sources}
        self.initial_phase_step, self.initial_data_greedy = initial_phase_step, initial_data_greedy
        self.rng = np.random.RandomState(seed)
        self._pending = []
        self.step = step

    def next_group(self):
        group = []
        names = list(self.sources)
        initial = self.step < self.initial_phase_step
        for name in names:
            draw_from = name
            if self.initial_data_greedy and initial and any("krbook" in d for d in names):
                draw_from = [d for d in names if "krbook" in d][0]
            count = int(self.batch_size * self.bpg // len(names)) if initial else int(self.batch_size * self.bpg * self.ratios[name])
            for _ in range(count):
                group.append(self.sources[draw_from]())
        return bucket(group, self.batch_size, self.rng, shuffle_rows=self.training, length=self.length)

    def __iter__(self):
        return self

    def __next__(self):
        if not self._pending:
            self._pending = self.next_group()
            if not self._pending:
                raise StopIteration
        self.step += 1
        return self.collate_fn(self._pending.pop(0), self.r)


# ---- the reference's on-disk examples (datasets/datafeeder.py:20-76,104-121,245-287) ----
def frame_limits(reduction_factor, min_iters, max_iters):
    """(min_n_frame, max_n_frame) of datafeeder.py:44-45 / :96-97: r * min_iters .. r * max_iters - r target frames."""
    return reduction_factor * min_iters, reduction_factor * max_iters - reduction_factor


def filter_items(items, min_n_frame, max_n_frame, min_tokens):
    """get_path_dict's filter (:47-48) over (path, n_frame, n_token) triples: frames within the limits and AT LEAST min_tokens tokens
    (the per-example filter of _get_next_example asks for MORE than min_tokens, :273 -- both kept as they are).  The reference's
    blacklist for the 'son' / 'yuinna' directories (:50-53) keeps an item if ANY of three substrings is absent from its path, which
    every path satisfies: a no-op, not reproduced.  Order: the reference collects the triples with Pool.imap_unordered (utils
    parallel_run), so the order of its filtered list -- and with it the train / test split -- is not deterministic; here the input
    order is kept."""
    return [p for p, n, nt in items if min_n_frame <= n <= max_n_frame and nt >= min_tokens]


def split_paths(paths, data_type, n_test):
    """datafeeder.py:66-71: the last n_test (= batch_size) paths of a directory are its test set."""
    if data_type == "train":
        return paths[:-n_test]
    if data_type == "test":
        return paths[-n_test:]
    raise Exception(" [!] Unkown data_type: {}".format(data_type))


def data_ratios(data_dirs, main_data=("",), main_data_greedy_factor=0):
    """DataFeeder.__init__ (:104-121): weight 1 per directory, + main_data_greedy_factor for every entry of hparams.main_data that
    occurs in the directory's name, normalised -- the draw ratios of a group once step >= initial_phase_step (:216-222)."""
    weight = {d: 1.0 for d in data_dirs}
    if main_data_greedy_factor > 0 and any(md in d for d in data_dirs for md in main_data):
        for md in main_data:
            for d in data_dirs:
                if md in d:
                    weight[d] += main_data_greedy_factor
    z = sum(weight.values())
    return {d: w / z for d, w in weight.items()}


class NpzSource(object):
    """Callable example source over the `.npz` files of one data directory, for GroupFeeder.

    The draw sequence of DataFeeder._get_next_example (datafeeder.py:245-287): the cursor starts at the THIRD path
    (`defaultdict(lambda: 2)`, :88); at the end of the list it wraps to 0 and, for training data, reshuffles the list with the
    FEEDER's generator (pass the GroupFeeder's `rng`); a path that no longer exists is skipped; with skip_path_filter (train.py:291,
    the lists were NOT pre-filtered) an example is taken only if min_n_frame <= frames <= max_n_frame and len(tokens) > min_tokens,
    without it every loadable file is taken.  `loss_coeff` defaults to 1 (:279-282).  One deliberate difference: a file that fails
    to load is skipped, not deleted (the reference calls remove_file on it, :267)."""

    def __init__(self, paths, speaker_id, rng, training=True, skip_path_filter=False, min_n_frame=0, max_n_frame=1 << 30, min_tokens=0):
        self.paths, self.speaker_id, self.rng, self.training = list(paths), speaker_id, rng, training
        self.skip_path_filter, self.min_n_frame, self.max_n_frame, self.min_tokens = skip_path_filter, min_n_frame, max_n_frame, min_tokens
        self.offset = 2
        self.skipped = []

    def __call__(self):
        while True:
            if self.offset >= len(self.paths):
                self.offset = 0
                if self.training:
                    self.rng.shuffle(self.paths)
            path = self.paths[self.offset]
            self.offset += 1
            if not os.path.exists(path):
                continue
            try:
                data = np.load(path)
                tokens, mel, linear = data["tokens"], data["mel"], data["linear"]
            except Exception:
                self.skipped.append(path)
                continue
            if not self.skip_path_filter:
                break
            if self.min_n_frame <= linear.shape[0] <= self.max_n_frame and len(tokens) > self.min_tokens:
                break
        coeff = data["loss_coeff"] if "loss_coeff" in data else 1
        return Example(tokens, coeff, mel, linear, self.speaker_id)


def open_data_dirs(data_dirs, batch_size, hparams, data_type="train", batches_per_group=32, seed=123, skip_path_filter=False, step=0,
                   corpus=None, collate_fn=None):
    """A GroupFeeder over the reference's data directories, wired the way DataFeeder.__init__ wires itself (datafeeder.py:78-121): one
    generator (config.random_seed) shuffles every directory's path list once (training data), filters it by frames / tokens unless
    skip_path_filter, keeps all but the last `batch_size` paths for training (those are the test set), and is then shared by the example
    sources (reshuffles) and the batcher (bucketing); speaker id = position of the directory; the two draw phases of GroupFeeder from
    hparams.initial_phase_step / initial_data_greedy / main_data / main_data_greedy_factor.

    corpus: a DeviceCorpus that holds these directories' files (DeviceCorpus.from_data_dirs).  The wiring is the same, but the sources
    draw `Ref`s out of the corpus instead of loading files (frame / token counts come from its tables) and the batches are collated on
    the device: for the same directories and seed the feeder hands out the same examples in the same rows of the same batches, as a
    `Batch` of device tensors.  collate_fn overrides what a batch of Refs becomes (tests record the indices with it)."""
    import glob
    g = lambda k, d: getattr(hparams, k, d)
    r = hparams.reduction_factor
    lo, hi = frame_limits(r, g("min_iters", 30), hparams.max_iters)
    rng = np.random.RandomState(seed)
    sources = {}
    for idx, d in enumerate(data_dirs):
        paths = glob.glob("{}/*.npz".format(d))
        if data_type == "train":
            rng.shuffle(paths)
        if not skip_path_filter:
            items = []
            for p in paths:
                if corpus is not None:
                    ref = corpus.ref_of(p)
                    items.append((p, ref.n_frames, ref.n_tokens))
                    continue
                z = np.load(p)
                items.append((p, z["linear"].shape[0], len(z["tokens"])))
            paths = filter_items(items, lo, hi, g("min_tokens", 50))
        paths = split_paths(paths, data_type, batch_size)
        make = NpzSource if corpus is None else corpus.source
        sources[d] = make(paths, idx if len(data_dirs) > 1 else None, rng, data_type == "train", skip_path_filter, lo, hi, g("min_tokens", 50))
    ratios = data_ratios(list(data_dirs), g("main_data", [""]), g("main_data_greedy_factor", 0))
    extra = {}
    if corpus is not None:
        extra = dict(collate_fn=corpus.collate_refs if collate_fn is None else collate_fn, length=lambda ref: ref.n_frames)
    elif collate_fn is not None:
        extra = dict(collate_fn=collate_fn)
    f = GroupFeeder(sources, batch_size, r, batches_per_group, ratios, seed, training=data_type == "train",
                    initial_phase_step=g("initial_phase_step", 8000), initial_data_greedy=g("initial_data_greedy", True), step=step, **extra)
    f.rng = rng
    return f


# ---- the same examples held on the device, collated by one kernel launch (taco_collate, csrc/taco_feed.h) ----
Ref = collections.namedtuple("Ref", "index n_tokens n_frames speaker_id")

_AUDIO_KEYS = ("num_mels", "num_freq", "sample_rate", "frame_length_ms", "frame_shift_ms", "preemphasis", "min_level_db", "ref_level_db",
               "power", "griffin_lim_iters")


def hop_length(hparams):
    """Samples per frame shift, with taco_gl_create's arithmetic (frame_shift_ms is a C float there)."""
    return int(float(np.float32(getattr(hparams, "frame_shift_ms", 12.5))) / 1000.0 * int(getattr(hparams, "sample_rate", 24000)))


def waveform_length(t_out, hop):
    """Samples per row of the waveform rectangle whose spectrogram has exactly t_out frames: (t_out - 1) * hop, the largest multiple
    of hop with 1 + Lmax // hop == t_out.  t_out = padded_length(longest frames, r) > longest frames = 1 + longest // hop, so
    Lmax >= (1 + longest // hop) * hop > longest > n_fft / 2 for every waveform a corpus accepts."""
    return (int(t_out) - 1) * int(hop)


def collate_streams(device, streams, index, n_rows, n_items):
    """ONE taco_collate launch on the device's current stream: row i of every stream's `out` (and entry i of its `counts`) is item
    index[i] (device int32 [n_rows]) of the n_items its `pack` holds.  A stream is a dict of TacoCollateStream's fields (include/taco_abi.h):
    pack, start, rows, out, counts are device tensors or None, width and rows_out ints."""
    arr = (_lib.TacoCollateStream * len(streams))()
    for a, d in zip(arr, streams):
        a.pack, a.start, a.rows, a.out, a.counts = (pointer(d[k]) for k in ("pack", "start", "rows", "out", "counts"))
        a.width, a.rows_out = d["width"], d["rows_out"]
    call(device, _lib.load_library().taco_collate, STREAM, arr, len(streams), index, n_rows, n_items)


class RefSource(object):
    """NpzSource's draw sequence over the Refs of a DeviceCorpus: the cursor starts at the third item, wraps to 0 and -- for training
    data -- reshuffles the list with the shared generator (the same number of draws as shuffling the path list); an item the corpus
    does not hold is skipped like a file that does not exist; with skip_path_filter a Ref is taken only if
    min_n_frame <= frames <= max_n_frame and tokens > min_tokens.  Items are paths (of DeviceCorpus.from_npz) or corpus indices."""

    def __init__(self, corpus, items, speaker_id, rng, training=True, skip_path_filter=False, min_n_frame=0, max_n_frame=1 << 30, min_tokens=0):
        self.corpus, self.paths, self.speaker_id, self.rng, self.training = corpus, list(items), speaker_id, rng, training
        self.skip_path_filter, self.min_n_frame, self.max_n_frame, self.min_tokens = skip_path_filter, min_n_frame, max_n_frame, min_tokens
        self.offset = 2
        self.skipped = []

    def __call__(self):
        while True:
            if self.offset >= len(self.paths):
                self.offset = 0
                if self.training:
                    self.rng.shuffle(self.paths)
            item = self.paths[self.offset]
            self.offset += 1
            try:
                ref = self.corpus.ref_of(item)
            except KeyError:
                self.skipped.append(item)
                continue
            if ref.speaker_id != self.speaker_id:
                raise Exception("corpus item %r was stored with speaker_id %r, the source draws for %r" % (item, ref.speaker_id, self.speaker_id))
            if not self.skip_path_filter:
                return ref
            if self.min_n_frame <= ref.n_frames <= self.max_n_frame and ref.n_tokens > self.min_tokens:
                return ref


class _AudioParams(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


class DeviceCorpus(object):
    """A training corpus that stays on the device.

    kind "targets": mel [T, num_mels] and linear [T, num_freq] exactly as the `.npz` files hold them; `collate` is ONE taco_collate
    launch that gathers tokens, mel, linear, loss_coeff and speaker_id into the padded rectangles of the host `collate`.
    kind "waveform": float32 samples; `collate` gathers tokens, samples, loss_coeff and speaker_id, the samples into [B, Lmax] with
    Lmax = waveform_length(T_out, hop), and Spectrogram.targets turns that buffer and the counts into both targets -- which then ARE
    the [B, T_out, .] rectangles (1 + Lmax // hop == T_out), with exact zeros past each row's frames.

    add(...) collects examples on the host, finalize() packs them end to end (item starts padded to `item_align` words) and uploads
    them once.  The host keeps the small tables: refs() is all the draw logic needs."""

    def __init__(self, hparams, device="cuda:0", kind="targets", item_align=1):
        if kind not in ("targets", "waveform"):
            raise Exception("kind must be 'targets' or 'waveform', got %r" % (kind,))
        self.hp, self.device, self.kind, self.item_align = hparams, device, kind, max(1, int(item_align))
        self.num_mels, self.num_freq = int(hparams.num_mels), int(hparams.num_freq)
        self.hop, self.n_fft = hop_length(hparams), (int(hparams.num_freq) - 1) * 2
        self._items = []            # (tokens, coeff, a, b) with a, b = mel, linear or wav, None -- until finalize()
        self._n_tokens, self._n_frames, self._speaker, self._n_samples = [], [], [], []
        self._path_index = {}
        self._packs = None          # name -> host array (after load) or device tensor (after finalize)
        self._on_device = False
        self._spec = None
        self._scratch = {}

    def __len__(self):
        return len(self._n_tokens)

    # ---- filling ----
    def add(self, tokens, loss_coeff=1, mel=None, linear=None, wav=None, speaker_id=None, path=None):
        if self._packs is not None:
            raise Exception("the corpus is finalized: examples can no longer be added")
        tokens = np.ascontiguousarray(np.asarray(tokens), dtype=np.int32).reshape(-1)
        if len(self) and (speaker_id is None) != (self._speaker[0] is None):
            raise Exception("either every example of a corpus has a speaker_id or none has")
        if self.kind == "targets":
            if mel is None or linear is None or wav is not None:
                raise Exception("a 'targets' corpus takes mel and linear (and no wav)")
            a = np.ascontiguousarray(np.asarray(mel), dtype=np.float32)
            b = np.ascontiguousarray(np.asarray(linear), dtype=np.float32)
            if a.ndim != 2 or b.ndim != 2 or a.shape[1] != self.num_mels or b.shape[1] != self.num_freq or a.shape[0] != b.shape[0]:
                raise Exception("mel must be [T, %d] and linear [T, %d], got %s and %s" % (self.num_mels, self.num_freq, a.shape, b.shape))
            frames = a.shape[0]
        else:
            if wav is None or mel is not None or linear is not None:
                raise Exception("a 'waveform' corpus takes wav (and no mel / linear)")
            a, b = np.ascontiguousarray(np.asarray(wav), dtype=np.float32).reshape(-1), None
            if len(a) <= self.n_fft // 2:
                raise Exception("a waveform of %d samples is too short: reflect padding needs more than n_fft/2 = %d (such a row would "
                                "be clamped by taco_spec_targets)" % (len(a), self.n_fft // 2))
            from . import audio
            frames = audio.num_frames(self.hp, len(a))
        if path is not None:
            self._path_index[str(path)] = len(self)
        self._items.append((tokens, np.float32(loss_coeff), a, b))
        self._n_tokens.append(len(tokens))
        self._n_frames.append(int(frames))
        self._n_samples.append(a.size if self.kind == "waveform" else 0)
        self._speaker.append(None if speaker_id is None else int(speaker_id))
        return len(self) - 1

    @classmethod
    def from_npz(cls, paths, hparams, device="cuda:0", speaker_id=None, finalize=True, **kw):
        """A 'targets' corpus of the reference's `.npz` examples; every file is read once.  speaker_id: None, one id, or one per path."""
        c = cls(hparams, device, "targets", **kw)
        paths = list(paths)
        ids = speaker_id if isinstance(speaker_id, (list, tuple, np.ndarray)) else [speaker_id] * len(paths)
        for p, sid in zip(paths, ids):
            z = np.load(p)
            c.add(z["tokens"], z["loss_coeff"] if "loss_coeff" in z else 1, z["mel"], z["linear"], speaker_id=sid, path=p)
        return c.finalize() if finalize else c

    @classmethod
    def from_data_dirs(cls, data_dirs, hparams, device="cuda:0", finalize=True, **kw):
        """Every `*.npz` of the reference's data directories, speaker id = position of the directory (none for a single directory):
        the corpus `open_data_dirs(data_dirs, ..., corpus=...)` feeds from."""
        import glob
        paths, ids = [], []
        for idx, d in enumerate(data_dirs):
            ps = sorted(glob.glob("{}/*.npz".format(d)))
            paths += ps
            ids += [idx if len(data_dirs) > 1 else None] * len(ps)
        return cls.from_npz(paths, hparams, device, speaker_id=ids, finalize=finalize, **kw)

    def _pack(self, arrays, dtype):
        """arrays laid end to end, each start rounded up to item_align words -> (pack, start [N] int64); slack is zero."""
        al = self.item_align
        sizes = np.array([a.size for a in arrays], np.int64)
        padded = -(-sizes // al) * al
        start = np.concatenate([[0], np.cumsum(padded)[:-1]]).astype(np.int64) if len(arrays) else np.zeros(0, np.int64)
        total = int(start[-1] + sizes[-1]) if len(arrays) else 0
        pack = np.zeros(max(total, 1), dtype)
        for a, s0 in zip(arrays, start):
            pack[s0:s0 + a.size] = a.reshape(-1)
        return pack, start

    def _build_packs(self):
        if not len(self):
            raise Exception("the corpus is empty")
        its = self._items
        p = {}
        p["tok_pack"], p["tok_start"] = self._pack([t[0] for t in its], np.int32)
        p["tok_rows"] = np.asarray(self._n_tokens, np.int32)
        p["coeff"] = np.asarray([t[1] for t in its], np.float32)
        if self._speaker[0] is not None:
            p["speaker"] = np.asarray(self._speaker, np.int32)
        p["frames"] = np.asarray(self._n_frames, np.int32)
        if self.kind == "targets":
            p["mel_pack"], p["mel_start"] = self._pack([t[2] for t in its], np.float32)
            p["lin_pack"], p["lin_start"] = self._pack([t[3] for t in its], np.float32)
        else:
            p["wav_pack"], p["wav_start"] = self._pack([t[2] for t in its], np.float32)
            p["wav_rows"] = np.asarray([t[2].size for t in its], np.int32)
        return p

    def finalize(self):
        """Pack the examples and upload them once.  Raises when the corpus does not fit the device's free memory."""
        if self._on_device:
            return self
        if self._packs is None:
            self._packs = self._build_packs()
        self._items = None
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise Exception("DeviceCorpus lives on a GPU (got %s); the host path is NpzSource / collate" % (self.device,))
        need = sum(int(a.nbytes) for a in self._packs.values())
        free, _total = torch.cuda.mem_get_info(dev)
        if need > free:
            raise Exception("DeviceCorpus needs %d bytes on %s and only %d are free" % (need, dev, free))
        for k in list(self._packs):
            self._packs[k] = torch.from_numpy(self._packs[k]).to(dev)
        self._dev, self._on_device = dev, True
        if self.kind == "waveform":
            from . import audio
            self._spec = audio.Spectrogram(self.hp, str(dev))
        return self

    @property
    def nbytes(self):
        """Bytes of the packs and tables (on the device once finalized)."""
        packs = self._packs if self._packs is not None else self._build_packs()
        return sum(int(a.nbytes) if isinstance(a, np.ndarray) else a.numel() * a.element_size() for a in packs.values())

    # ---- what the host draws from ----
    def refs(self):
        return [Ref(i, self._n_tokens[i], self._n_frames[i], self._speaker[i]) for i in range(len(self))]

    def ref_of(self, item):
        """Ref of a corpus index or of a path the corpus was filled from (KeyError if it holds neither)."""
        if isinstance(item, (int, np.integer)):
            i = int(item)
            if not 0 <= i < len(self):
                raise KeyError(item)
        else:
            i = self._path_index[str(item)]
        return Ref(i, self._n_tokens[i], self._n_frames[i], self._speaker[i])

    def source(self, paths_or_indices, speaker_id, rng, training=True, skip_path_filter=False, min_n_frame=0, max_n_frame=1 << 30, min_tokens=0):
        return RefSource(self, paths_or_indices, speaker_id, rng, training, skip_path_filter, min_n_frame, max_n_frame, min_tokens)

    # ---- batches ----
    def _buffer(self, name, shape, dtype):
        """Grow-only scratch of the corpus (index upload, waveform rectangle, counts): no allocation once a shape has been seen."""
        n = int(np.prod(shape))
        t = self._scratch.get(name)
        if t is None or t.numel() < n:
            t = self._scratch[name] = torch.empty(n, dtype=dtype, device=self._dev)
        return t[:n].view(*shape)

    def collate(self, indices, reduction_factor, out=None):
        """A `Batch` of device tensors with the shapes, dtypes and bits of the host collate on the same examples.  indices: host data
        (uploaded, 4 * B bytes) or a device int32 tensor, which the host cannot see: the shapes then come from `out` or, without it,
        from the corpus-wide maxima, and an index outside the corpus gives an all-zero row.  out: a Batch of preallocated contiguous
        tensors of the right shapes, written in place (nothing is allocated)."""
        if not self._on_device:
            raise Exception("call finalize() first")
        r, p = int(reduction_factor), self._packs
        if torch.is_tensor(indices) and indices.is_cuda:
            idx = indices
            if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.dim() != 1:
                raise Exception("a device index must be a contiguous int32 vector")
            if out is not None:
                t_in, t_out = int(out.inputs.shape[1]), int(out.mel_targets.shape[1])
            else:
                t_in, t_out = max(self._n_tokens), padded_length(max(self._n_frames), r)
            longest = None
        else:
            ih = np.asarray(indices, np.int64).reshape(-1)
            if not len(ih) or ih.min() < 0 or ih.max() >= len(self):
                raise IndexError("indices must be a non-empty list within [0, %d)" % len(self))
            t_in = int(max(self._n_tokens[i] for i in ih))
            t_out = padded_length(int(max(self._n_frames[i] for i in ih)), r)
            idx = self._buffer("index", (len(ih),), torch.int32)
            idx.copy_(torch.from_numpy(ih.astype(np.int32)))
            longest = ih
        B = int(idx.numel())
        if B < 1 or t_out % r:
            raise Exception("bad batch: %d rows, T_out %d for reduction factor %d" % (B, t_out, r))
        spk = "speaker" in p
        shapes = [("inputs", (B, t_in), torch.int32), ("input_lengths", (B,), torch.int32), ("loss_coeff", (B,), torch.float32),
                  ("mel_targets", (B, t_out, self.num_mels), torch.float32), ("linear_targets", (B, t_out, self.num_freq), torch.float32)]
        if spk:
            shapes.append(("speaker_id", (B,), torch.int32))
        if out is None:
            f = {k: torch.empty(s, dtype=dt, device=self._dev) for k, s, dt in shapes}
            out = Batch(f["inputs"], f["input_lengths"], f["loss_coeff"], f["mel_targets"], f["linear_targets"], f.get("speaker_id"))
        else:
            for k, s, dt in shapes:
                t = getattr(out, k)
                if not (torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == s and t.dtype == dt and t.is_contiguous()):
                    raise Exception("out.%s must be a contiguous %s device tensor of shape %s" % (k, dt, s))
        st = [dict(pack=p["tok_pack"], start=p["tok_start"], rows=p["tok_rows"], width=1, rows_out=t_in, out=out.inputs, counts=out.input_lengths),
              dict(pack=p["coeff"], start=None, rows=None, width=1, rows_out=1, out=out.loss_coeff, counts=None)]
        if spk:
            st.append(dict(pack=p["speaker"], start=None, rows=None, width=1, rows_out=1, out=out.speaker_id, counts=None))
        if self.kind == "targets":
            st.append(dict(pack=p["mel_pack"], start=p["mel_start"], rows=p["frames"], width=self.num_mels, rows_out=t_out, out=out.mel_targets, counts=None))
            st.append(dict(pack=p["lin_pack"], start=p["lin_start"], rows=p["frames"], width=self.num_freq, rows_out=t_out, out=out.linear_targets, counts=None))
        else:
            lmax = waveform_length(t_out, self.hop)
            # the identity that makes the spectrogram's outputs the training rectangles themselves: no second copy
            assert 1 + lmax // self.hop == t_out and lmax > self.n_fft // 2, (lmax, self.hop, t_out, self.n_fft)
            assert longest is None or lmax > max(self._n_samples[i] for i in longest), (lmax, t_out)
            wav = self._buffer("wav", (B, lmax), torch.float32)
            ns = self._buffer("num_samples", (B,), torch.int32)
            st.append(dict(pack=p["wav_pack"], start=p["wav_start"], rows=p["wav_rows"], width=1, rows_out=lmax, out=wav, counts=ns))
        collate_streams(self._dev, st, idx, B, len(self))
        if self.kind == "waveform":
            nf = self._buffer("num_frames", (B,), torch.int32)
            self._spec.targets(wav, ns, out=(out.linear_targets, out.mel_targets, nf))
        return out

    def collate_refs(self, refs, reduction_factor):
        """GroupFeeder's collate_fn: one bucketed batch of Refs -> a device Batch."""
        return self.collate([ref.index for ref in refs], reduction_factor)

    # ---- one file instead of ten thousand ----
    def save(self, path):
        """The host packs and tables as one `.npz` (read back from the device when the corpus is finalized)."""
        import json
        packs = self._packs if self._packs is not None else self._build_packs()
        host = {k: (a if isinstance(a, np.ndarray) else a.cpu().numpy()) for k, a in packs.items()}
        meta = dict(kind=self.kind, item_align=self.item_align, audio={k: getattr(self.hp, k) for k in _AUDIO_KEYS if hasattr(self.hp, k)},
                    paths=sorted(self._path_index, key=self._path_index.get), path_index=sorted(self._path_index.values()))
        with open(path, "wb") as fh:
            np.savez(fh, meta=np.array(json.dumps(meta)), **host)

    @classmethod
    def load(cls, path, device="cuda:0", hparams=None):
        """A corpus written by save(); uploaded to `device` (None: kept on the host, for refs() and the draw logic only).  hparams
        default to the audio parameters recorded in the file."""
        import json
        z = np.load(path)
        meta = json.loads(str(z["meta"]))
        c = cls(hparams if hparams is not None else _AudioParams(**meta["audio"]), device, meta["kind"], item_align=meta["item_align"])
        c._packs = {k: z[k] for k in z.files if k != "meta"}
        c._items = None
        c._n_tokens = [int(v) for v in c._packs["tok_rows"]]
        c._n_frames = [int(v) for v in c._packs["frames"]]
        c._speaker = [int(v) for v in c._packs["speaker"]] if "speaker" in c._packs else [None] * len(c._n_tokens)
        c._n_samples = [int(v) for v in c._packs["wav_rows"]] if "wav_rows" in c._packs else [0] * len(c._n_tokens)
        c._path_index = dict(zip(meta["paths"], meta["path_index"]))
        return c.finalize() if device is not None else c
