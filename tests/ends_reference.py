"""The two ENDS of the training step on the CPU, float64 and float32, with reverse-mode autograd -- the yardstick of the block tests
(tests/test_ends_reference_host.py, tests/test_gpu_ends_train.py).  No GPU, no library: tests/torch_formulation.py::dense / add_loss only.

  front   embedding gather -> encoder prenet (-> pre), the speaker rows of 'simple' (-> spk_emb), the speaker vectors of deepvoice (-> vec/...).
          The upstream gradients dpre, dvec_i, dspk_emb are inputs, so the loss  sum(pre * dpre) + sum_i sum(vec_i * dvec_i) [+ sum(spk_emb *
          dspk_emb)]  has no kink of its own; what kinks remain (the prenet's ReLUs) are kept at a distance by the choice of the seed.
  head    teacher-frame gather, linear head (the speaker rows of 'simple' in front of the kernel), add_loss with loss_coeff and the priority
          band, and their backward: dmel (+ dmel_post, the post CBHG's share, an input), dpost, d(speaker rows), linear/kernel, linear/bias.
          The L1 kinks are kept away by CONSTRUCTION, not by seed: tgt = out64 + s * u with s = +-1 and u ~ U[0.25, 1], out64 the float64
          head output (and the given mel), so every |out - tgt| >= 0.25 -- a condition the host test asserts, not a tolerance.

  error bar of tensor k      bar_k = max(max|g32_k - g64_k|, 2^-20 * s_k),  s_k = max|g64_k|
                             (the float32 restatement's own error; the floor is 8 fp32 ulps of the largest element)
  structural zero            an embedding row whose symbol is absent from the batch, a row of speaker_embedding / of the spk tables whose
                             speaker the batch does not use: zero by construction.  They lie inside tensors whose other rows set s_k, so
                             they take that scale (the tensor's own, of its present rows); Reference.zero_rows names them and the GPU test
                             asserts that they come back as exact zeros.  No whole tensor of these scopes is a structural zero.
  kink condition (front)     with delta = 32 * max|z32 - z64| of a pre-activation tensor z: every prenet ReLU pre-activation has
                             |z64| > delta.  A seed is admissible when all of them hold; find_seed() returns the first admissible seed from a
                             base, and FRONT_CASES pins what it returned.  (A reference-width layer of 130 rows has 33280 pre-activations:
                             fewer seeds keep all of them away than at the tiny widths, hence pins other than 3.)
  flip-free (head)           min|out64 - tgt| >= 0.25 and > 1000 * max|lin32 - lin64| (Reference.kinks holds both)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import taco_oracle as O
import torch_formulation as TF
from cbhg_reference import COMMON_MARGIN, FLOOR, KINK_FACTOR, compare, ratios          # the comparator is the CBHG block test's
from util import tiny_hp

__all__ = ["COMMON_MARGIN", "FLOOR", "KINK_FACTOR", "compare", "ratios"]

# taco_train_debug_front's `paths` word (include/taco_debug.h)
P_EMBED_DET, P_EMBED_ATOMIC, P_SPK_TABLES, P_SPK_DENSE = 1 << 0, 1 << 1, 1 << 2, 1 << 3

L1_GAP = 0.25                 # every |out64 - tgt| of the head cases is at least this
L1_GAP_OVER_ERROR = 1000.0    # ... and this many times the float32 head's own error


class Case(object):
    """One row of a table.  kind 'front': T = T_in; 'head': T = T_out.  speakers > 1: a multi-speaker model (hp.model_type says which).
    front: atomic = the k_embed_bwd arm (taco_train_set_deterministic(False)), held to the bars only.
    head: coeff = a loss_coeff of U[0.5, 1.5] (else none); prioritize / sample_rate: the priority band; dmel_post: with the post CBHG's share.
    margins: tensors with a stated margin of their own over the common one, {name: (margin, reason)}."""

    def __init__(self, kind, name, hp, B, T, seed, speakers=1, atomic=False, coeff=False, prioritize=False, sample_rate=24000, dmel_post=False,
                 margins=None):
        self.kind, self.name, self.hp_fn, self.B, self.T, self.seed, self.speakers = kind, name, hp, B, T, seed, speakers
        self.atomic, self.coeff, self.prioritize, self.sample_rate, self.dmel_post = atomic, coeff, prioritize, sample_rate, dmel_post
        self.margins = margins or {}
        self.id = "%s-B%d-T%d" % (name, B, T)

    def hp(self):
        return self.hp_fn()

    @property
    def paths(self):
        hp = self.hp()
        word = P_EMBED_ATOMIC if self.atomic else P_EMBED_DET
        if self.speakers > 1 and hp.model_type == "deepvoice":
            word |= P_SPK_TABLES if hp.speaker_embedding_size == 1 else P_SPK_DENSE
        return word


def _tiny(**kw):
    return lambda: tiny_hp(**kw)


def _ref(**kw):
    return lambda: O.OracleHParams(**kw)


# seeds: find_seed(case, base=3), printed by `python tests/ends_reference.py` -- see
# tests/test_ends_reference_host.py::test_every_front_case_is_admissible_at_its_pinned_seed
FRONT_CASES = [
    # ---- tiny widths: E = 32, less than the 64 columns of one wave of k_embed_bwd_det ----
    Case("front", "tiny", _tiny(), 3, 9, 3),                                                    # 27 rows: less than one 64-id ballot block
    Case("front", "tiny_odd", _tiny(enc_prenet_sizes=[32, 18], enc_proj_sizes=[14, 18]), 5, 13, 3),                      # 65 rows: a block and a one-row tail; odd prenet widths
    Case("front", "tiny_atomic", _tiny(), 5, 13, 3, atomic=True),                               # k_embed_bwd
    Case("front", "tiny", _tiny(), 2, 64, 3),                                                   # 128 rows, no tail; batch row 0 is ONE id: all 64 ballot bits
    Case("front", "tiny_deepvoice", _tiny(model_type="deepvoice"), 3, 9, 3, speakers=3),        # S = 4
    Case("front", "tiny_deepvoice_s1", _tiny(model_type="deepvoice", speaker_embedding_size=1), 3, 9, 3, speakers=3),      # the tables path
    Case("front", "tiny_simple", _tiny(model_type="simple"), 3, 9, 3, speakers=3),
    # ---- reference widths: E = 256, four column blocks per table row; prenet 256 -> 128 ----
    Case("front", "reference", _ref(), 5, 13, 7),                                               # 65 rows
    Case("front", "reference", _ref(), 2, 64, 3),                                               # 128 rows; batch row 0 is ONE id
    Case("front", "reference_deepvoice", _ref(model_type="deepvoice"), 17, 7, 15, speakers=3),   # S = 16, 119 rows
    Case("front", "reference_simple", _ref(model_type="simple"), 10, 13, 10, speakers=3),        # 130 rows
]

HEAD_CASES = [
    # ---- tiny widths: F = 36, 64 inputs, r = 3 ----
    Case("head", "tiny", _tiny(), 2, 6, 3),                                                                              # 12 rows
    Case("head", "tiny_band24k", _tiny(), 2, 6, 4, coeff=True, prioritize=True, dmel_post=True),                          # band 0..15
    Case("head", "tiny_band8k", _tiny(), 2, 6, 5, coeff=True, prioritize=True, sample_rate=8000),                         # band 1..45, clamped to 36
    Case("head", "tiny_r1", _tiny(reduction_factor=1), 3, 5, 6, coeff=True, dmel_post=True),
    Case("head", "tiny_simple", _tiny(model_type="simple"), 3, 6, 7, speakers=2, coeff=True, prioritize=True, dmel_post=True),
    # ---- reference widths: F = 1025, 512 inputs, r = 5 ----
    Case("head", "reference", _ref(reduction_factor=5), 2, 10, 8),                                                        # 20 rows
    Case("head", "reference_band24k", _ref(reduction_factor=5), 2, 10, 9, coeff=True, prioritize=True, dmel_post=True),   # band 14..427
    Case("head", "reference_band16k", _ref(reduction_factor=5), 2, 10, 10, prioritize=True, sample_rate=16000),           # band 21..640
    Case("head", "reference_band8k", _ref(reduction_factor=5), 1, 65, 11, coeff=True, prioritize=True, sample_rate=8000, dmel_post=True),   # B = 1, 65 rows; band 42..1281, clamped to 1025
    Case("head", "reference_simple", _ref(reduction_factor=5, model_type="simple"), 2, 10, 12, speakers=2, coeff=True, prioritize=True,
         sample_rate=8000),                                                                                               # S = 16 rows in front of the kernel
]
CASES = FRONT_CASES + HEAD_CASES

FRONT_SCOPES = ("embedding", "prenet/", "speaker_embedding", "spk/")
HEAD_SCOPES = ("linear/",)


def in_scope(kind, name):
    return name.startswith(FRONT_SCOPES if kind == "front" else HEAD_SCOPES)


def band(prioritize, sample_rate, num_freq):
    """[lo, hi) of the priority band as tacotron.py:283-288 slices it: a slice clamps its upper end to the axis."""
    if not prioritize:
        return 0, 0
    hi, lo = int(5000 / (sample_rate * 0.5) * num_freq), int(165 / (sample_rate * 0.5) * num_freq)
    return lo, min(hi, num_freq)


def vector_names(hp):
    return ["before_highway", "encoder_rnn_init", "attention_rnn_init"] + ["decoder_rnn_init_%d" % (i + 1) for i in range(hp.dec_layer_num)]


def vector_dims(hp):
    return [hp.enc_prenet_sizes[-1], 2 * hp.enc_rnn_size, hp.attention_state_size] + [hp.dec_rnn_size] * hp.dec_layer_num


ABSENT_SYMBOL, REPEATED_SYMBOL, UNUSED_SPEAKER = 5, 7, 1
_f32 = lambda a: np.ascontiguousarray(a, np.float32)


def make_front_inputs(hp, B, T_in, seed, speakers=1):
    """Weights of the whole model from O.init_weights(seed) and the block's data from RandomState(seed + 1).  Into the random ids, by hand:
    symbol ABSENT_SYMBOL never occurs; batch row 0 is REPEATED_SYMBOL alone; the pad id 0 fills every row beyond its length (row 1 is the
    shortest) -- dpre is NOT zero there, the reference masks nothing in the prenet; the last symbol of the table opens the last row.
    Speakers (three): UNUSED_SPEAKER never speaks, the others repeat."""
    V = hp.num_symbols
    w = O.init_weights(hp, speakers, seed)
    rs = np.random.RandomState(seed + 1)
    ids = rs.randint(1, V, size=(B, T_in)).astype(np.int32)
    ids[ids == ABSENT_SYMBOL] = ABSENT_SYMBOL + 1
    ids[0, :] = REPEATED_SYMBOL
    lengths = rs.randint(max(T_in // 2, 1), T_in + 1, size=B).astype(np.int32)
    lengths[0], lengths[1] = T_in, max(T_in // 2, 1)
    for b in range(B):
        ids[b, lengths[b]:] = 0
    ids[-1, 0] = V - 1
    d = {"w": w, "ids": ids, "lengths": lengths, "dpre": _f32(rs.randn(B, T_in, hp.enc_prenet_sizes[-1])), "speaker_id": None, "dvec": None,
         "dspk_emb": None, "speakers": speakers}
    if speakers > 1:
        assert speakers == 3
        sid = rs.choice([0, 2], size=B).astype(np.int32)
        sid[0], sid[1] = 0, 2                   # both used, whatever was drawn; with B = 3 one of them repeats
        d["speaker_id"] = sid
        if hp.model_type == "deepvoice":
            d["dvec"] = [_f32(rs.randn(B, n)) for n in vector_dims(hp)]
        else:
            d["dspk_emb"] = _f32(rs.randn(B, hp.speaker_embedding_size))
    return d


def make_head_inputs(hp, B, T_out, seed, speakers=1, coeff=False, prioritize=False, sample_rate=24000, dmel_post=False):
    """Weights from O.init_weights(seed) (linear/bias from RandomState(seed + 1): the initialiser leaves it zero); post_out, speaker rows ~ 0.5 * randn (a
    BiGRU's outputs lie in (-1, 1)), mel ~ randn; the targets sit at s * u from the float64 outputs, s = +-1, u ~ U[0.25, 1]."""
    w = dict(O.init_weights(hp, speakers, seed))
    rs = np.random.RandomState(seed + 1)
    w["linear/bias"] = _f32(0.1 * rs.randn(hp.num_freq))
    simple = speakers > 1 and hp.model_type == "simple"
    d = {"w": w, "post_out": _f32(0.5 * rs.randn(B, T_out, 2 * hp.post_rnn_size)), "mel": _f32(rs.randn(B, T_out, hp.num_mels)),
         "spk_emb": _f32(0.5 * rs.randn(B, hp.speaker_embedding_size)) if simple else None,
         "coeff": _f32(rs.uniform(0.5, 1.5, size=B)) if coeff else None, "prioritize": bool(prioritize), "sample_rate": int(sample_rate),
         "dmel_post": _f32(rs.randn(B, T_out, hp.num_mels) / (B * T_out * hp.num_mels)) if dmel_post else None}      # the size of the L1 gradient beside it
    lin64 = _head_linear(hp, d, torch.float64).detach().numpy()

    def away(out64):      # the float32 target at s * u from out64; where the rounding to float32 cut the gap below L1_GAP, the next float32 outwards
        s = rs.choice([-1.0, 1.0], size=out64.shape)
        tgt = _f32(out64 + s * rs.uniform(L1_GAP, 1.0, size=out64.shape))
        short = np.abs(tgt.astype(np.float64) - out64) < L1_GAP
        tgt[short] = np.nextafter(tgt[short], _f32(s[short] * np.inf))
        return tgt

    d["lin_tgt"] = away(lin64)
    d["mel_tgt"] = away(d["mel"].astype(np.float64))
    return d


def _leaf(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)


def _const(a, dtype):
    return None if a is None else torch.tensor(np.asarray(a), dtype=dtype)


class _Recorder(object):
    """Stands in for torch.nn.functional: records every ReLU input and passes everything through."""

    def __init__(self):
        self.relu_in = []

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, y):
        self.relu_in.append(y)
        return F.relu(y)


def _run(dtype, fn):
    """fn() with torch_formulation at `dtype`, on one thread (one summation order for the float32 run, whatever the host)."""
    old_dt, old_nt = TF.DT, torch.get_num_threads()
    TF.DT = dtype
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        TF.DT = old_dt
        torch.set_num_threads(old_nt)


_f64 = lambda t: t.detach().numpy().astype(np.float64)
_grad = lambda t: _f64(t.grad) if t.grad is not None else np.zeros(tuple(t.shape))


def evaluate_front(hp, inp, dtype):
    """(tensors, relu): tensors = pre [B, T_in, P], vec/<name> (deepvoice), spk_emb (simple, and deepvoice with S > 1) and every parameter
    gradient of embedding, prenet/..., speaker_embedding, spk/... by its name; relu = the prenet's ReLU pre-activations.  All float64 NumPy."""
    def fn():
        rec = _Recorder()
        w = {k: _leaf(v, dtype) for k, v in inp["w"].items() if in_scope("front", k)}
        ids = torch.as_tensor(np.asarray(inp["ids"]), dtype=torch.long)
        x = w["embedding"][ids]
        for i in range(len(hp.enc_prenet_sizes)):
            x = rec.relu(TF.dense(x, w, "prenet/dense_%d" % (i + 1)))
        loss = (x * _const(inp["dpre"], dtype)).sum()
        out = {"pre": x}
        if inp["speakers"] > 1:
            sid = torch.as_tensor(np.asarray(inp["speaker_id"]), dtype=torch.long)
            spk = w["speaker_embedding"][sid] if hp.speaker_embedding_size != 1 else None
            if spk is not None:
                out["spk_emb"] = spk
            if hp.model_type == "deepvoice":
                for nm, dv in zip(vector_names(hp), inp["dvec"]):
                    v = w["spk/%s/table" % nm][sid] if spk is None else F.softsign(TF.dense(spk, w, "spk/" + nm))
                    out["vec/" + nm] = v
                    loss = loss + (v * _const(dv, dtype)).sum()
            else:
                loss = loss + (spk * _const(inp["dspk_emb"], dtype)).sum()
        loss.backward()
        res = {k: _f64(v) for k, v in out.items()}
        res.update({k: _grad(t) for k, t in w.items()})
        return res, [_f64(z) for z in rec.relu_in]
    return _run(dtype, fn)


def _head_linear(hp, inp, dtype, w=None, post=None, spk=None):
    def fn():
        ww = w if w is not None else {k: _const(v, dtype) for k, v in inp["w"].items() if in_scope("head", k)}
        p = post if post is not None else _const(inp["post_out"], dtype)
        s = spk if spk is not None else _const(inp["spk_emb"], dtype)
        if s is not None:      # linear(concat(tiled speaker rows, post)) (tacotron.py:226-235)
            p = torch.cat([s[:, None].expand(p.shape[0], p.shape[1], s.shape[1]), p], -1)
        return TF.dense(p, ww, "linear")
    return _run(dtype, fn) if w is None else fn()


def evaluate_head(hp, inp, dtype):
    """tensors = teacher [B, T_out / r, num_mels], lin [B, T_out, F], losses [4] (loss, mel_loss, linear_loss, loss_without_coeff), dmel (with
    dmel_post added where given), dpost, dspk (simple) and the gradients of linear/kernel, linear/bias.  All float64 NumPy."""
    def fn():
        w = {k: _leaf(v, dtype) for k, v in inp["w"].items() if in_scope("head", k)}
        post, mel, spk = _leaf(inp["post_out"], dtype), _leaf(inp["mel"], dtype), _leaf(inp["spk_emb"], dtype)
        mt, lt = _const(inp["mel_tgt"], dtype), _const(inp["lin_tgt"], dtype)
        B = mt.shape[0]
        ones = torch.ones(B, dtype=dtype)
        co = ones if inp["coeff"] is None else _const(inp["coeff"], dtype)
        lin = _head_linear(hp, inp, dtype, w, post, spk)
        pr, sr = inp["prioritize"], inp["sample_rate"]
        loss = TF.add_loss(mel, mt, lin, lt, co, pr, sr)
        total = loss if inp["dmel_post"] is None else loss + (mel * _const(inp["dmel_post"], dtype)).sum()
        total.backward()
        with torch.no_grad():      # the other three fetches of tacotron.py:297-302, through the same function
            without = TF.add_loss(mel, mt, lin, lt, ones, pr, sr)
            linear_loss = TF.add_loss(mel, mel, lin, lt, ones, pr, sr)
            mel_loss = TF.add_loss(mel, mt, lin, lin, ones, False, sr)
        r = hp.reduction_factor
        res = {"teacher": np.asarray(inp["mel_tgt"], np.float64)[:, r - 1::r], "lin": _f64(lin),
               "losses": np.array([float(v.detach()) for v in (loss, mel_loss, linear_loss, without)]), "dmel": _grad(mel), "dpost": _grad(post)}
        if spk is not None:
            res["dspk"] = _grad(spk)
        res.update({k: _grad(t) for k, t in w.items()})
        return res
    return _run(dtype, fn)


class Reference(object):
    """float64 and float32 evaluations of one case, the per-tensor bars, and the kink report.  zero_rows: {tensor: rows that are zero by
    construction}.  The four losses are bounded one by one (loss_bars), not as a tensor."""

    def __init__(self, kind, hp, inp):
        self.kind, self.hp, self.inp = kind, hp, inp
        self.kinks, self.zero_rows = [], {}
        if kind == "front":
            self.ref64, relu64 = evaluate_front(hp, inp, torch.float64)
            self.ref32, relu32 = evaluate_front(hp, inp, torch.float32)
            for i, (z64, z32) in enumerate(zip(relu64, relu32)):
                self.kinks.append(("relu_l%d" % (i + 1), float(np.abs(z64).min()), KINK_FACTOR * float(np.abs(z32 - z64).max())))
            self.zero_rows["embedding"] = sorted(set(range(hp.num_symbols)) - set(int(v) for v in np.unique(inp["ids"])))
            if inp["speakers"] > 1:
                unused = sorted(set(range(inp["speakers"])) - set(int(v) for v in inp["speaker_id"]))
                for k in self.ref64:
                    if k == "speaker_embedding" or k.endswith("/table"):
                        self.zero_rows[k] = unused
        else:
            self.ref64, self.ref32 = evaluate_head(hp, inp, torch.float64), evaluate_head(hp, inp, torch.float32)
            lin_err = float(np.abs(self.ref32["lin"] - self.ref64["lin"]).max())
            gap = min(float(np.abs(self.ref64["lin"] - inp["lin_tgt"]).min()), float(np.abs(inp["mel"].astype(np.float64) - inp["mel_tgt"]).min()))
            self.kinks.append(("l1_gap", gap, float(np.nextafter(L1_GAP, 0.0))))          # gap >= L1_GAP
            self.kinks.append(("l1_gap_over_error", gap, L1_GAP_OVER_ERROR * lin_err))
        self.scale, self.bars = {}, {}
        for k, g in self.ref64.items():
            if k == "losses":
                continue
            self.scale[k] = float(np.abs(g).max())
            self.bars[k] = max(float(np.abs(self.ref32[k] - g).max()), FLOOR * self.scale[k])
        if kind == "head":
            l64, l32 = self.ref64.pop("losses"), self.ref32.pop("losses")
            self.losses64, self.losses32 = l64, l32
            self.loss_bars = np.maximum(np.abs(l32 - l64), FLOOR * np.abs(l64))

    def admissible(self, safety=1.0):
        return all(dist > safety * delta for _, dist, delta in self.kinks)


def make_inputs(case, seed):
    hp = case.hp()
    if case.kind == "front":
        return make_front_inputs(hp, case.B, case.T, seed, case.speakers)
    return make_head_inputs(hp, case.B, case.T, seed, case.speakers, case.coeff, case.prioritize, case.sample_rate, case.dmel_post)


@functools.lru_cache(maxsize=None)
def _reference(case_index, seed):
    c = CASES[case_index]
    return Reference(c.kind, c.hp(), make_inputs(c, seed))


def reference(case):
    """The (cached, shared, read-only) reference of a case of the tables at its pinned seed."""
    return _reference(CASES.index(case), case.seed)


def find_seed(case, base=3, tries=4000):
    """The first seed >= base that is admissible with TWICE the distance: delta is measured on a float32 run, whose rounding differs a
    little from one host's BLAS to the next, and the pinned seed has to be admissible (at the plain factor) on every one of them."""
    for seed in range(base, base + tries):
        if Reference(case.kind, case.hp(), make_inputs(case, seed)).admissible(2.0):
            return seed
    raise RuntimeError("no admissible seed in [%d, %d) for %s" % (base, base + tries, case.id))


def _find(i):
    torch.set_num_threads(1)
    return FRONT_CASES[i].id, find_seed(FRONT_CASES[i])


if __name__ == "__main__":       # prints the seeds that FRONT_CASES pins
    import multiprocessing
    with multiprocessing.Pool(8) as pool:
        for cid, seed in pool.imap(_find, range(len(FRONT_CASES))):
            print(cid, seed, flush=True)
