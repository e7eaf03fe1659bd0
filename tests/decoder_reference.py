"""The decoder in training mode on the CPU, float64 and float32, with reverse-mode autograd -- the yardstick of the block tests
(tests/test_decoder_reference_host.py, tests/test_gpu_decoder_train.py).  No GPU, no library: tests/torch_formulation.py::decoder only.

The upstream gradient `dmel` is an input, so the loss sum(mel * dmel) has no kink of its own -- the L1 loss, to whose kinks the 2e-3 bound
of the whole-model gradient tests is owed, is not part of the block.  What kinks remain (the ReLUs of the decoder prenet; the two clips of
the monotonic normaliser) are kept at a distance by the choice of the seed:

  error bar of tensor k      bar_k = max(max|g32_k - g64_k|, 2^-20 * s_k),  s_k = max|g64_k|
                             (the float32 restatement's own error; the floor is 8 fp32 ulps of the largest element)
  structural zero            a tensor whose float64 gradient is zero by construction takes the scale of a named neighbour:
                               n = 1       decoder/prenet/dense_1/kernel: the first step's prenet input is the zero frame and the zero
                                           context; scale of the same layer's bias
                               T_in = 1    (softmax attentions) the softmax of ONE score is 1 whatever the score, so nothing reaches
                                           the score path: query_layer/kernel, memory_layer/kernel, attention_v (bah_norm: _g, _b too);
                                           scale of decoder/attention_gru/candidate/bias, the nearest bias in front of the query
  kink condition             with delta = 32 * max|z32 - z64| of a pre-activation tensor z: every decoder-prenet ReLU pre-activation has
                             |z64| > delta.  bah_mon: every element of the exclusive cumprod cp is farther from the 1e-10 clip than 32
                             times its own float32-vs-float64 difference (the error of cp is relative: cp spans thirty decades), and the
                             smallest 1 - p of the float32 run is more than 32 * tiny above the `tiny` clip.  A seed is admissible when all
                             of them hold; find_seed() returns the first admissible seed from a base, and CASES pins what it returned.

Where the 1e-10 clip IS active (cp < 1e-10: long inputs, where the monotonic mass has moved on) tf.gradients -- and this reference --
stop the gradient through the clipped denominator; the case table has such cases on purpose (Reference.clip_active counts the elements)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import taco_oracle as O
import torch_formulation as TF
from cbhg_reference import COMMON_MARGIN, FLOOR, KINK_FACTOR, compare, ratios          # the comparator is the CBHG block test's
from util import tiny_hp

__all__ = ["COMMON_MARGIN", "FLOOR", "KINK_FACTOR", "compare", "ratios"]

# taco_train_debug_decoder's `paths` word (include/taco_debug.h)
P_FWD_PERSISTENT, P_FWD_STAGES, P_BWD_PERSISTENT, P_BWD_STAGES = 1 << 0, 1 << 1, 1 << 2, 1 << 3
P_FWD_RG_SHIFT, P_BWD_RG_SHIFT = 4, 8
P_XCD_LOCAL, P_WRITE_THROUGH = 1 << 12, 1 << 13
P_PROTOCOLS = P_XCD_LOCAL | P_WRITE_THROUGH
STAGES = P_FWD_STAGES | P_BWD_STAGES


def persistent(rg):
    """The word (without the protocol bits, which the census of the launch decides) of a call whose two loops both ran as ONE launch."""
    return P_FWD_PERSISTENT | P_BWD_PERSISTENT | rg << P_FWD_RG_SHIFT | rg << P_BWD_RG_SHIFT


def forward_only(rg):
    """... with taco_train_set_bptt_engine(t, 0): the persistent forward, the per-stage BPTT."""
    return P_FWD_PERSISTENT | P_BWD_STAGES | rg << P_FWD_RG_SHIFT


class Case(object):
    """One row of the table.  paths: the word of a whole MI355X without its protocol bits (STAGES: the launch-per-stage engines; persistent(rg)
    at the reference widths); paths_partition: on a device of fewer than 256 compute units.  speakers > 1: a multi-speaker model -- deepvoice
    feeds initial states (and takes their gradients), 'simple' the speaker rows.  write_through: the exchanges of the persistent launches are
    forced write-through (taco_debug_set_decoder_persist mode 2).  margins: tensors with a stated margin of their own, {name: (margin, reason)}."""

    def __init__(self, name, hp, B, T_in, n, seed, paths=STAGES, speakers=1, write_through=False, margins=None):
        self.name, self.hp_fn, self.B, self.T_in, self.n, self.seed = name, hp, B, T_in, n, seed
        self.paths, self.paths_partition, self.speakers, self.write_through = paths, STAGES, speakers, write_through
        self.margins = margins or {}
        self.id = "%s-B%d-T%d-n%d" % (name, B, T_in, n)

    def hp(self):
        return self.hp_fn()

    @property
    def reference_widths(self):
        return self.paths != STAGES


def _tiny(**kw):
    return lambda: tiny_hp(**kw)


def _ref(**kw):
    return lambda: O.OracleHParams(**kw)


# seeds: find_seed(case, base=3), printed by `python tests/decoder_reference.py` -- see
# tests/test_decoder_reference_host.py::test_every_case_is_admissible_at_its_pinned_seed.  (At 64 rows a prenet layer has 16384 pre-activations
# per step, of which one in ten thousand lies within twice delta of zero: few seeds keep all of them away, hence 3927.)
CASES = [
    # ---- tiny widths: the launch-per-stage engines ----
    Case("bah", _tiny(attention_type="bah"), 3, 9, 4, 3),
    Case("bah_norm", _tiny(attention_type="bah_norm"), 5, 13, 6, 3),                 # odd sizes, more rows than one weight-gradient slice of a step
    Case("bah_mon", _tiny(attention_type="bah_mon"), 3, 9, 4, 3),
    Case("one_position", _tiny(attention_type="bah"), 3, 1, 3, 3),                   # T_in = 1: the softmax of one score
    Case("one_position_mon", _tiny(attention_type="bah_mon"), 3, 1, 3, 3),
    Case("one_step", _tiny(attention_type="bah_norm"), 3, 9, 1, 3),                  # n = 1: no recurrence, zero prenet input
    Case("clip_active", _tiny(attention_type="bah_mon"), 2, 72, 4, 3),               # cp < 1e-10 from the 35th position or so on
    Case("r1", _tiny(attention_type="bah_mon", reduction_factor=1), 3, 9, 5, 3),
    Case("r5", _tiny(attention_type="bah", reduction_factor=5), 3, 9, 3, 3),
    Case("deepvoice", _tiny(attention_type="bah_mon", model_type="deepvoice"), 3, 9, 4, 3, speakers=2),
    Case("simple", _tiny(attention_type="bah_norm", model_type="simple"), 3, 9, 4, 3, speakers=2),
    Case("deepvoice_s1", _tiny(attention_type="bah", model_type="deepvoice", speaker_embedding_size=1), 4, 13, 3, 3, speakers=2),
    # ---- reference widths: persistent forward and BPTT on an unpartitioned device; rows per group 1 / 2 / 4 / 8 ----
    Case("reference", _ref(), 3, 24, 3, 3, persistent(1)),
    Case("reference_wt", _ref(), 3, 24, 4, 3, persistent(1), write_through=True),
    Case("reference_bah", _ref(attention_type="bah"), 9, 24, 4, 10, persistent(2)),
    Case("reference_bah_norm", _ref(attention_type="bah_norm"), 9, 24, 4, 7, persistent(2)),
    Case("reference", _ref(), 9, 24, 4, 6, persistent(2)),
    Case("reference_deepvoice", _ref(model_type="deepvoice"), 17, 24, 3, 3, persistent(4), speakers=2),
    Case("reference", _ref(), 33, 24, 3, 13, persistent(8)),
    Case("reference", _ref(), 64, 24, 3, 3927, persistent(8)),                       # all rows of the chip
    Case("reference_long", _ref(), 9, 150, 3, 4, persistent(2)),                     # the chunked normaliser backward; the 1e-10 clip active
]

SCOPES = ("decoder/", "attention/")


def in_scope(name):
    return name.startswith(SCOPES)


def dims(hp):
    """(D, attention_state_size, dec_rnn_size, r * num_mels)"""
    return 2 * hp.enc_rnn_size, hp.attention_state_size, hp.dec_rnn_size, hp.reduction_factor * hp.num_mels


def make_inputs(hp, B, T_in, n, seed, speakers=1):
    """Weights of the whole model from O.init_weights(seed) and the block's data from RandomState(seed + 1): the attention memory and the
    initial states / speaker rows ~ 0.5 * randn (GRU states and softsign outputs lie in (-1, 1)), teacher frames and dmel ~ randn."""
    D, As, Hd, rM = dims(hp)
    w = O.init_weights(hp, speakers, seed)
    rs = np.random.RandomState(seed + 1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    d = {"w": w, "enc": f32(0.5 * rs.randn(B, T_in, D)), "teacher": f32(rs.randn(B, n, hp.num_mels)), "dmel": f32(rs.randn(B, n, rM)),
         "att_init": None, "dec_inits": None, "spk": None}
    if speakers > 1 and hp.model_type == "deepvoice":
        d["att_init"] = f32(0.5 * rs.randn(B, As))
        d["dec_inits"] = [f32(0.5 * rs.randn(B, Hd)) for _ in range(hp.dec_layer_num)]
    if speakers > 1 and hp.model_type == "simple":
        d["spk"] = f32(0.5 * rs.randn(B, hp.speaker_embedding_size))
    return d


class _Recorder(object):
    """Stands in for torch.nn.functional inside torch_formulation for one call: records every ReLU input and passes everything through."""

    def __init__(self):
        self.relu_in = []

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, y):
        self.relu_in.append(y)
        return F.relu(y)


def evaluate(hp, inp, dtype, closed_form=None):
    """torch_formulation.decoder(training=True, teacher forced) at `dtype` + autograd of sum(mel * dmel).  Returns (tensors, relu, mono):
    tensors = mel [B, n, r*num_mels], alignments [B, T_in, n], denc, datt_init / ddec_init_i / dspk (where given) and every parameter
    gradient of decoder/... and attention/... by its name; relu = the prenet's ReLU pre-activations in call order (step-major); mono = per
    step (cp, 1 - p) of the monotonic normaliser (bah_mon; else empty).  All float64 NumPy."""
    old_dt, old_F, old_cf, old_nt = TF.DT, TF.F, TF.monotonic_closed_form, torch.get_num_threads()
    rec, mono = _Recorder(), []
    cf = closed_form or old_cf

    def recording_closed_form(p, prev):
        lg = torch.log(torch.clamp(1 - p, torch.finfo(p.dtype).tiny, 1.0))        # as monotonic_closed_form computes them
        mono.append((torch.exp(torch.cumsum(lg, 1) - lg).detach(), (1 - p).detach()))
        return cf(p, prev)

    TF.DT, TF.F, TF.monotonic_closed_form = dtype, rec, recording_closed_form
    torch.set_num_threads(1)          # one summation order for the float32 run, whatever the host
    try:
        leaf = lambda a: None if a is None else torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True)
        w = {k: leaf(v) for k, v in inp["w"].items() if in_scope(k)}
        enc, att_init, spk = leaf(inp["enc"]), leaf(inp["att_init"]), leaf(inp["spk"])
        dec_inits = None if inp["dec_inits"] is None else [leaf(a) for a in inp["dec_inits"]]
        n = inp["teacher"].shape[1]
        y, al = TF.decoder(w, hp, enc, n, spk, att_init, dec_inits, None, True, torch.tensor(np.asarray(inp["teacher"]), dtype=dtype))
        (y * torch.tensor(np.asarray(inp["dmel"]), dtype=dtype)).sum().backward()
    finally:
        TF.DT, TF.F, TF.monotonic_closed_form = old_dt, old_F, old_cf
        torch.set_num_threads(old_nt)
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    grad = lambda t: f64(t.grad) if t.grad is not None else np.zeros(tuple(t.shape))
    res = {"mel": f64(y), "alignments": f64(al), "denc": grad(enc)}
    if att_init is not None:
        res["datt_init"] = grad(att_init)
    for i, t in enumerate(dec_inits or []):
        res["ddec_init_%d" % (i + 1)] = grad(t)
    if spk is not None:
        res["dspk"] = grad(spk)
    for k, t in w.items():
        res[k] = grad(t)
    assert len(rec.relu_in) == n * len(hp.dec_prenet_sizes) and len(mono) == (n if hp.attention_type == "bah_mon" else 0)
    return res, [f64(z) for z in rec.relu_in], [(f64(c), f64(q)) for c, q in mono]


CLIP = 1e-10
_SCORE_PATH = ("attention/query_layer/kernel", "attention/memory_layer/kernel", "attention/attention_v", "attention/attention_g",
               "attention/attention_b")


class Reference(object):
    """float64 and float32 evaluations of one case, the per-tensor bars, and the kink report."""

    def __init__(self, hp, inp):
        self.hp, self.inp = hp, inp
        self.ref64, relu64, mono64 = evaluate(hp, inp, torch.float64)
        self.ref32, relu32, mono32 = evaluate(hp, inp, torch.float32)
        B, T_in, _ = inp["enc"].shape
        n = inp["teacher"].shape[1]
        self.structural_zero = {}
        if n == 1:
            self.structural_zero["decoder/prenet/dense_1/kernel"] = "decoder/prenet/dense_1/bias"
        if T_in == 1 and hp.attention_type != "bah_mon":
            for k in _SCORE_PATH:
                if k in self.ref64:
                    self.structural_zero[k] = "decoder/attention_gru/candidate/bias"
        self.scale, self.bars = {}, {}
        for k, g in self.ref64.items():
            s = float(np.abs(self.ref64[self.structural_zero.get(k, k)]).max())
            self.scale[k] = s
            self.bars[k] = max(float(np.abs(self.ref32[k] - g).max()) if g.size else 0.0, FLOOR * s)
        # kinks: (name, smallest distance from the kink, delta)
        self.kinks = []
        npre = len(hp.dec_prenet_sizes)
        for i, (z64, z32) in enumerate(zip(relu64, relu32)):
            self.kinks.append(("relu_t%d_l%d" % (i // npre, i % npre + 1), float(np.abs(z64).min()), KINK_FACTOR * float(np.abs(z32 - z64).max())))
        self.clip_active = 0
        tiny32 = float(np.finfo(np.float32).tiny)
        for t, ((cp64, q64), (cp32, q32)) in enumerate(zip(mono64, mono32)):
            dist, delta = np.abs(cp64 - CLIP), KINK_FACTOR * np.abs(cp32 - cp64)
            j = int(np.argmin(dist - delta))                      # the element nearest to failing (element-wise: the error of cp is relative)
            self.kinks.append(("cp_t%d" % t, float(dist.reshape(-1)[j]), float(delta.reshape(-1)[j])))
            self.kinks.append(("one_minus_p_t%d" % t, float(min(q32.min(), q64.min())), KINK_FACTOR * tiny32))
            self.clip_active += int((cp64 < CLIP).sum())

    def admissible(self, safety=1.0):
        return all(dist > safety * delta for _, dist, delta in self.kinks)


@functools.lru_cache(maxsize=None)
def _reference(case_index, seed):
    c = CASES[case_index]
    hp = c.hp()
    return Reference(hp, make_inputs(hp, c.B, c.T_in, c.n, seed, c.speakers))


def reference(case):
    """The (cached, shared, read-only) reference of a case of the table at its pinned seed."""
    return _reference(CASES.index(case), case.seed)


def find_seed(case, base=3, tries=4000):
    """The first seed >= base that is admissible with TWICE the distance: delta is measured on a float32 run, whose rounding differs a
    little from one host's BLAS to the next, and the pinned seed has to be admissible (at the plain factor) on every one of them."""
    hp = case.hp()
    for seed in range(base, base + tries):
        if Reference(hp, make_inputs(hp, case.B, case.T_in, case.n, seed, case.speakers)).admissible(2.0):
            return seed
    raise RuntimeError("no admissible seed in [%d, %d) for %s" % (base, base + tries, case.id))


def _admissible_twice(args):
    i, seed = args
    torch.set_num_threads(1)
    c = CASES[i]
    hp = c.hp()
    return seed, Reference(hp, make_inputs(hp, c.B, c.T_in, c.n, seed, c.speakers)).admissible(2.0)


if __name__ == "__main__":       # prints the seeds that CASES pins: find_seed's answer, the seeds of a block tried side by side
    import multiprocessing
    with multiprocessing.Pool(8) as pool:
        for i, case in enumerate(CASES):
            base, found = 3, None
            while found is None and base < 4003:
                found = next((seed for seed, good in pool.map(_admissible_twice, [(i, s) for s in range(base, base + 64)], chunksize=2) if good), None)
                base += 64
            print(case.id, found, flush=True)
