"""The yardstick of the ends block test (tests/ends_reference.py) checked on the CPU: the pinned seeds keep every prenet ReLU at a distance,
the head's targets keep every L1 kink at a distance by construction, the hand-written ids and speakers are what the case table says, the
two blocks chained into torch_formulation.train_grads carry the whole model's gradient, the priority band is the reference's slice -- and
the host side of the hooks taco_train_debug_front / taco_train_debug_head: symbols, prototypes, declarations, and every argument error,
all returned before any HIP call (so they work without a GPU, on a trainer that stays on the host)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ends_reference as R
import taco_oracle as O
import torch_formulation as TF
from taco_amd import _lib
from util import tiny_hp, to_product_hp

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "taco_debug.h")


def _comparator_sees(ref, k):
    got = {n: v.copy() for n, v in ref.ref32.items()}
    got[k].reshape(-1)[5] += 64.0 * ref.bars[k]
    bad = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN)
    assert [n for n, _ in bad] == [k] and 63.0 <= bad[0][1] <= 65.0, bad


@pytest.mark.parametrize("case", R.FRONT_CASES, ids=[c.id for c in R.FRONT_CASES])
def test_every_front_case_is_admissible_at_its_pinned_seed(case):
    """The kink condition holds in the reference of every case (the seeds are what `python tests/ends_reference.py` prints), the float32
    restatement passes its own bars at margin 1, the comparator reports an element moved by 64 bars -- and the ids and speakers carry what was
    written into them by hand."""
    ref = R.reference(case)
    hp, inp = ref.hp, ref.inp
    for name, dist, delta in ref.kinks:
        print("%s %-10s distance %.3e  delta %.3e" % (case.id, name, dist, delta))
    assert len(ref.kinks) == len(hp.enc_prenet_sizes) and ref.admissible(), [k for k in ref.kinks if not k[1] > k[2]]
    assert R.compare(ref.ref32, ref.ref64, ref.bars, 1.0) == []
    assert all(b > 0 for b in ref.bars.values())
    _comparator_sees(ref, "prenet/dense_1/kernel")
    ids, V = inp["ids"], hp.num_symbols
    assert ids.shape == (case.B, case.T) and ids.min() == 0 and ids.max() == V - 1
    assert (ids[0] == R.REPEATED_SYMBOL).all() and not (ids == R.ABSENT_SYMBOL).any()
    if case.T == 64:
        assert (ids.reshape(-1)[:64] == R.REPEATED_SYMBOL).all()          # one whole ballot block of k_embed_bwd_det
    pad = np.arange(case.T)[None, :] >= inp["lengths"][:, None]
    assert pad.any() and (ids[pad] == 0).all() and (ids[~pad] != 0).all() and np.abs(inp["dpre"][pad]).min() > 0
    zero = ref.zero_rows["embedding"]
    assert R.ABSENT_SYMBOL in zero and 0 not in zero and V - 1 not in zero
    for k, rows in ref.zero_rows.items():
        assert rows, k
        assert not ref.ref64[k][rows].any() and not ref.ref32[k][rows].any(), k
        present = sorted(set(range(ref.ref64[k].shape[0])) - set(rows))
        assert all(np.abs(ref.ref64[k][r]).max() > 0 for r in present), k
    if case.speakers > 1:
        sid = inp["speaker_id"]
        assert set(sid) == {0, 2} and len(sid) > len(set(sid)) and R.UNUSED_SPEAKER not in sid
        tabs = [k for k in ref.zero_rows if k != "embedding"]
        assert tabs == (["speaker_embedding"] if hp.speaker_embedding_size != 1 else ["spk/%s/table" % n for n in R.vector_names(hp)])
        assert all(ref.zero_rows[k] == [R.UNUSED_SPEAKER] for k in tabs)
    want = {"pre", "embedding"} | {"prenet/dense_%d/%s" % (i + 1, p) for i in range(len(hp.enc_prenet_sizes)) for p in ("kernel", "bias")}
    if case.speakers > 1 and hp.model_type == "deepvoice":
        want |= {"vec/" + n for n in R.vector_names(hp)}
        want |= ({"spk/%s/table" % n for n in R.vector_names(hp)} if hp.speaker_embedding_size == 1 else
                 {"spk/%s/%s" % (n, p) for n in R.vector_names(hp) for p in ("kernel", "bias")} | {"spk_emb", "speaker_embedding"})
    if case.speakers > 1 and hp.model_type == "simple":
        want |= {"spk_emb", "speaker_embedding"}
    assert set(ref.ref64) == want


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=[c.id for c in R.HEAD_CASES])
def test_every_head_case_is_flip_free_by_construction(case):
    """No L1 term of a head case can change sign between arithmetics: every |out64 - tgt| is at least 0.25, and more than 1000 times the
    float32 head's own error.  A condition on the inputs, not a tolerance."""
    ref = R.reference(case)
    inp = ref.inp
    gap_lin = float(np.abs(ref.ref64["lin"] - inp["lin_tgt"]).min())
    gap_mel = float(np.abs(inp["mel"].astype(np.float64) - inp["mel_tgt"]).min())
    lin_err = float(np.abs(ref.ref32["lin"] - ref.ref64["lin"]).max())
    print("%s gap lin %.6f mel %.6f, float32 head error %.3e" % (case.id, gap_lin, gap_mel, lin_err))
    assert min(gap_lin, gap_mel) >= R.L1_GAP and min(gap_lin, gap_mel) > R.L1_GAP_OVER_ERROR * lin_err
    assert max(float(np.abs(ref.ref64["lin"] - inp["lin_tgt"]).max()), float(np.abs(inp["mel"] - inp["mel_tgt"]).max())) <= 1.0 + 1e-6
    assert ref.admissible() and len(ref.kinks) == 2
    assert R.compare(ref.ref32, ref.ref64, ref.bars, 1.0) == [] and all(b > 0 for b in ref.bars.values())
    assert (np.abs(ref.losses32 - ref.losses64) <= ref.loss_bars).all() and (ref.loss_bars > 0).all()
    _comparator_sees(ref, "linear/kernel")
    # the sign pattern is the same in both arithmetics: the L1 gradients differ by rounding only
    assert np.array_equal(np.sign(ref.ref32["lin"] - inp["lin_tgt"]), np.sign(ref.ref64["lin"] - inp["lin_tgt"]))
    want = {"teacher", "lin", "dmel", "dpost", "linear/kernel", "linear/bias"} | ({"dspk"} if case.speakers > 1 else set())
    assert set(ref.ref64) == want
    r = ref.hp.reduction_factor
    assert np.array_equal(ref.ref64["teacher"], inp["mel_tgt"][:, r - 1::r].astype(np.float64)) and ref.ref64["teacher"].shape[1] == case.T // r
    if inp["coeff"] is not None:
        assert 0.5 <= inp["coeff"].min() and inp["coeff"].max() <= 1.5 and len(set(inp["coeff"])) == case.B
    # loss_without_coeff = mel_loss + linear_loss (tacotron.py:301)
    assert abs(ref.losses64[3] - ref.losses64[1] - ref.losses64[2]) <= 1e-14
    if inp["coeff"] is None:
        assert abs(ref.losses64[0] - ref.losses64[3]) <= 1e-14


def test_the_case_tables_reach_what_they_are_there_for():
    front, head = R.FRONT_CASES, R.HEAD_CASES
    assert len({c.id for c in R.CASES}) == len(R.CASES)
    assert {c.B * c.T for c in front} >= {27, 65, 128} and max(c.B * c.T for c in R.CASES) <= 130
    tiny = [c for c in front if c.hp().embedding_size == 32]
    refw = [c for c in front if c.hp().embedding_size == 256]
    assert len(tiny) + len(refw) == len(front) and all(c.hp().enc_prenet_sizes == [256, 128] for c in refw)
    assert any(c.hp().enc_prenet_sizes == [32, 18] for c in tiny)
    kinds = lambda cs: {(c.hp().model_type if c.speakers > 1 else "single", c.hp().speaker_embedding_size if c.speakers > 1 else 0) for c in cs}
    assert kinds(tiny) == {("single", 0), ("deepvoice", 4), ("deepvoice", 1), ("simple", 4)}
    assert kinds(refw) == {("single", 0), ("deepvoice", 16), ("simple", 16)}
    assert {c.B for c in front if c.speakers > 1 and c.hp().model_type == "deepvoice"} == {3, 17}
    assert sum(c.atomic for c in front) == 1 and all(c.speakers in (1, 3) for c in front)
    assert {c.paths for c in front} == {R.P_EMBED_DET, R.P_EMBED_ATOMIC, R.P_EMBED_DET | R.P_SPK_TABLES, R.P_EMBED_DET | R.P_SPK_DENSE}
    htiny = [c for c in head if c.hp().num_freq == 36]
    href = [c for c in head if c.hp().num_freq == 1025]
    assert len(htiny) + len(href) == len(head)
    assert all(c.hp().reduction_factor == 5 and 2 * c.hp().post_rnn_size == 512 for c in href)
    assert {c.B * c.T for c in htiny} >= {12} and {c.B * c.T for c in href} == {20, 65}
    assert 1 in {c.B for c in head} and {c.hp().reduction_factor for c in htiny} >= {1, 3}
    assert {(c.prioritize, c.sample_rate) for c in href} >= {(False, 24000), (True, 24000), (True, 16000), (True, 8000)}
    assert {(c.prioritize, c.sample_rate) for c in htiny} >= {(False, 24000), (True, 24000), (True, 8000)}
    assert {c.coeff for c in head} == {False, True} and {c.dmel_post for c in head} == {False, True}
    assert {c.hp().num_freq for c in head if c.speakers > 1 and c.hp().model_type == "simple"} == {36, 1025}


def test_the_priority_band_is_the_slice_of_the_reference():
    """tacotron.py:283-288 slices linear_loss[:, :, lower:upper]; a slice clamps its upper end.  The bounds by hand, and add_loss against them."""
    assert R.band(True, 24000, 1025) == (14, 427) and R.band(True, 16000, 1025) == (21, 640) and R.band(True, 8000, 1025) == (42, 1025)
    assert R.band(True, 24000, 36) == (0, 15) and R.band(True, 8000, 36) == (1, 36) and R.band(False, 8000, 36) == (0, 0)
    assert int(5000 / (8000 * 0.5) * 1025) == 1281 and int(5000 / (8000 * 0.5) * 36) == 45          # the unclamped upper ends
    rs = np.random.RandomState(0)
    for sr, Fq in ((24000, 1025), (16000, 1025), (8000, 1025), (24000, 36), (8000, 36)):
        lo, hi = R.band(True, sr, Fq)
        mo, mt = torch.zeros(2, 3, 4, dtype=torch.float64), torch.zeros(2, 3, 4, dtype=torch.float64)
        lo_, lt = torch.tensor(rs.randn(2, 3, Fq)), torch.tensor(rs.randn(2, 3, Fq))
        co = torch.tensor(rs.uniform(0.5, 1.5, size=2))
        l1 = (lt - lo_).abs() * co[:, None, None]
        want = 0.5 * l1.mean() + 0.5 * l1[:, :, lo:hi].sum() / (2 * 3 * (hi - lo))
        assert abs(float(TF.add_loss(mo, mt, lo_, lt, co, True, sr)) - float(want)) <= 1e-15, (sr, Fq)


@pytest.mark.parametrize("model_type,speakers,spk_size", [("single", 1, 4), ("deepvoice", 3, 4), ("deepvoice", 2, 1)])
def test_the_two_blocks_chained_carry_the_gradient_of_the_whole_model(model_type, speakers, spk_size):
    """TF.train_grads of the whole model, with the tensors at the seams captured: the front block fed d(prenet output) and d(speaker vectors)
    of the whole graph reproduces its gradients of embedding, prenet/..., speaker_embedding, spk/...; the head block fed the post CBHG's output
    reproduces linear/..., d(post output) and the loss -- to float64 round-off.  So the block reference is the same function as the whole one."""
    hp = tiny_hp(attention_type="bah_mon", model_type=model_type, speaker_embedding_size=spk_size)
    B, T_in, n, r = 3, 7, 4, hp.reduction_factor
    w = O.init_weights(hp, speakers, 11)
    rs = np.random.RandomState(12)
    w["linear/bias"] = 0.1 * rs.randn(hp.num_freq)
    ids = rs.randint(1, 20, size=(B, T_in))
    L = np.array([T_in, 5, 6])
    mt, lt = rs.randn(B, n * r, hp.num_mels), rs.randn(B, n * r, hp.num_freq)
    coeff = rs.uniform(0.5, 1.5, size=B)
    sid = np.array([0, speakers - 1, speakers - 1]) if speakers > 1 else None
    seen = {}
    inner_cbhg, inner_dec = TF.cbhg, TF.decoder

    def cbhg(x, lengths, wt, scope, K, depth, nproj, before=None, init=None, training=False):
        out = inner_cbhg(x, lengths, wt, scope, K, depth, nproj, before, init, training)
        if scope == "encoder_cbhg":
            for t in (x, before, init):
                if t is not None:
                    t.retain_grad()
            seen.update(pre=x, before=before, enc_init=init)
        else:
            out.retain_grad()
            seen.update(post_out=out, mel=x)
        return out

    def decoder(wt, hp_, enc, n_, spk, att_init, dec_inits, manual, training, teacher_frames):
        for t in [att_init] + list(dec_inits or []):
            if t is not None:
                t.retain_grad()
        seen.update(att_init=att_init, dec_inits=dec_inits)
        return inner_dec(wt, hp_, enc, n_, spk, att_init, dec_inits, manual, training, teacher_frames)

    TF.cbhg, TF.decoder = cbhg, decoder
    try:
        loss, g, out = TF.train_grads(w, hp, ids, L, mt, lt, coeff, sid, speakers, prioritize_loss=True, sample_rate=8000)
    finally:
        TF.cbhg, TF.decoder = inner_cbhg, inner_dec
    np64 = lambda t: t.detach().numpy()
    close = lambda a, b, k: float(np.abs(a - b).max()) <= 1e-12 * float(np.abs(b).max()) > 0 or pytest.fail(k)
    # ---- front ----
    inp = {"w": w, "ids": ids, "speaker_id": sid, "speakers": speakers, "dpre": np64(seen["pre"].grad), "dvec": None, "dspk_emb": None}
    if speakers > 1:
        vecs = [seen["before"], seen["enc_init"], seen["att_init"]] + list(seen["dec_inits"])
        inp["dvec"] = [np64(t.grad) for t in vecs]
    res, _ = R.evaluate_front(hp, inp, torch.float64)
    assert np.array_equal(res["pre"], np64(seen["pre"]))
    want = {k: v for k, v in g.items() if R.in_scope("front", k)}
    assert set(want) == set(res) - {"pre", "spk_emb"} - {k for k in res if k.startswith("vec/")} and len(want) >= 5
    assert speakers == 1 or any(k.startswith("spk/") for k in want)
    for k, v in want.items():
        close(res[k], v, k)
    if speakers > 1:
        for nm, t in zip(R.vector_names(hp), vecs):
            assert np.array_equal(res["vec/" + nm], np64(t)), nm
    # ---- head ----
    inp = {"w": w, "post_out": np64(seen["post_out"]), "mel": out["mel"], "spk_emb": None, "mel_tgt": mt, "lin_tgt": lt, "coeff": coeff,
           "prioritize": True, "sample_rate": 8000, "dmel_post": None}
    res = R.evaluate_head(hp, inp, torch.float64)
    assert np.array_equal(res["lin"], out["linear"]) and abs(res["losses"][0] - loss) <= 1e-14 * abs(loss)
    for k in ("linear/kernel", "linear/bias"):
        close(res[k], g[k], k)
    close(res["dpost"], np64(seen["post_out"].grad), "dpost")
    assert np.array_equal(res["teacher"], mt[:, r - 1::r])


NAMES = ("taco_train_debug_front", "taco_train_debug_front_workspace_bytes", "taco_train_debug_head", "taco_train_debug_head_workspace_bytes")
FRONT_ARGS = ["taco_train* t", "void* hip_stream", "float* d_params", "float* d_grads", "const int32_t* d_ids", "const int32_t* d_speaker_id",
              "const float* d_dpre", "const float* const* d_dvec", "const float* d_dspk_emb", "int B", "int T_in", "float* d_pre",
              "float* const* d_vec", "float* d_spk_emb", "void* d_ws", "size_t ws_bytes", "uint32_t* paths"]
HEAD_ARGS = ["taco_train* t", "void* hip_stream", "float* d_params", "float* d_grads", "const float* d_post_out", "const float* d_mel",
             "const float* d_mel_tgt", "const float* d_lin_tgt", "const float* d_loss_coeff", "const float* d_dmel_post", "const float* d_spk_emb",
             "int B", "int T_out", "int prioritize_loss", "int sample_rate", "float* d_teacher", "float* d_lin", "float* d_losses", "float* d_dmel",
             "float* d_dpost", "float* d_dspk_emb", "void* d_ws", "size_t ws_bytes"]


def test_the_library_exports_the_hooks_and_the_prototypes_carry_them():
    lib = _lib.load_library()
    P, I, S = C.c_void_p, C.c_int, C.c_size_t
    for name in NAMES:
        assert name in _lib.PROTOTYPES and getattr(lib, name)
    fn = lib.taco_train_debug_front
    assert fn.restype is C.c_int and list(fn.argtypes) == [P] * 9 + [I] * 2 + [P] * 4 + [S, P]
    fn = lib.taco_train_debug_head
    assert fn.restype is C.c_int and list(fn.argtypes) == [P] * 11 + [I] * 4 + [P] * 7 + [S]
    for fn in (lib.taco_train_debug_front_workspace_bytes, lib.taco_train_debug_head_workspace_bytes):
        assert fn.restype is S and list(fn.argtypes) == [P, I, I]


@pytest.mark.parametrize("which,args,words", [
    ("front", FRONT_ARGS, ("front_forward_train", "front_backward", "speaker_rows_backward", "ADDED", "TACO_ERR_ARG", "TACO_ERR_STATE",
                           "before the first HIP call", "bit 0 / 1", "bit 2 / 3", "k_embed_bwd_det", "single-speaker")),
    ("head", HEAD_ARGS, ("teacher_frames", "head_forward_train", "head_backward", "head_backward_join", "taco_loss_f32", "ADDED", "TACO_ERR_ARG",
                         "TACO_ERR_STATE", "TACO_ERR_SHAPE", "before the first HIP call", "without its input"))])
def test_the_header_declares_the_hooks_and_their_contracts(which, args, words):
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*size_t\s+taco_train_debug_%s_workspace_bytes\s*\(([^;]*)\)\s*;\s*int\s+taco_train_debug_%s\s*\(([^;]*)\)\s*;"
                  % (which, which), text, flags=re.S)
    assert m, "not declared"
    comment = re.sub(r"\s+", " ", m.group(1))
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(3).split(",")] == args
    assert [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")] == ["const taco_train* t", "int B", "int T_in" if which == "front" else "int T_out"]
    for word in words:
        assert word in comment, word


class _HostTrainer(object):
    def __init__(self, hp, speakers=1):
        self.lib = _lib.load_library()
        self.h = C.c_void_p()
        chp = _lib.to_c_hparams(to_product_hp(hp), speakers)
        _lib.check(self.lib.taco_debug_train_create_host(C.byref(chp), C.byref(self.h)))

    def close(self):
        self.lib.taco_train_destroy(self.h)


A = lambda i: (i + 1) << 24                        # dummy device addresses: 16 MiB apart, 16-byte aligned
_p = lambda v: C.c_void_p(v) if v else None
_tab = lambda v: None if v is None else (C.c_void_p * len(v))(*v)


def _front(lib, tr, **kw):
    a = dict(t=tr.h if tr else None, params=A(0), grads=A(1), ids=A(2), sid=0, dpre=A(3), dvec=None, dspk=0, B=2, T_in=5, pre=A(4), vec=None, spk=0,
             ws=A(8), ws_bytes=None, paths=0)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(lib.taco_train_debug_front_workspace_bytes(a["t"], a["B"], a["T_in"])) if tr else 1 << 20
    rc = lib.taco_train_debug_front(a["t"], None, _p(a["params"]), _p(a["grads"]), _p(a["ids"]), _p(a["sid"]), _p(a["dpre"]), _tab(a["dvec"]), _p(a["dspk"]),
                                    a["B"], a["T_in"], _p(a["pre"]), _tab(a["vec"]), _p(a["spk"]), _p(a["ws"]), a["ws_bytes"], _p(a["paths"]))
    return rc, lib.taco_last_error()


def _head(lib, tr, **kw):
    a = dict(t=tr.h if tr else None, params=A(0), grads=A(1), post=A(2), mel=A(3), mel_tgt=A(4), lin_tgt=A(5), coeff=0, dmel_post=0, spk=0, B=2, T_out=6,
             prioritize=0, sample_rate=24000, teacher=A(6), lin=A(7), losses=A(9), dmel=A(10), dpost=A(11), dspk=0, ws=A(8), ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = int(lib.taco_train_debug_head_workspace_bytes(a["t"], a["B"], a["T_out"])) if tr else 1 << 20
    rc = lib.taco_train_debug_head(a["t"], None, _p(a["params"]), _p(a["grads"]), _p(a["post"]), _p(a["mel"]), _p(a["mel_tgt"]), _p(a["lin_tgt"]),
                                   _p(a["coeff"]), _p(a["dmel_post"]), _p(a["spk"]), a["B"], a["T_out"], a["prioritize"], a["sample_rate"], _p(a["teacher"]),
                                   _p(a["lin"]), _p(a["losses"]), _p(a["dmel"]), _p(a["dpost"]), _p(a["dspk"]), _p(a["ws"]), a["ws_bytes"])
    return rc, lib.taco_last_error()


ARG, STATE, SHAPE, UNSUPPORTED = _lib.TACO_ERR_ARG, _lib.TACO_ERR_STATE, _lib.TACO_ERR_SHAPE, _lib.TACO_ERR_UNSUPPORTED


def test_front_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory on a trainer that never touched a device: validation rejects every one of these
    calls before anything is launched; a call that passes them all is refused because the trainer is host-only."""
    lib = _lib.load_library()
    assert lib.taco_train_debug_front_workspace_bytes(None, 2, 5) == 0
    rc, msg = _front(lib, None)
    assert rc == ARG and b"null" in msg

    tr = _HostTrainer(tiny_hp())
    try:
        for B, T in ((0, 5), (2, 0), (-1, 5)):
            assert lib.taco_train_debug_front_workspace_bytes(tr.h, B, T) == 0
        nb = int(lib.taco_train_debug_front_workspace_bytes(tr.h, 2, 5))
        assert nb > 0 and nb % 256 == 0
        for k in ("params", "grads", "ids", "dpre", "pre", "ws"):
            rc, msg = _front(lib, tr, **{k: 0})
            assert rc == ARG and b"null" in msg, k
        for kw in (dict(sid=A(9)), dict(dvec=[A(9)] * 5), dict(dspk=A(9)), dict(vec=[A(9)] * 5), dict(spk=A(9))):      # speaker inputs on a single-speaker model
            rc, msg = _front(lib, tr, **kw)
            assert rc == ARG and b"single-speaker" in msg, kw
        for kw in (dict(B=0), dict(T_in=0), dict(B=-3)):
            rc, msg = _front(lib, tr, ws_bytes=nb, **kw)
            assert rc == ARG and b"bad" in msg, kw
        rc, msg = _front(lib, tr, B=65)
        assert rc == UNSUPPORTED and b"64" in msg
        rc, msg = _front(lib, tr, ws=A(8) + 4)
        assert rc == ARG and b"aligned" in msg
        rc, msg = _front(lib, tr)                                       # the trainer as created wants split-bf16 planes, and none were ever generated
        assert rc == STATE and b"stale" in msg
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        for bad in (nb - 1, 0):
            rc, msg = _front(lib, tr, ws_bytes=bad)
            assert rc == STATE and b"too small" in msg
        for kw in (dict(), dict(paths=A(11))):                          # every check passed: only now would the device be touched
            rc, msg = _front(lib, tr, **kw)
            assert rc == STATE and b"host-only" in msg, kw
        assert lib.taco_train_set_deterministic(tr.h, 0) == 0           # the switches that size the workspace are the trainer's
        assert 0 < int(lib.taco_train_debug_front_workspace_bytes(tr.h, 2, 5)) < nb
    finally:
        tr.close()

    for spk_size in (4, 1):
        tr = _HostTrainer(tiny_hp(model_type="deepvoice", speaker_embedding_size=spk_size), speakers=3)
        try:
            assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
            vec, dvec = [A(20 + i) for i in range(5)], [A(30 + i) for i in range(5)]
            rc, msg = _front(lib, tr, vec=vec, dvec=dvec)
            assert rc == ARG and b"speaker_id" in msg
            rc, msg = _front(lib, tr, sid=A(9), dvec=dvec)
            assert rc == ARG and b"without its forward output" in msg
            for kw in (dict(), dict(vec=vec), dict(vec=vec, dvec=dvec[:4] + [0]), dict(vec=[0] + vec[1:], dvec=dvec), dict(vec=vec, dvec=dvec, dspk=A(12), spk=A(13))):
                rc, msg = _front(lib, tr, sid=A(9), **kw)
                assert rc == ARG, kw
            rc, msg = _front(lib, tr, sid=A(9), vec=vec, dvec=dvec)
            assert rc == STATE and b"host-only" in msg
            rc, msg = _front(lib, tr, sid=A(9), vec=vec, dvec=dvec, spk=A(13))      # the gathered rows: an optional output, where there are rows
            assert (rc == STATE and b"host-only" in msg) if spk_size > 1 else (rc == ARG and b"tables" in msg)
        finally:
            tr.close()

    tr = _HostTrainer(tiny_hp(model_type="simple"), speakers=3)
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        rc, msg = _front(lib, tr, spk=A(13), dspk=A(12))
        assert rc == ARG and b"speaker_id" in msg
        rc, msg = _front(lib, tr, sid=A(9), dspk=A(12))
        assert rc == ARG and b"without its forward output" in msg
        for kw in (dict(), dict(spk=A(13)), dict(spk=A(13), dspk=A(12), vec=[A(20)] * 5, dvec=[A(30)] * 5)):
            rc, msg = _front(lib, tr, sid=A(9), **kw)
            assert rc == ARG, kw
        rc, msg = _front(lib, tr, sid=A(9), spk=A(13), dspk=A(12))
        assert rc == STATE and b"host-only" in msg
    finally:
        tr.close()


def test_head_argument_errors_return_before_any_device_call():
    lib = _lib.load_library()
    assert lib.taco_train_debug_head_workspace_bytes(None, 2, 6) == 0
    rc, msg = _head(lib, None)
    assert rc == ARG and b"null" in msg

    tr = _HostTrainer(tiny_hp())                                        # r = 3, max_iters = 7
    try:
        for B, T in ((0, 6), (2, 0), (-1, 6)):
            assert lib.taco_train_debug_head_workspace_bytes(tr.h, B, T) == 0
        nb = int(lib.taco_train_debug_head_workspace_bytes(tr.h, 2, 6))
        assert nb > 0 and nb % 256 == 0
        for k in ("params", "grads", "post", "mel", "mel_tgt", "lin_tgt", "teacher", "lin", "losses", "dmel", "dpost", "ws"):
            rc, msg = _head(lib, tr, **{k: 0})
            assert rc == ARG and b"null" in msg, k
        rc, msg = _head(lib, tr, dspk=A(12))
        assert rc == ARG and b"without its input" in msg
        for kw in (dict(spk=A(13)), dict(spk=A(13), dspk=A(12))):       # speaker rows on a single-speaker model
            rc, msg = _head(lib, tr, **kw)
            assert rc == ARG and b"simple" in msg, kw
        for kw in (dict(B=0), dict(T_out=0), dict(B=-3), dict(sample_rate=0)):
            rc, msg = _head(lib, tr, ws_bytes=nb, **kw)
            assert rc == ARG and b"bad" in msg, kw
        rc, msg = _head(lib, tr, B=65)
        assert rc == UNSUPPORTED and b"64" in msg
        rc, msg = _head(lib, tr, T_out=7)
        assert rc == SHAPE and b"multiple" in msg
        rc, msg = _head(lib, tr, T_out=24)
        assert rc == SHAPE and b"max_iters" in msg
        rc, msg = _head(lib, tr, ws=A(8) + 4)
        assert rc == ARG and b"aligned" in msg
        rc, msg = _head(lib, tr)
        assert rc == STATE and b"stale" in msg
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        for bad in (nb - 1, 0):
            rc, msg = _head(lib, tr, ws_bytes=bad)
            assert rc == STATE and b"too small" in msg
        for kw in (dict(), dict(coeff=A(12), dmel_post=A(13), prioritize=1, sample_rate=8000)):
            rc, msg = _head(lib, tr, **kw)
            assert rc == STATE and b"host-only" in msg, kw
        assert lib.taco_train_set_deterministic(tr.h, 0) == 0
        assert 0 < int(lib.taco_train_debug_head_workspace_bytes(tr.h, 2, 6)) < nb
    finally:
        tr.close()

    tr = _HostTrainer(tiny_hp(model_type="simple"), speakers=2)
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        for kw in (dict(), dict(spk=A(13))):
            rc, msg = _head(lib, tr, **kw)
            assert rc == ARG and b"simple" in msg, kw
        rc, msg = _head(lib, tr, dspk=A(12))
        assert rc == ARG and b"without its input" in msg
        rc, msg = _head(lib, tr, spk=A(13), dspk=A(12))
        assert rc == STATE and b"host-only" in msg
    finally:
        tr.close()

    tr = _HostTrainer(tiny_hp(model_type="deepvoice"), speakers=2)      # the head of a deepvoice model takes no speaker rows
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        rc, msg = _head(lib, tr, spk=A(13), dspk=A(12))
        assert rc == ARG and b"simple" in msg
        rc, msg = _head(lib, tr)
        assert rc == STATE and b"host-only" in msg
    finally:
        tr.close()
