"""The yardstick of the decoder block test (tests/decoder_reference.py) checked on the CPU: the pinned seeds keep every kink at a distance,
the cases meant to have the 1e-10 clip active have it, decoder() lifted out of torch_formulation.forward still carries the whole model's
gradient, the closed form of the monotonic normaliser equals its recurrence exactly where no clip acts -- and the host side of the hook
taco_train_debug_decoder: symbols, prototypes, declaration, and every argument error, all returned before any HIP call (so they work
without a GPU, on a trainer that stays on the host)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import decoder_reference as R
import taco_oracle as O
import torch_formulation as TF
from taco_amd import _lib
from util import tiny_hp, to_product_hp

IDS = [c.id for c in R.CASES]
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "taco_debug.h")


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_case_is_admissible_at_its_pinned_seed(case):
    """The kink conditions of tests/decoder_reference.py hold in the reference of every case.  (The seeds are what
    `python tests/decoder_reference.py` prints: the first admissible seed from 3 upwards.)  The float32 restatement passes its own bars at
    margin 1, and the comparator reports an element moved by 64 bars."""
    ref = R.reference(case)
    for name, dist, delta in ref.kinks:
        print("%s %-18s distance %.3e  delta %.3e" % (case.id, name, dist, delta))
    assert ref.kinks and ref.admissible(), [k for k in ref.kinks if not k[1] > k[2]]
    mon = ref.hp.attention_type == "bah_mon"
    assert len(ref.kinks) == case.n * (len(ref.hp.dec_prenet_sizes) + (2 if mon else 0))
    # the clip's zero-gradient branch is active in the two long cases (elsewhere it may be: 24 positions reach 1e-10 where p is large)
    print("%s elements of cp below 1e-10: %d" % (case.id, ref.clip_active))
    assert ref.clip_active > 0 or not (mon and case.T_in >= 72)
    assert R.compare(ref.ref32, ref.ref64, ref.bars, 1.0) == []
    assert all(b > 0 for b in ref.bars.values())
    k = "attention/query_layer/kernel"
    got = {n: v.copy() for n, v in ref.ref32.items()}
    got[k].reshape(-1)[5] += 64.0 * ref.bars[k]
    bad = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN)
    assert [n for n, _ in bad] == [k] and 63.0 <= bad[0][1] <= 65.0, bad


def test_the_structural_zero_rule_names_exactly_the_tensors_whose_gradient_vanishes():
    """A tensor of the scope whose float64 gradient is below 1e-12 of the largest gradient of the case is a structural zero, and the rule
    of tests/decoder_reference.py names these and no others; each takes a neighbour's scale, which is nowhere near zero."""
    seen = set()
    for case in R.CASES:
        ref = R.reference(case)
        params = [k for k in ref.ref64 if R.in_scope(k)]
        top = max(float(np.abs(ref.ref64[k]).max()) for k in params)
        zeros = {k for k in params if float(np.abs(ref.ref64[k]).max()) < 1e-12 * top}
        assert zeros == set(ref.structural_zero), (case.id, zeros, ref.structural_zero)
        for z, src in ref.structural_zero.items():
            assert ref.scale[z] == float(np.abs(ref.ref64[src]).max()) > 1e-6 * top, (case.id, z)
            assert float(np.abs(ref.ref32[z]).max()) <= ref.bars[z]
        seen |= set(ref.structural_zero)
    assert "decoder/prenet/dense_1/kernel" in seen and "attention/query_layer/kernel" in seen


def test_the_case_table_reaches_every_engine_and_rows_per_group():
    words = [c.paths for c in R.CASES]
    assert {(w >> R.P_FWD_RG_SHIFT) & 15 for w in words if w != R.STAGES} == {1, 2, 4, 8}
    assert all(((w >> R.P_FWD_RG_SHIFT) & 15) == ((w >> R.P_BWD_RG_SHIFT) & 15) for w in words)
    assert R.STAGES in words and any(c.write_through for c in R.CASES) and all(c.paths_partition == R.STAGES for c in R.CASES)
    ref = [c for c in R.CASES if c.reference_widths]
    assert {c.hp().attention_type for c in ref if c.B == 9 and c.T_in == 24} == {"bah", "bah_norm", "bah_mon"}
    assert {c.B for c in ref} >= {3, 9, 17, 33, 64} and {c.T_in for c in ref} == {24, 150}
    tiny = [c for c in R.CASES if not c.reference_widths]
    assert {c.hp().reduction_factor for c in tiny} >= {1, 3, 5} and {c.T_in for c in tiny} >= {1, 9, 72} and 1 in {c.n for c in tiny}
    assert {(c.hp().model_type, c.hp().speaker_embedding_size == 1) for c in tiny if c.speakers > 1} == {("deepvoice", False), ("simple", False),
                                                                                                       ("deepvoice", True)}
    assert all(1 <= c.n <= 6 for c in R.CASES)


def test_decoder_inside_forward_carries_the_gradient_of_the_whole_model():
    """TF.forward calls decoder(); chaining d(mel) of the whole training graph through the block alone reproduces TF.train_grads on every
    decoder and attention tensor, and d(encoder output) / d(initial states) as the whole graph sees them, to float64 round-off."""
    hp = tiny_hp(attention_type="bah_mon", model_type="deepvoice")
    B, T_in, n, r, ns = 3, 7, 4, hp.reduction_factor, 2
    w = O.init_weights(hp, ns, 11)
    rs = np.random.RandomState(12)
    ids = rs.randint(1, 20, size=(B, T_in))
    L = np.array([T_in, 5, 6])
    mt, lt = rs.randn(B, n * r, hp.num_mels), rs.randn(B, n * r, hp.num_freq)
    seen = {}
    inner = TF.decoder

    def capturing(wt, hp_, enc, n_, spk, att_init, dec_inits, manual, training, teacher_frames):
        y, al = inner(wt, hp_, enc, n_, spk, att_init, dec_inits, manual, training, teacher_frames)
        for t in [enc, att_init, y] + list(dec_inits):
            t.retain_grad()
        seen.update(enc=enc, att_init=att_init, dec_inits=dec_inits, y=y, teacher=teacher_frames, training=training)
        return y, al

    TF.decoder = capturing
    try:
        _, g, out = TF.train_grads(w, hp, ids, L, mt, lt, speaker_id=np.array([0, 1, 1]), num_speakers=ns)
    finally:
        TF.decoder = inner
    assert seen["training"] is True
    np64 = lambda t: t.detach().numpy()
    inp = {"w": w, "enc": np64(seen["enc"]), "teacher": np64(seen["teacher"]), "dmel": np64(seen["y"].grad), "att_init": np64(seen["att_init"]),
           "dec_inits": [np64(t) for t in seen["dec_inits"]], "spk": None}
    res, _, _ = R.evaluate(hp, inp, torch.float64)
    assert np.array_equal(res["mel"].reshape(out["mel"].shape), out["mel"]) and np.array_equal(res["alignments"], out["alignments"])
    want = {k: v for k, v in g.items() if R.in_scope(k)}
    want.update(denc=np64(seen["enc"].grad), datt_init=np64(seen["att_init"].grad))
    want.update({"ddec_init_%d" % (i + 1): np64(t.grad) for i, t in enumerate(seen["dec_inits"])})
    assert set(want) == set(res) - {"mel", "alignments"} and len(want) > 20
    for k, v in want.items():
        s = float(np.abs(v).max())
        assert s > 0 and float(np.abs(res[k] - v).max()) <= 1e-12 * s, k


def test_monotonic_closed_form_equals_the_recurrence_where_no_clip_acts_and_not_in_gradient_where_one_does():
    def both(T, seed):
        rs = np.random.RandomState(seed)
        outs = []
        for fn in (TF.monotonic_closed_form, TF.monotonic_sequential):
            p = torch.tensor(rs.uniform(0.3, 0.7, size=(2, T)), dtype=torch.float64, requires_grad=True)
            prev = torch.softmax(torch.tensor(rs.randn(2, T), dtype=torch.float64), 1).requires_grad_(True)
            a = fn(p, prev)
            (a * torch.tensor(rs.randn(2, T))).sum().backward()
            outs.append((a.detach().numpy(), p.grad.numpy(), prev.grad.numpy()))
            rs = np.random.RandomState(seed)
        return outs

    (a, dp, dprev), (a2, dp2, dprev2) = both(9, 1)                   # cp >= 0.3^8 = 6.6e-5: no clip
    for x, y in ((a, a2), (dp, dp2), (dprev, dprev2)):
        assert float(np.abs(x - y).max()) <= 1e-12 * float(np.abs(y).max())
    (a, dp, dprev), (a2, dp2, dprev2) = both(72, 2)                  # cp <= 0.7^j < 1e-10 from j = 65 at the latest: the clip acts
    assert float(np.abs(dp - dp2).max()) > 1e-6 * float(np.abs(dp2).max())


NAMES = ("taco_train_debug_decoder", "taco_train_debug_decoder_workspace_bytes", "taco_debug_train_create_host")


def test_the_library_exports_the_hook_and_the_prototypes_carry_it():
    lib = _lib.load_library()
    assert lib.taco_abi_version() == 1
    P, I, S = C.c_void_p, C.c_int, C.c_size_t
    for name in NAMES:
        assert name in _lib.PROTOTYPES and getattr(lib, name)
    fn = lib.taco_train_debug_decoder
    assert fn.restype is C.c_int and list(fn.argtypes) == [P] * 10 + [I] * 3 + [P] * 7 + [S, P]
    fn = lib.taco_train_debug_decoder_workspace_bytes
    assert fn.restype is S and list(fn.argtypes) == [P, I, I, I]


def test_the_header_declares_the_hook_and_its_contract():
    text = open(HEADER).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*size_t\s+taco_train_debug_decoder_workspace_bytes\s*\(([^;]*)\)\s*;\s*int\s+taco_train_debug_decoder\s*\(([^;]*)\)\s*;",
                  text, flags=re.S)
    assert m, "not declared"
    comment = re.sub(r"\s+", " ", m.group(1))
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(3).split(",")]
    assert args == ["taco_train* t", "void* hip_stream", "float* d_params", "float* d_grads", "const float* d_enc_out", "const float* d_teacher",
                    "const float* d_dmel", "const float* d_att_init", "const float* const* d_dec_init", "const float* d_spk_emb", "int B", "int T_in",
                    "int n", "float* d_mel", "float* d_alignments", "float* d_denc", "float* d_datt_init", "float* const* d_ddec_init",
                    "float* d_dspk_emb", "void* d_ws", "size_t ws_bytes", "uint32_t* paths"]
    for word in ("decoder_forward_train", "decoder_backward", "carve_dec_tape", "ADDED", "TACO_ERR_ARG", "TACO_ERR_STATE", "TACO_ERR_UNSUPPORTED",
                 "before the first HIP call", "bits 4-7", "bits 8-11", "bit 12 / 13", "write-through"):
        assert word in comment, word
    assert re.search(r"int\s+taco_debug_train_create_host\s*\(\s*const taco_hparams\* hp,\s*taco_train\*\* out\s*\)\s*;", text)


class _HostTrainer(object):
    def __init__(self, hp, speakers=1):
        self.lib = _lib.load_library()
        self.h = C.c_void_p()
        chp = _lib.to_c_hparams(to_product_hp(hp), speakers)
        _lib.check(self.lib.taco_debug_train_create_host(C.byref(chp), C.byref(self.h)))

    def close(self):
        self.lib.taco_train_destroy(self.h)


def test_argument_errors_return_before_any_device_call():
    """Dummy non-null addresses stand in for device memory on a trainer that never touched a device: validation rejects every one of these
    calls before anything is launched; a call that passes them all is refused because the trainer is host-only."""
    lib = _lib.load_library()
    A = lambda i: (i + 1) << 24                        # 16 MiB apart, 16-byte aligned
    B, T_in, n = 2, 5, 3

    def call(tr, **kw):
        a = dict(t=tr.h if tr else None, params=A(0), grads=A(1), enc=A(2), teacher=A(3), dmel=A(4), att_init=0, dec_init=None, spk=0, B=B, T_in=T_in, n=n,
                 mel=A(5), align=A(6), denc=A(7), datt_init=0, ddec_init=None, dspk=0, ws=A(8), ws_bytes=None, paths=0)
        a.update(kw)
        if a["ws_bytes"] is None:
            a["ws_bytes"] = int(lib.taco_train_debug_decoder_workspace_bytes(a["t"], a["B"], a["T_in"], a["n"])) if tr else 1 << 20
        p = lambda v: C.c_void_p(v) if v else None
        tab = lambda v: None if v is None else (C.c_void_p * len(v))(*v)
        rc = lib.taco_train_debug_decoder(a["t"], None, p(a["params"]), p(a["grads"]), p(a["enc"]), p(a["teacher"]), p(a["dmel"]), p(a["att_init"]),
                                          tab(a["dec_init"]), p(a["spk"]), a["B"], a["T_in"], a["n"], p(a["mel"]), p(a["align"]), p(a["denc"]),
                                          p(a["datt_init"]), tab(a["ddec_init"]), p(a["dspk"]), p(a["ws"]), a["ws_bytes"], p(a["paths"]))
        return rc, lib.taco_last_error()

    assert lib.taco_train_debug_decoder_workspace_bytes(None, B, T_in, n) == 0
    rc, msg = call(None)
    assert rc == _lib.TACO_ERR_ARG and b"null" in msg
    rc = lib.taco_debug_train_create_host(None, None)
    assert rc == _lib.TACO_ERR_ARG

    tr = _HostTrainer(tiny_hp(attention_type="bah_mon"))
    try:
        for bad in (dict(B=0), dict(T_in=0), dict(n=0), dict(B=-1)):
            shape = dict(B=B, T_in=T_in, n=n)
            shape.update(bad)
            assert lib.taco_train_debug_decoder_workspace_bytes(tr.h, shape["B"], shape["T_in"], shape["n"]) == 0
        nb = int(lib.taco_train_debug_decoder_workspace_bytes(tr.h, B, T_in, n))
        assert nb > 0 and nb % 256 == 0
        for k in ("params", "grads", "enc", "teacher", "dmel", "mel", "align", "denc", "ws"):
            rc, msg = call(tr, **{k: 0})
            assert rc == _lib.TACO_ERR_ARG and b"null" in msg, k
        # a gradient output without its input; inputs of another model type
        for kw in (dict(datt_init=A(9)), dict(ddec_init=[A(9), 0]), dict(ddec_init=[0, A(9)], dec_init=[A(10), 0]), dict(dspk=A(9))):
            rc, msg = call(tr, **kw)
            assert rc == _lib.TACO_ERR_ARG and b"without its input" in msg, kw
        for kw in (dict(att_init=A(9)), dict(dec_init=[A(9), 0])):
            rc, msg = call(tr, **kw)
            assert rc == _lib.TACO_ERR_ARG and b"deepvoice" in msg, kw
        rc, msg = call(tr, spk=A(9), dspk=A(10))
        assert rc == _lib.TACO_ERR_ARG and b"simple" in msg
        for kw in (dict(B=0), dict(T_in=0), dict(B=-3), dict(n=0), dict(n=-1)):
            rc, msg = call(tr, ws_bytes=nb, **kw)
            assert rc == _lib.TACO_ERR_ARG and b"bad" in msg, kw
        rc, msg = call(tr, B=65)
        assert rc == _lib.TACO_ERR_UNSUPPORTED and b"64" in msg
        rc, msg = call(tr, n=8)                                       # tiny_hp: max_iters = 7
        assert rc == _lib.TACO_ERR_SHAPE and b"max_iters" in msg
        rc, msg = call(tr, ws=A(8) + 4)
        assert rc == _lib.TACO_ERR_ARG and b"aligned" in msg
        # the trainer as created wants split-bf16 planes, and none were ever generated: stale
        rc, msg = call(tr)
        assert rc == _lib.TACO_ERR_STATE and b"stale" in msg
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0             # the engines that need no planes
        rc, msg = call(tr, T_in=2049)
        assert rc == _lib.TACO_ERR_UNSUPPORTED and b"2048" in msg
        rc, msg = call(tr, ws_bytes=nb - 1)
        assert rc == _lib.TACO_ERR_STATE and b"too small" in msg
        rc, msg = call(tr, ws_bytes=0)
        assert rc == _lib.TACO_ERR_STATE and b"too small" in msg
        # every check passed: only now would the device be touched
        for kw in (dict(), dict(paths=A(11))):
            rc, msg = call(tr, **kw)
            assert rc == _lib.TACO_ERR_STATE and b"host-only" in msg, kw
        # the switches that size the workspace are the trainer's
        assert lib.taco_train_set_deterministic(tr.h, 0) == 0
        assert 0 < int(lib.taco_train_debug_decoder_workspace_bytes(tr.h, B, T_in, n)) < nb
    finally:
        tr.close()

    tr = _HostTrainer(tiny_hp(attention_type="bah", attention_size=1028))          # a multiple of 4 past what the attention kernels hold
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        rc, msg = call(tr)
        assert rc == _lib.TACO_ERR_UNSUPPORTED and b"attention sizes" in msg
    finally:
        tr.close()

    tr = _HostTrainer(tiny_hp(attention_type="bah_norm", model_type="simple"), speakers=2)
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        for kw in (dict(), dict(spk=A(9)), dict(dspk=A(9))):
            rc, msg = call(tr, **kw)
            assert rc == _lib.TACO_ERR_ARG, kw
        rc, msg = call(tr, spk=A(9), dspk=A(10))
        assert rc == _lib.TACO_ERR_STATE and b"host-only" in msg
    finally:
        tr.close()

    tr = _HostTrainer(tiny_hp(attention_type="bah_mon", model_type="deepvoice"), speakers=2)
    try:
        assert lib.taco_train_set_exact_gemm(tr.h, 1) == 0
        rc, msg = call(tr, att_init=A(9), datt_init=A(10), dec_init=[A(11), A(12)], ddec_init=[A(13), 0])
        assert rc == _lib.TACO_ERR_STATE and b"host-only" in msg
        rc, msg = call(tr, att_init=A(9), dec_init=[A(11), 0], ddec_init=[0, A(13)])
        assert rc == _lib.TACO_ERR_ARG and b"layer 2" in msg
    finally:
        tr.close()
