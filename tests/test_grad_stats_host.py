"""Training summaries (add_stats, train.py:50-77) -- the host side of the per-variable gradient norms: the exported symbols, their
ctypes prototypes and declarations, every argument error (all returned before any HIP call, so they work without a GPU), the piece
table of taco_segment_norms as its host-only builder makes it, and the Python surface (Trainer.trainable, Tacotron.add_stats) on stub
objects.  The kernels are held to float64 NumPy in tests/test_gpu_grad_stats.py."""
import ctypes as C
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import taco_amd
from taco_amd import _lib
from taco_amd import trainer as T
from taco_amd.hparams import hparams as default_hparams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["taco_segment_norms", "taco_segnorm_piece_floats", "taco_segnorm_plan_create", "taco_segnorm_plan_destroy", "taco_train_grad_norms"]
A, O, S, X = 1 << 20, 1 << 24, 1 << 25, 1 << 26          # dummy device addresses, 16 MiB or more apart


def _u64(v):
    return (C.c_uint64 * len(v))(*v)


def _u8(v):
    return None if v is None else (C.c_uint8 * len(v))(*v)


def _pieces(offsets, skip=None, cap=None):
    """(rc, [(begin, len, seg)], n_pieces) of taco_debug_segnorm_pieces"""
    lib = _lib.load_library()
    n_seg = len(offsets) - 1
    cap = 4096 if cap is None else cap
    room = cap + 8                                                    # guard entries behind `cap`: they must stay untouched
    b, l, s = (C.c_uint64 * room)(*([2 ** 64 - 1] * room)), (C.c_int32 * room)(*([-7] * room)), (C.c_int32 * room)(*([-7] * room))
    n = C.c_int(-1)
    rc = lib.taco_debug_segnorm_pieces(_u64(offsets), n_seg, _u8(skip), b, l, s, cap, C.byref(n))
    assert all(b[i] == 2 ** 64 - 1 and l[i] == -7 and s[i] == -7 for i in range(cap, room)), "written past cap"
    got = [(int(b[i]), int(l[i]), int(s[i])) for i in range(max(n.value, 0))] if rc == 0 else []
    return rc, got, n.value


def test_the_library_exports_the_symbols_and_the_prototypes_match():
    lib = _lib.load_library()
    assert lib.taco_abi_version() == 1                                # additive: the version stays
    P, I, Z = C.c_void_p, C.c_int, C.c_size_t
    want = {"taco_segment_norms": (I, [P, P, P, Z, P, P, P]),
            "taco_segnorm_piece_floats": (I, []),
            "taco_segnorm_plan_create": (I, [C.POINTER(C.c_uint64), I, C.POINTER(C.c_uint8), I, C.POINTER(P)]),
            "taco_segnorm_plan_destroy": (None, [P]),
            "taco_train_grad_norms": (I, [P, P, P, P, P, P]),
            "taco_debug_segnorm_pieces": (I, [C.POINTER(C.c_uint64), I, C.POINTER(C.c_uint8), C.POINTER(C.c_uint64), C.POINTER(C.c_int32),
                                              C.POINTER(C.c_int32), I, C.POINTER(I)])}
    for name, (res, args) in want.items():
        assert name in _lib.PROTOTYPES, name
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    P_ = lib.taco_segnorm_piece_floats()
    assert P_ >= 1024 and P_ % 1024 == 0                              # whole 16-byte loads for every thread of a 256-thread workgroup


def test_the_header_declares_them_after_the_adam_step_with_the_rules_in_the_comment():
    text = open(os.path.join(ROOT, "include", "taco_abi.h")).read()
    bare = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    order = [x.group(1) for x in re.finditer(r"\b(?:int|void|size_t)\s+(taco_\w+)\s*\(", bare)]
    assert order[order.index("taco_adam_step_f32") + 1] == "taco_segment_norms"
    for name in NEW:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:typedef struct taco_segnorm_plan taco_segnorm_plan;\s*)?(?:int|void)\s+%s\s*\(" % name,
                      text, flags=re.S)
        assert m, "%s: no comment directly in front of the declaration" % name
        assert "train.py:50-77" in re.sub(r"\s+", " ", m.group(1)), name
    for name in ("taco_segment_norms", "taco_train_grad_norms"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:typedef struct taco_segnorm_plan taco_segnorm_plan;\s*)?int\s+%s\s*\(([^;]*)\)\s*;" % name,
                      text, flags=re.S)
        c = re.sub(r"\s+", " ", m.group(1))
        assert "train.py:156" in c and "'stats'" in c and "'train'" in c and "never executes" in c, name       # the caveat
        assert "UNCLIPPED" in c and "tacotron.py:328-330" in c, name
        assert "double" in c and "NaN" in c and "skip" in c, name
    c = re.sub(r"\s+", " ", re.search(r"/\*((?:(?!\*/).)*)\*/\s*typedef struct taco_segnorm_plan", text, flags=re.S).group(1))
    assert "ties go to the first index" in c and "first NaN segment" in c and "tf.reduce_max" in c and "+inf" in c
    assert "atomics" in c and "capturable" in c and "before any HIP call" in c
    args = re.sub(r"/\*.*?\*/", "", re.search(r"int\s+taco_segment_norms\s*\(([^;]*)\)\s*;", text, flags=re.S).group(1), flags=re.S).split(",")
    assert [re.sub(r"\s+", " ", a).strip() for a in args] == ["const taco_segnorm_plan* plan", "void* hip_stream", "const float* d_flat", "size_t n",
                                                             "float* d_norms", "float* d_stats", "int32_t* d_argmax"]
    dbg = open(os.path.join(ROOT, "include", "taco_debug.h")).read()
    assert "taco_debug_segnorm_pieces" in dbg and "taco_debug_segnorm_pieces" not in text


def test_plan_create_argument_errors_come_before_any_device_call():
    lib = _lib.load_library()
    out = C.c_void_p(0)

    def create(off, n_seg=None, skip=None, o=out):
        rc = lib.taco_segnorm_plan_create(None if off is None else _u64(off), len(off) - 1 if n_seg is None else n_seg, _u8(skip), 0,
                                          None if o is None else C.byref(o))
        return rc, lib.taco_last_error()

    rc, msg = create(None, n_seg=1)
    assert rc == _lib.TACO_ERR_ARG and b"null" in msg
    rc, msg = create([0, 4], o=None)
    assert rc == _lib.TACO_ERR_ARG and b"null" in msg
    for n_seg in (0, -1, -2 ** 31):
        rc, msg = create([0, 4], n_seg=n_seg)
        assert rc == _lib.TACO_ERR_ARG and b">= 1" in msg, n_seg
    for off in ([4, 0], [0, 8, 7], [0, 8, 8, 2 ** 40, 2 ** 40 - 1]):
        rc, msg = create(off)
        assert rc == _lib.TACO_ERR_ARG and b"ascend" in msg, off
    assert not out.value                                              # nothing was made


def test_segment_norms_argument_errors_come_before_any_device_call():
    """A plan that stays on the host stands in for a device plan; dummy non-null addresses stand in for device memory."""
    lib = _lib.load_library()
    plan = C.c_void_p(0)
    off = [1, 1, 5, 105]                                              # three segments, the table ends at element 105
    assert lib.taco_debug_segnorm_plan_create_host(_u64(off), 3, None, C.byref(plan)) == 0 and plan.value
    try:
        def call(p=plan, x=A, n=105, norms=O, stats=S, am=X):
            v = lambda a: C.c_void_p(a) if a else None
            rc = lib.taco_segment_norms(p if p else None, None, v(x), n, v(norms), v(stats), v(am))
            return rc, lib.taco_last_error()

        for kw in (dict(p=None), dict(x=0), dict(norms=0), dict(stats=0), dict(x=0, norms=0, stats=0)):
            rc, msg = call(**kw)
            assert rc == _lib.TACO_ERR_ARG and b"null" in msg, kw
        for n in (104, 5, 0):
            rc, msg = call(n=n)
            assert rc == _lib.TACO_ERR_ARG and b"105" in msg, n
        rc, msg = call(x=A + 2)
        assert rc == _lib.TACO_ERR_ARG and b"aligned" in msg
        nbytes = 105 * 4
        for norms in (A, A + 4, A + nbytes - 4, A - 3 * 4 + 4):       # [3] floats of norms against [105] floats of input
            rc, msg = call(norms=norms)
            assert rc == _lib.TACO_ERR_ARG and b"d_norms" in msg and b"overlap" in msg, norms
        for stats in (A, A + nbytes - 4, A - 4):
            rc, msg = call(stats=stats)
            assert rc == _lib.TACO_ERR_ARG and b"d_stats" in msg and b"overlap" in msg, stats
        rc, msg = call(am=A + 8)
        assert rc == _lib.TACO_ERR_ARG and b"d_argmax" in msg and b"overlap" in msg
        # buffers that touch the input but do not overlap it pass every check; so does a null d_argmax.  The host-only plan then
        # refuses to run: still no device call
        for kw in (dict(norms=A + nbytes), dict(norms=A - 12), dict(stats=A - 8), dict(am=0), dict(n=106)):
            rc, msg = call(**kw)
            assert rc == _lib.TACO_ERR_STATE and b"host-only" in msg, kw
    finally:
        lib.taco_segnorm_plan_destroy(plan)
    lib.taco_segnorm_plan_destroy(None)                               # as free(NULL)


def test_train_grad_norms_refuses_null_pointers_before_it_touches_the_trainer():
    """Without a GPU there is no trainer: a dummy handle stands in, which the null checks never read.  (The overlap checks need the
    trainer's size: tests/test_gpu_grad_stats.py.)"""
    lib = _lib.load_library()
    v = lambda a: C.c_void_p(a) if a else None
    for t, g, n, s in ((0, A, O, S), (X, 0, O, S), (X, A, 0, S), (X, A, O, 0), (0, 0, 0, 0)):
        rc = lib.taco_train_grad_norms(v(t), None, v(g), v(n), v(s), None)
        assert rc == _lib.TACO_ERR_ARG and b"null" in lib.taco_last_error(), (t, g, n, s)


def _check_table(offsets, skip, pieces, P):
    n_seg = len(offsets) - 1
    assert all(1 <= l <= P for _, l, _ in pieces)
    assert [b for b, _, _ in pieces] == sorted(b for b, _, _ in pieces)            # ascending
    for s in range(n_seg):
        mine = [(b, l) for b, l, g in pieces if g == s]
        if skip is not None and skip[s]:
            assert mine == [], "skipped segment %d has pieces" % s
            continue
        pos = offsets[s]
        for b, l in mine:                                                          # they tile the segment exactly, in order
            assert b == pos and b + l <= offsets[s + 1]
            pos += l
        assert pos == offsets[s + 1], s
        assert len(mine) == -(-(offsets[s + 1] - offsets[s]) // P)                  # as few as P allows
    assert all(0 <= g < n_seg for _, _, g in pieces)


def test_piece_table_on_hand_written_offsets():
    lib = _lib.load_library()
    P = lib.taco_segnorm_piece_floats()
    lens = [0, 1, 2, 3, P - 1, P, P + 1, 2 * P + 3, 0, 0, 1, 5, 3 * P, 1, 0]
    for first in (0, 1, 3, 2 ** 33 + 1):                              # an unaligned first offset; one beyond 32 bits
        off = list(np.cumsum([first] + lens).astype(object))
        rc, pieces, n = _pieces(off)
        assert rc == 0 and n == len(pieces)
        _check_table(off, None, pieces, P)
        want = {P - 1: [P - 1], P: [P], P + 1: [P, 1], 2 * P + 3: [P, P, 3], 3 * P: [P, P, P]}
        for s, ln in enumerate(lens):
            if ln in want:
                assert [l for _, l, g in pieces if g == s] == want[ln], ln
        skip = [0] * len(lens)
        for s in (0, 3, 7, 12, 14):                                   # an empty one, a short one, the two long ones, the last
            skip[s] = 1
        rc, skipped, n = _pieces(off, skip)
        assert rc == 0
        _check_table(off, skip, skipped, P)
        assert skipped == [p for p in pieces if not skip[p[2]]]       # skipping a segment changes nothing about the others
    rc, pieces, n = _pieces([7, 7, 7])                                # nothing but empty segments: a valid table without pieces
    assert rc == 0 and pieces == [] and n == 0
    rc, pieces, n = _pieces([0, 5, 9], [1, 1])
    assert rc == 0 and pieces == [] and n == 0
    rc, pieces, n = _pieces([0, 1])
    assert rc == 0 and pieces == [(0, 1, 0)]


def test_a_cap_that_is_too_small_is_an_error_and_not_an_overrun():
    lib = _lib.load_library()
    P = lib.taco_segnorm_piece_floats()
    off = [1, 1 + 2 * P + 3, 1 + 2 * P + 4]                           # 3 + 1 pieces
    for cap in (0, 1, 3):
        rc, pieces, n = _pieces(off, cap=cap)                         # (_pieces checks the guard entries behind cap)
        assert rc == _lib.TACO_ERR_ARG and b"room for" in lib.taco_last_error() and n == 4, cap
    rc, pieces, n = _pieces(off, cap=4)
    assert rc == 0 and n == 4 and [l for _, l, _ in pieces] == [P, P, 3, 1]
    rc, pieces, n = _pieces([0, 4, 2])
    assert rc == _lib.TACO_ERR_ARG and b"ascend" in lib.taco_last_error()


def test_trainable_leaves_out_the_moving_statistics_and_maps_one_to_one_onto_tf_variables():
    tr = T.Trainer.__new__(T.Trainer)                                 # a stub: no device, no library handle
    tr.spec = [("embedding", (80, 256)), ("prenet/dense_1/kernel", (256, 256)), ("encoder_cbhg/proj_1/gamma", (128,)),
               ("encoder_cbhg/proj_1/moving_mean", (128,)), ("encoder_cbhg/proj_1/moving_variance", (128,)),
               ("attention/attention_score_bias", ()), ("linear/bias", (1025,))]
    assert tr.trainable == ["embedding", "prenet/dense_1/kernel", "encoder_cbhg/proj_1/gamma", "attention/attention_score_bias", "linear/bias"]
    assert "attention/attention_v" in T.Trainer.trainable.__doc__      # the exception to the scope table is listed
    # the real specs (they come from the library, which needs no device for them): every trainable name maps to its own TF variable
    from taco_amd.weights import weight_spec
    import copy
    for ns, mt, at in ((1, "single", "bah_mon"), (4, "deepvoice", "bah_norm"), (3, "simple", "bah")):
        hp = copy.deepcopy(default_hparams)
        hp.model_type, hp.attention_type = mt, at
        tr.spec = weight_spec(hp, ns)
        names = tr.trainable
        assert len(names) + 2 * sum(n.endswith("/moving_mean") for n, _ in tr.spec) == len(tr.spec)
        assert not [n for n in names if "moving_" in n]
        tf_names = [T.tf_variable_name(n) for n in names]
        assert len(set(tf_names)) == len(tf_names), (mt, at)
        assert [n for n in names if n.startswith("attention/attention_")]           # the listed exception occurs in every model
    with pytest.raises(KeyError):
        T.tf_variable_name("no_such_scope/kernel")


class _StubTrainer(object):
    def __init__(self, have):
        self.have_gradients, self.learning_rate, self.calls = have, 0.00125, 0

    def gradient_stats(self):
        self.calls += 1
        return {"max_gradient_norm": 3.5, "argmax": "linear/kernel", "global_norm": 4.0, "norms": {}}


def _stub_model(trainer, mel, lin, lwc):
    m = taco_amd.Tacotron(default_hparams)
    m._trainer = trainer
    m.mel_loss, m.linear_loss, m.loss_without_coeff, m.loss = np.float32(mel), np.float32(lin), np.float32(lwc), np.float32(9.0)
    return m


def test_add_stats_tag_names_and_order_on_stub_models():
    tr = _StubTrainer(True)
    model, test_model = _stub_model(tr, 0.25, 0.5, 0.75), _stub_model(tr, 0.375, 0.75, 1.125)
    s = model.add_stats()                                             # scope 'train' is the reference's default
    assert isinstance(s, OrderedDict)
    assert list(s.items()) == [("train/loss_mel", 0.25), ("train/loss_linear", 0.5), ("train/loss", 0.75),     # 'loss' is loss_without_coeff
                               ("train/learning_rate", 0.00125), ("train/max_gradient_norm", 3.5)]
    assert all(type(v) is float for v in s.values()) and tr.calls == 1
    s = model.add_stats(scope_name="stats")                           # what train.py:156 asks for: no gradient scalars
    assert list(s) == ["stats/loss_mel", "stats/loss_linear", "stats/loss"] and tr.calls == 1
    s = test_model.add_stats(model, "test")                           # train.py:168
    assert list(s) == ["test/loss_mel", "test/loss_linear", "test/loss", "gap_test-train/loss_mel", "gap_test-train/loss_linear",
                       "gap_test-train/loss"]
    assert (s["gap_test-train/loss_mel"], s["gap_test-train/loss_linear"], s["gap_test-train/loss"]) == (0.125, 0.25, 0.375)
    assert tr.calls == 1
    s = model.add_stats(test_model)                                   # both extras at once, in the reference's order
    assert list(s)[3:] == ["train/learning_rate", "train/max_gradient_norm", "gap_test-train/loss_mel", "gap_test-train/loss_linear",
                           "gap_test-train/loss"]
    assert s["gap_test-train/loss"] == -0.375


def test_add_stats_scope_train_needs_a_backward_pass():
    tr = _StubTrainer(False)
    model = _stub_model(tr, 0.25, 0.5, 0.75)
    with pytest.raises(_lib.TacoError) as e:
        model.add_stats()
    assert e.value.code == _lib.TACO_ERR_STATE and tr.calls == 0
    assert list(model.add_stats(scope_name="test")) == ["test/loss_mel", "test/loss_linear", "test/loss"]     # needs no gradients
    tr.have_gradients = True
    assert model.add_stats()["train/max_gradient_norm"] == 3.5
