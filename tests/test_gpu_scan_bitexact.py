"""The whole-chip BiGRU scan k_bigru_oct (csrc/taco_bigru_xcd.h) and one whole training step compute, bit for bit, what they computed at the
commit before round 8 -- the round that reordered the GRU gate stages of the persistent decoder to publish r*h first (the update gate's
reduction and sigmoid and the candidate's x-rows behind the publish store) and tried the same order in the scan's gates phases (measured,
not adopted: the scan keeps its order; a later attempt is held to the same bits).  Every value keeps its FMA chain and its reduction tree.
Three scans through the op-level call tools/trace_bigru.py times (taco_bigru_f32 on the post-net's
weights: input projection + scan), and the same three through the training forward's TAPE instantiation (taco_train_debug_bigru: output and
gate tape), all with ragged lengths that include 1 and T and a non-zero initial state, T = 50 (two refills of the 16-step LDS ring):
20 rows on k_bigru_oct<4> (partly filled), 12 rows on k_bigru_oct<2>, 8 rows forced onto k_bigru_oct<1>.
Then one training step at the reference widths (9 rows, T_in 128, T_out 64: the teacher-forced k_decoder_xcd TAPE instantiation and
k_bigru_oct<2, true> inside the whole step), twice, in deterministic mode: losses and gradient bucket.

tests/golden/scan_bitexact.json holds the sha256 of every complete array, recorded from the kernels of the commit before round 8
(tools/make_scan_bitexact_golden.py); scan_bitexact.npz the first and last frames of two rows of every scan array, which says WHERE two
builds differ when the digests do not agree.  Every comparison is for equality."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 50
# name -> (rows, taco_debug_set_persistent mode, units per wave expected)
CASES = {"oct4_20rows": (20, 1, 4), "oct2_12rows": (12, 1, 2), "oct1_8rows": (8, 10, 1)}
TRAIN = {"B": 9, "T_in": 128, "T_out": 64, "seed": 2208}
H = 256


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def sample(a):
    """first and last frames of the first and the last row"""
    return np.ascontiguousarray(a[[0, -1]][:, [0, -1]])


def _hp(max_iters=4):
    import taco_amd
    return taco_amd.hparams.copy(max_iters=max_iters, model_type="single")


def _inputs(B, width):
    """uniform draws only (no libm in the recipe): the scan's input, lengths with 1 and T among them, an initial state"""
    rs = np.random.RandomState(8000 + B)
    x = rs.uniform(-0.6, 0.6, size=(B, T, width)).astype(np.float32)
    lens = rs.randint(1, T + 1, size=B).astype(np.int32)
    lens[0], lens[1], lens[B - 1] = T, 1, 17
    h0 = rs.uniform(-0.5, 0.5, size=(B, 2 * H)).astype(np.float32)
    return x, lens, h0


def run_infer(name):
    """out [B, T, 2H] of taco_bigru_f32 on the post-net's BiGRU"""
    import torch
    import taco_amd
    from util import dev, ptr, stream
    B, mode, upw = CASES[name]
    hp = _hp()
    m = taco_amd.create_model(hp)
    m.load_weights(taco_amd.weights.random_weights(hp, 1, seed=1234))
    m.initialize(None, None, 1, None, device="cuda:0")
    L = taco_amd._lib
    L.check(m._lib.taco_debug_set_persistent(m._handle, mode))
    assert "post-net scan: persistent k_bigru_oct<%d>" % upw in m.engine_plan(B, 128, T), m.engine_plan(B, 128, T)
    x, lens, h0 = _inputs(B, H)
    xd, ld, hd = dev(x), dev(lens), dev(h0)
    out = torch.full((B, T, 2 * H), float("nan"), device="cuda")
    n = int(m._lib.taco_stage_workspace_bytes(m._handle, B, T))
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    L.check(m._lib.taco_bigru_f32(m._handle, stream(), b"post_cbhg", ptr(xd), ptr(ld), ptr(hd), B, T, ptr(out), ptr(ws), n))
    torch.cuda.synchronize()
    m.check_device_errors()
    got = out.cpu().numpy()
    m.close()
    return got


def run_tape(name):
    """(out [B, T, 2H], gate tape [B, T, 6H]) of the training forward's scan, the hoisted projection given directly"""
    import torch
    import taco_amd
    from util import dev, ptr, stream
    B, mode, upw = CASES[name]
    hp = _hp()
    tr = taco_amd.Trainer(hp, taco_amd.weights.random_weights(hp, 1, seed=1234))
    mh = C.c_void_p(tr._lib.taco_train_model(tr._h))
    taco_amd._lib.check(tr._lib.taco_debug_set_persistent(mh, mode))
    xproj, lens, h0 = _inputs(B, 6 * H)
    dout = np.random.RandomState(8100 + B).uniform(-1.0, 1.0, size=(B, T, 2 * H)).astype(np.float32)
    xd, ld, hd, dd = dev(xproj), dev(lens), dev(h0), dev(dout)
    scratch = torch.empty((2 << 20,), dtype=torch.uint8, device="cuda")
    o = {k: torch.zeros(s, device="cuda") for k, s in (("out", (B, T, 2 * H)), ("gsave", (B, T, 6 * H)), ("dg", (B, T, 6 * H)),
                                                       ("rh", (B, T, 2 * H)), ("dh0", (B, 2 * H)))}
    taco_amd._lib.check(tr._lib.taco_train_debug_bigru(tr._h, stream(), ptr(xd), ptr(ld), ptr(hd), ptr(dd), B, T, 1, ptr(o["out"]), ptr(o["gsave"]),
                                                       ptr(o["dg"]), ptr(o["rh"]), ptr(o["dh0"]), ptr(scratch), scratch.numel()))
    torch.cuda.synchronize()
    tr.check_device_errors()
    got = o["out"].cpu().numpy(), o["gsave"].cpu().numpy()
    tr.close()
    return got


def run_train():
    """[(losses, gradient bucket)] of two identical steps of one trainer, deterministic mode"""
    import torch
    import taco_amd
    import taco_oracle as O
    B, T_in, T_out, seed = TRAIN["B"], TRAIN["T_in"], TRAIN["T_out"], TRAIN["seed"]
    hp = _hp(T_out // 4)
    ids, L = O.synthetic_inputs(B, T_in, seed, ragged=True)
    rs = np.random.RandomState(seed)
    mt, lt = rs.rand(B, T_out, hp.num_mels), rs.rand(B, T_out, hp.num_freq)
    tr = taco_amd.Trainer(hp, taco_amd.weights.random_weights(hp, 1, seed=seed))
    tr.set_deterministic(True)
    res = []
    for _ in range(2):
        losses = tr.forward_backward(ids, L, mt, lt, freeze_moving_averages=True)
        torch.cuda.synchronize()
        tr.check_device_errors()
        res.append((losses.cpu().numpy().astype(np.float32), tr.grads.detach().cpu().numpy()))
    tr.close()
    return res


def _gold():
    return json.load(open(os.path.join(GOLDEN, "scan_bitexact.json"))), np.load(os.path.join(GOLDEN, "scan_bitexact.npz"))


def _same(name, a, doc, z):
    assert list(a.shape) == doc[name + "_shape"]
    s, g = sample(a).view(np.uint32), z[name].view(np.uint32)
    assert np.array_equal(s, g), "%s: %d of %d sampled words differ (first / last frames of the first / last row)" % (name, int((s != g).sum()), s.size)
    assert digest(a) == doc[name + "_sha256"], "%s differs outside the sampled frames" % name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_output_is_bit_identical_to_the_kernel_before_round_8(name):
    doc, z = _gold()
    _same(name + "/out", run_infer(name), doc, z)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_scan_gate_tape_is_bit_identical_to_the_kernel_before_round_8(name):
    doc, z = _gold()
    out, gsave = run_tape(name)
    _same(name + "/tape_out", out, doc, z)
    _same(name + "/tape_gates", gsave, doc, z)


@pytest.mark.gpu
def test_training_step_is_bit_identical_to_the_kernels_before_round_8():
    doc, _ = _gold()
    (l1, g1), (l2, g2) = run_train()
    assert np.isfinite(l1).all() and np.isfinite(g1).all()
    assert np.array_equal(l1.view(np.uint32), l2.view(np.uint32)) and np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), "two identical steps differ"
    assert [int(v) for v in l1.view(np.uint32)] == doc["train/losses_bits"], (l1.tolist(), doc["train/losses"])
    assert list(g1.shape) == doc["train/grads_shape"]
    assert digest(g1) == doc["train/grads_sha256"], "the gradient bucket differs"
