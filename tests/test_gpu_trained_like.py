"""Parity against the float64 oracle on weights without a constant vector (tests/trained_like.py).

Every other weight set of the suite has all-1.0 GRU gate biases, all-(-1.0) highway T biases and (almost everywhere) a zero score bias, so a
bias read through a wrong index -- r and u halves swapped, a column off, the other direction's or layer's vector, a wave reading its
neighbour's column -- changes no output there.  With trained_like weights each such mistake moves mel, linear or alignments by more than
twenty times the bars held here (tests/test_trained_like_host.py measures it on the oracle, case by case).  The whole forward per engine
and arithmetic level, the BiGRU scans alone per kernel, the decoder cells and the highway layer alone, and the training forward before and
after a step that rebuilds the packs on the device.  Every test prints the max|err| it measured before it asserts."""
import functools

import numpy as np
import pytest

import taco_oracle as O
from trained_like import trained_like
from util import tiny_hp, build_model, to_product_hp, dev, ptr, stream, maxabs, argmax_detail

# name -> (widths, model_type, attention_type, speakers, B, T_in, decoder steps, seed); init_weights(seed), trained_like(seed + 1), synthetic_inputs(seed + 2, ragged).
# The seeds satisfy what tests/test_trained_like_host.py asserts on the oracle alone: no step masked by the arg-max floor, the top two
# positions of every bah_mon step at least 1e-4 of the peak apart, and every bias mutation worth at least ten bars.
FORWARD_CASES = {
    "ref_B8": ("ref", "single", "bah_mon", 1, 8, 24, 19, 77),           # T_mel 76: no multiple of 64.  One row per group
    "ref_B12": ("ref", "single", "bah_mon", 1, 12, 20, 5, 177),         # two rows per group, k_bigru_oct<2>
    "simple_B20": ("ref", "simple", "bah", 3, 20, 20, 5, 277),          # four rows per group, k_bigru_oct<4>, the row-bias table with speaker terms
    "deepvoice_B33": ("ref", "deepvoice", "bah_norm", 3, 33, 20, 4, 377),      # eight rows per group, k_bigru_duo<8>, attention_b, initial states
    "tiny_bah_mon": ("tiny", "single", "bah_mon", 1, 3, 13, 7, 477),    # the launch-per-stage kernels at widths outside the presets
    "tiny_bah": ("tiny", "single", "bah", 1, 3, 13, 7, 477),
    "tiny_bah_norm": ("tiny", "single", "bah_norm", 1, 3, 13, 7, 477),
}
BAR = {"ref": 1e-3, "tiny": 2e-4}      # on mel, linear and alignments: test_gpu_e2e.py's bars at the reference widths (C1, C3) and at tiny_hp
ARRAYS = ("mel", "linear", "alignments")


@functools.lru_cache(maxsize=None)
def forward_case(name):
    """(ohp, speakers, init_weights, trained_like weights, ids, lengths, speaker ids or None, bar) of a FORWARD_CASES entry"""
    widths, mt, atype, ns, B, T_in, n, seed = FORWARD_CASES[name]
    if widths == "tiny":
        ohp = tiny_hp(attention_type=atype, max_iters=n)
    else:
        ohp = O.OracleHParams(max_iters=n, model_type=mt, attention_type=atype)
    w0 = O.init_weights(ohp, ns, seed)
    ids, L = O.synthetic_inputs(B, T_in, seed + 2, ragged=True)
    spk = (np.arange(B) % ns).astype(np.int32) if ns > 1 else None
    return ohp, ns, w0, trained_like(w0, seed + 1), ids, L, spk, BAR[widths]


def oracle_forward(name, w):
    ohp, ns, _, _, ids, L, spk, _ = forward_case(name)
    return O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, honor_stop=False)


@functools.lru_cache(maxsize=None)
def oracle_reference(name):
    return oracle_forward(name, forward_case(name)[3])


def _forward_infer(m, ohp, ids, L, spk):
    """one eager taco_forward_infer: (mel, linear, alignments) on the host"""
    import torch
    import taco_amd
    B, T_in = ids.shape
    n, T_mel = ohp.max_iters, ohp.max_iters * ohp.reduction_factor
    idd, Ld, sd = dev(ids), dev(L), (dev(spk) if spk is not None else None)
    nb = int(m._lib.taco_workspace_bytes(m._handle, B, T_in, n))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    mel = torch.full((B, T_mel, ohp.num_mels), float("nan"), device="cuda")
    lin = torch.full((B, T_mel, ohp.num_freq), float("nan"), device="cuda")
    al = torch.full((B, T_in, n), float("nan"), device="cuda")
    stop = torch.zeros((1,), dtype=torch.int32, device="cuda")
    taco_amd._lib.check(m._lib.taco_forward_infer(m._handle, stream(), ptr(idd), ptr(Ld), ptr(sd), B, T_in, n,
                                                  ptr(None), ptr(mel), ptr(lin), ptr(al), ptr(stop), ptr(ws), nb))
    torch.cuda.synchronize()
    m.check_device_errors()
    return tuple(t.cpu().numpy() for t in (mel, lin, al))


def _judge(tag, hip, ref, bar):
    """test_gpu_e2e._check's criteria, and no step masked by the arg-max floor.  Prints the figures, returns what is wrong (a list)."""
    bad = []
    errs = []
    for a, k in zip(hip, ARRAYS):
        if a.shape != ref[k].shape:
            return ["%s: %s has shape %s, the oracle's %s" % (tag, k, a.shape, ref[k].shape)]
        errs.append(maxabs(a, ref[k]) if np.isfinite(a).all() else float("inf"))
    d = argmax_detail(hip[2], ref["alignments"])
    print("%-58s max|err| mel %.2e  linear %.2e  alignments %.2e  (bar %.0e); arg-max: %d steps, %d masked, %d excused as ties, %d mismatches"
          % (tag, errs[0], errs[1], errs[2], bar, d["steps"], d["masked_by_floor"], d["excused_as_ties"], d["mismatch"]))
    bad += ["%s: %s off by %.3e (bar %.0e)" % (tag, k, e, bar) for k, e in zip(ARRAYS, errs) if not e < bar]
    if d["mismatch"]:
        bad.append("%s: alignment argmax differs at %d of %d steps" % (tag, d["mismatch"], d["compared"]))
    if d["masked_by_floor"]:
        bad.append("%s: %d steps masked by the arg-max floor" % (tag, d["masked_by_floor"]))
    return bad


def _plan_holds(plan, present, absent=()):
    return ["engine_plan lacks %r: %s" % (s, plan) for s in present if s not in plan] + ["engine_plan holds %r: %s" % (s, plan) for s in absent if s in plan]


FUSED_FF = ["k_cbhg_front<", "k_pointwise_chain<", "(the last projection in its entry)"]
# arm -> (taco_debug_set_bf3 mode, decoder engine, fuse_concat, fuse_prenet, words engine_plan must hold, words it must not hold)
REF_B8_ARMS = {
    "default (bf16 x 3, fused front and chain)": (1, 1, 1, 1, ["persistent k_decoder_xcd<1>", "post-net scan: persistent k_bigru_duo<1>", "encoder scan: k_bigru_quad"] + FUSED_FF, [" -- no "]),
    "per-layer k_gemm_bf3 (mode 29)": (29, 1, 1, 1, ["persistent k_decoder_xcd<1>", "point-wise layers on k_gemm_bf3 "], ["k_pointwise_chain<", "k_cbhg_front<", "X6"]),
    "exact fp32, per-layer k_gemm (mode 0)": (0, 1, 1, 1, ["persistent k_decoder_xcd<1>", "exact-fp32 MFMA (k_gemm)", "point-wise layers on k_gemm "], ["k_pointwise_chain<", "k_cbhg_front<", "k_gemm_bf3"]),
    "launch per stage, folds on": (1, 0, 1, 1, ["decoder loop: one launch per stage -- switched off", "post-net scan: resident per-row kernels -- switched off"] + FUSED_FF, []),
    "launch per stage, concat projection unfolded": (1, 0, 0, 1, ["decoder loop: one launch per stage -- switched off"], []),
    "launch per stage, prenet layer 1 unfolded": (1, 0, 1, 0, ["decoder loop: one launch per stage -- switched off"], []),
}


@pytest.mark.gpu
def test_forward_ref_B8_every_engine_and_arithmetic_level():
    """single / bah_mon, B 8, T_in 24, 19 steps (T_mel 76) at the reference widths: k_decoder_xcd<1> (own-column gate biases, the folded
    GRU-1 bias), k_bigru_quad, k_bigru_duo<1>, k_cbhg_front and k_pointwise_chain (T bias inside the chain); taco_debug_set_bf3 29 and 0 put
    the T bias into the epilogues of the per-layer k_gemm_bf3 / k_gemm launches; with the persistent decoder off the launch-per-stage cells and
    k_bigru_resw run, with the folded GRU-1 bias (default) and the unfolded one, and prenet layer 1 folded and not.  All against the oracle."""
    import taco_amd
    check = taco_amd._lib.check
    ohp, ns, _, w, ids, L, spk, bar = forward_case("ref_B8")
    ref = oracle_reference("ref_B8")
    m = build_model(ohp, w, num_speakers=ns)
    bad = []
    try:
        for arm, (bf3, engine, fc, fp, present, absent) in REF_B8_ARMS.items():
            check(m._lib.taco_debug_set_bf3(m._handle, bf3, 0))
            check(m._lib.taco_debug_set_decoder_persist(m._handle, engine, 0))
            check(m._lib.taco_debug_set_fuse_concat(m._handle, fc))
            check(m._lib.taco_debug_set_fuse_prenet(m._handle, fp))
            bad += _plan_holds(m.engine_plan(8, 24), present, absent)
            bad += _judge("ref_B8, " + arm, _forward_infer(m, ohp, ids, L, spk), ref, bar)
            if engine:
                info = m.decoder_engine_info()
                if not (info["has_pack"] and info["protocol"] in (1, 2)):
                    bad.append("%s: the persistent decoder did not run: %s" % (arm, info))
    finally:
        m._lib.taco_debug_set_bf3(m._handle, 1, 0)
        m._lib.taco_debug_set_decoder_persist(m._handle, 1, 0)
        m._lib.taco_debug_set_fuse_concat(m._handle, 1)
        m._lib.taco_debug_set_fuse_prenet(m._handle, 1)
        m.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("name,present", [
    ("ref_B12", ["persistent k_decoder_xcd<2>", "post-net scan: persistent k_bigru_oct<2>", "encoder scan: k_bigru_quad"] + FUSED_FF),
    ("simple_B20", ["persistent k_decoder_xcd<4>", "post-net scan: persistent k_bigru_oct<4>", "encoder scan: k_bigru_quad"] + FUSED_FF),
    ("deepvoice_B33", ["persistent k_decoder_xcd<8>", "post-net scan: persistent k_bigru_duo<8>", "encoder scan: k_bigru_quad"] + FUSED_FF),
    ("tiny_bah_mon", ["decoder loop: one launch per stage -- widths outside the presets", "point-wise layers on k_gemm_bf3 "]),
    ("tiny_bah", ["decoder loop: one launch per stage -- widths outside the presets", "point-wise layers on k_gemm_bf3 "]),
    ("tiny_bah_norm", ["decoder loop: one launch per stage -- widths outside the presets", "point-wise layers on k_gemm_bf3 "]),
])
def test_forward_rows_per_group_model_types_and_tiny_widths(name, present):
    """The other instantiations, each at the smallest batch that reaches it: two, four and eight rows per group of the persistent decoder
    (k_bigru_oct<2>, k_bigru_oct<4>, k_bigru_duo<8> behind it), 'simple' with speaker terms in the row-bias table, deepvoice with initial
    states and bah_norm's attention_b; and the launch-per-stage kernels at widths outside the presets under the three attention types."""
    ohp, ns, _, w, ids, L, spk, bar = forward_case(name)
    ref = oracle_reference(name)
    m = build_model(ohp, w, num_speakers=ns)
    try:
        plan = m.engine_plan(ids.shape[0], ids.shape[1])
        bad = _plan_holds(plan, present)
        bad += _judge(name, _forward_infer(m, ohp, ids, L, spk), ref, bar)
        if FORWARD_CASES[name][0] == "ref":
            info = m.decoder_engine_info()
            if not (info["has_pack"] and info["protocol"] in (1, 2)):
                bad.append("the persistent decoder did not run: %s" % info)
    finally:
        m.close()
    assert not bad, "\n".join(bad)


# ---- the scans, the cells and the highway layer alone ----

@pytest.fixture(scope="module")
def ref_model():
    """the reference widths on ref_B8's trained_like weights"""
    ohp, ns, _, w, _, _, _, _ = forward_case("ref_B8")
    m = build_model(ohp, w, num_speakers=ns)
    yield ohp, w, m
    m.close()


SCAN_T = 35      # two refills of the whole-chip scans' 16-step ring, and three steps


@functools.lru_cache(maxsize=None)
def scan_case(scope, B):
    """(x, lengths, initial state, float64 reference) of a scan: 0.5 * randn inputs, ragged lengths with 1 and T among them, a non-zero state"""
    ohp, _, _, w, _, _, _, _ = forward_case("ref_B8")
    H = ohp.post_rnn_size if scope == "post_cbhg" else ohp.enc_rnn_size
    rs = np.random.RandomState(1000 + B + H)
    x = rs.randn(B, SCAN_T, H) * 0.5
    lens = rs.randint(1, SCAN_T + 1, size=B).astype(np.int32)
    lens[0], lens[1] = SCAN_T, 1
    init = rs.randn(B, 2 * H) * 0.5
    return x, lens, init, O.bidirectional_gru(x, lens, w, scope + "/bigru", init)


def _scan_words(scope, persist, B):
    """what engine_plan says about this scan (a whole MI355X)"""
    if scope == "encoder_cbhg":
        return "encoder scan: k_bigru_quad" if persist == 1 else "encoder scan: k_bigru_res (rows"
    oct_ = "post-net scan: persistent k_bigru_oct<%d>" % (4 if B > 16 else 2 if B > 8 else 1)
    duo = "post-net scan: persistent k_bigru_duo<%d>" % (4 if B > 16 else 2 if B > 8 else 1)
    return {1: oct_ if B > 8 else duo, 10: oct_, 11: duo, 2: "taco_debug_set_persistent(2): k_bigru_rows;",
            3: "taco_debug_set_persistent(3): k_bigru_res;", 7: "taco_debug_set_persistent(7): k_bigru_resw;"}[persist]


@pytest.mark.gpu
@pytest.mark.parametrize("scope,persist,B", [("post_cbhg", p, B) for p in (1, 2, 3, 7, 10, 11) for B in (5, 12, 20)] +
                                            [("encoder_cbhg", p, 5) for p in (1, 3)])
def test_bigru_scan_alone(ref_model, scope, persist, B):
    """taco_bigru_f32 against O.bidirectional_gru, 1e-4 (test_bigru_persistent_full_width_repeatable's bar): the packs' bx[dir * 3H + j]
    and the candidate bias beside the h rows, per scan kernel -- post-net (H 256): the default (k_bigru_duo<1> at 5 rows, k_bigru_oct<2> at
    12, <4> at 20), k_bigru_rows, k_bigru_res, k_bigru_resw, k_bigru_oct wherever it fits, k_bigru_duo<1 / 2 / 4>; encoder (H 128):
    k_bigru_quad and k_bigru_res."""
    import torch
    import taco_amd
    ohp, w, m = ref_model
    x, lens, init, ref = scan_case(scope, B)
    H = x.shape[2]
    xd, ld, idv = dev(x, torch.float32), dev(lens), dev(init, torch.float32)
    n = int(m._lib.taco_stage_workspace_bytes(m._handle, B, SCAN_T))
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    out = torch.full((B, SCAN_T, 2 * H), float("nan"), device="cuda")
    taco_amd._lib.check(m._lib.taco_debug_set_persistent(m._handle, persist))
    try:
        plan = m.engine_plan(B, SCAN_T, SCAN_T)
        taco_amd._lib.check(m._lib.taco_bigru_f32(m._handle, stream(), scope.encode(), ptr(xd), ptr(ld), ptr(idv), B, SCAN_T, ptr(out), ptr(ws), n))
        torch.cuda.synchronize()
        m.check_device_errors()
    finally:
        taco_amd._lib.check(m._lib.taco_debug_set_persistent(m._handle, 1))
    got = out.cpu().numpy()
    err = maxabs(got, ref) if np.isfinite(got).all() else float("inf")
    print("%s scan, taco_debug_set_persistent %d, %d rows (%s): max|err| %.2e" % (scope, persist, B, _scan_words(scope, persist, B), err))
    assert _scan_words(scope, persist, B) in plan, plan
    assert err < 1e-4


@pytest.fixture(scope="module")
def tiny_ctx():
    """test_gpu_ops.py's model (tiny_hp, init_weights seed 7), its weights made trained-like"""
    import taco_amd
    ohp = tiny_hp()
    w = trained_like(O.init_weights(ohp, 1, 7), 8)
    m = build_model(ohp, w)
    yield ohp, w, m, taco_amd._lib
    m.close()


OPS_TOL = 3e-5      # test_gpu_ops.py's TOL


@pytest.mark.gpu
@pytest.mark.parametrize("name,res", [("decoder/attention_gru", False), ("decoder/gru_1", True), ("decoder/gru_2", True)])
def test_decoder_gru_cell_trained_like(tiny_ctx, name, res):
    """test_gpu_ops.py::test_decoder_gru_cell, the same call and bar, on gate biases that are not constant"""
    import torch
    ohp, w, m, L = tiny_ctx
    rs = np.random.RandomState(3)
    I = w[name + "/gates/kernel"].shape[0] - w[name + "/candidate/bias"].shape[0]
    H = w[name + "/candidate/bias"].shape[0]
    R = 6
    x, h = rs.randn(R, I), rs.randn(R, H)
    hn = O.gru_cell(x, h, w, name)
    hd = dev(h, torch.float32)
    outr = torch.full((R, H), float("nan"), device="cuda") if res else None
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
    xd = dev(x, torch.float32)
    L.check(m._lib.taco_gru_cell_f32(m._handle, stream(), name.encode(), ptr(xd), ptr(hd), R, ptr(outr), ptr(ws), 1 << 16))
    torch.cuda.synchronize()
    print("%s: max|err| of h' %.2e" % (name, maxabs(hd.cpu().numpy(), hn)))
    assert maxabs(hd.cpu().numpy(), hn) < OPS_TOL
    if res:
        assert maxabs(outr.cpu().numpy(), hn + x) < OPS_TOL


@pytest.mark.gpu
def test_highway_trained_like(tiny_ctx):
    """test_gpu_ops.py::test_highway, the same calls and bar, on T biases that are not constant"""
    import torch
    ohp, w, m, L = tiny_ctx
    rs = np.random.RandomState(8)
    for scope, D in (("encoder_cbhg", ohp.enc_rnn_size), ("post_cbhg", ohp.post_rnn_size)):
        x = rs.randn(77, D)
        out = torch.full((77, D), float("nan"), device="cuda")
        xd = dev(x, torch.float32)
        L.check(m._lib.taco_highway_f32(m._handle, stream(), (scope + "/highway_2").encode(), ptr(xd), 77, ptr(out)))
        torch.cuda.synchronize()
        err = maxabs(out.cpu().numpy(), O.highwaynet(x, w, scope + "/highway_2"))
        print("%s/highway_2: max|err| %.2e" % (scope, err))
        assert err < OPS_TOL


# ---- the training forward ----

@pytest.mark.gpu
@pytest.mark.parametrize("model_type,atype,B", [("single", "bah_mon", 9), ("simple", "bah_norm", 5), ("deepvoice", "bah", 20)])
def test_training_forward_trained_like(model_type, atype, B):
    """Trainer on trained_like weights at the shapes of test_training_forward_on_the_persistent_kernels (T_in 14, 8 steps; rows per group
    2 / 1 / 4) with its bars -- 1e-4 on mel, linear and alignments, 2e-5 on the loss -- against the oracle's teacher-forced training forward,
    on the persistent engine and on the launch-per-stage one.  Then one train_step: the packs are rebuilt on the device (k_dx_fold and the
    index-map gather) from live parameters, none of them constant; the forward after it is held to the oracle on the weights read back."""
    import torch
    import taco_amd
    ns = 1 if model_type == "single" else 3
    hp = O.OracleHParams(max_iters=8, model_type=model_type, attention_type=atype)
    w = trained_like(O.init_weights(hp, ns, 581), 582)
    r = hp.reduction_factor
    T_in, T_out = 14, 8 * r
    ids, L = O.synthetic_inputs(B, T_in, 583, ragged=True)
    rs = np.random.RandomState(584)
    mt, lt = rs.rand(B, T_out, hp.num_mels), rs.rand(B, T_out, hp.num_freq)
    co = rs.uniform(0.5, 1.5, size=B)
    spk = (np.arange(B) % ns).astype(np.int32) if ns > 1 else None
    tr = taco_amd.Trainer(to_product_hp(hp), w, num_speakers=ns)
    bad = []

    def hold(tag, weights):
        ref = O.forward(weights, hp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=8, honor_stop=False, teacher_frames=mt[:, r - 1::r], training=True)
        want = O.add_loss(ref["mel"], mt, ref["linear"], lt, co)["loss"]
        for engine in (1, 0):
            tr.set_decoder_engine(engine)
            losses = tr.forward_backward(ids, L, mt, lt, co, backward=False, keep_outputs=True, speaker_id=spk)
            torch.cuda.synchronize()
            tr.check_device_errors()
            if engine:
                info = tr.decoder_engine_info()
                if not (info["has_pack"] and info["protocol"] in (1, 2)):
                    bad.append("%s: the persistent decoder did not run: %s" % (tag, info))
            e = [maxabs(tr.mel_outputs.cpu().numpy(), ref["mel"]), maxabs(tr.linear_outputs.cpu().numpy(), ref["linear"]),
                 maxabs(tr.alignments.cpu().numpy(), ref["alignments"]), abs(float(losses[0]) - want)]
            arm = "%s / %s, %d rows, %s, %s engine" % (model_type, atype, B, tag, "persistent" if engine else "launch-per-stage")
            print("%-86s max|err| mel %.2e  linear %.2e  alignments %.2e  loss %.2e" % ((arm,) + tuple(e)))
            bad.extend("%s: %s off by %.3e (bar %.0e)" % (arm, k, x, b) for k, x, b in zip(ARRAYS + ("loss",), e, (1e-4, 1e-4, 1e-4, 2e-5)) if not x < b)
        tr.set_decoder_engine(1)

    try:
        hold("trained_like weights", w)
        step, lwc = tr.train_step(ids, L, mt, lt, co, speaker_id=spk)
        torch.cuda.synchronize()
        tr.check_device_errors()
        assert step == 1 and np.isfinite(float(lwc))
        w2 = tr.get_weights()
        moved = sum(1 for k in w if not k.endswith(("/moving_mean", "/moving_variance")) and not np.array_equal(w2[k], w[k]))
        assert moved > len(w) // 2, "the step changed %d of %d tensors" % (moved, len(w))
        hold("after one train_step", w2)
    finally:
        tr.close()
    assert not bad, "\n".join(bad)
