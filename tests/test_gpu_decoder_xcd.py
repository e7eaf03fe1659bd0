"""Persistent XCD-local decoder (csrc/taco_decoder_xcd.h) at the reference widths: every step against the float64 oracle,
against the launch-per-stage engine, across batch sizes / rows-per-group / exchange protocols, and the horizons VERDICT r01
asked for (C5 at real widths, C1 and C3 at full length).  Reference: rnn_wrappers.py:218-341,367-415; helpers.py:9-32."""
import numpy as np
import pytest

import taco_oracle as O
from util import build_model, maxabs, argmax_match

pytestmark = pytest.mark.gpu


def _decoder_vs_oracle(ohp, w, ids, L, n, spk=None, ns=1, mode=1, rows=0, tol=2e-4):
    import torch
    taps = {}
    ref = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=n, taps=taps, honor_stop=False)
    m = build_model(ohp, w, num_speakers=ns)
    m.set_decoder_engine(mode, rows)
    mel, al, stop, dbg = m.decoder(taps["encoder"], n, speaker_id=spk, debug=True)
    torch.cuda.synchronize()
    info = m.decoder_engine_info()
    m.check_device_errors()
    dbg = dbg.cpu().numpy()
    As, D, H = ohp.attention_state_size, 2 * ohp.enc_rnn_size, ohp.dec_rnn_size
    for t, st in enumerate(taps["steps"]):
        assert maxabs(dbg[t, :, :As], st["h_att"]) < tol, "h_att step %d" % t
        assert maxabs(dbg[t, :, As:As + D], st["ctx"]) < tol, "ctx step %d" % t
        for i, h in enumerate(st["h"]):
            o = As + D + i * H
            assert maxabs(dbg[t, :, o:o + H], h) < tol, "h_%d step %d" % (i + 1, t)
    assert maxabs(mel.cpu().numpy(), ref["mel"]) < tol
    assert maxabs(al.cpu().numpy(), ref["alignments"]) < tol
    nchk, bad = argmax_match(al.cpu().numpy(), ref["alignments"])
    assert bad == 0
    assert int(stop.item()) == n
    return m, info, (mel.cpu().numpy(), al.cpu().numpy()), taps


@pytest.mark.parametrize("atype", ["bah_mon", "bah", "bah_norm"])
def test_every_step_matches_the_oracle_at_reference_widths(atype):
    ohp = O.OracleHParams(max_iters=6, attention_type=atype)
    w = O.init_weights(ohp, 1, 311)
    ids, L = O.synthetic_inputs(5, 37, 312, ragged=True)
    m, info, _, _ = _decoder_vs_oracle(ohp, w, ids, L, 6)
    assert info["has_pack"] and info["protocol"] in (1, 2), info
    assert sum(info["per_xcd"]) == 256 and info["compute_units"] >= 256, info      # the whole-chip kernels run only on a whole MI355X


def test_deepvoice_initial_states_and_reduction_factor_5():
    ohp = O.OracleHParams(max_iters=5, reduction_factor=5, model_type="deepvoice")
    w = O.init_weights(ohp, 4, 313)
    ids, L = O.synthetic_inputs(6, 20, 314, ragged=True)
    spk = (np.arange(6) % 4).astype(np.int32)
    _, info, _, _ = _decoder_vs_oracle(ohp, w, ids, L, 5, spk=spk, ns=4)
    assert info["protocol"] in (1, 2)


@pytest.mark.parametrize("B,rows", [(1, 0), (8, 0), (13, 0), (32, 0), (33, 0), (64, 0), (8, 2), (8, 8), (16, 4)])
def test_batch_sizes_and_rows_per_group(B, rows):
    """rows per group 1 / 2 / 4 / 8 (B <= 8, 16, 32, 64), ragged last group, and batches packed onto fewer XCDs."""
    ohp = O.OracleHParams(max_iters=4)
    w = O.init_weights(ohp, 1, 315)
    ids, L = O.synthetic_inputs(B, 32, 316 + B, ragged=True)
    _, info, _, _ = _decoder_vs_oracle(ohp, w, ids, L, 4, rows=rows)
    assert info["protocol"] in (1, 2)


def test_write_through_protocol_and_launch_engine_agree():
    """mode 2 (sc1 stores, placement-independent) and mode 1 must give bit-identical results (same arithmetic, different cache
    policy); the launch-per-stage engine (mode 0) is the same function up to summation order."""
    import torch
    ohp = O.OracleHParams(max_iters=12)
    w = O.init_weights(ohp, 1, 317)
    ids, L = O.synthetic_inputs(9, 50, 318, ragged=True)
    m, info, (mel1, al1), taps = _decoder_vs_oracle(ohp, w, ids, L, 12)
    m.set_decoder_engine(2)
    mel2, al2, _, _ = m.decoder(taps["encoder"], 12)
    info2 = m.decoder_engine_info()
    assert info2["protocol"] == 2
    assert np.array_equal(mel2.cpu().numpy(), mel1) and np.array_equal(al2.cpu().numpy(), al1)
    m.set_decoder_engine(1)
    mel3, al3, _, _ = m.decoder(taps["encoder"], 12)
    torch.cuda.synchronize()
    assert np.array_equal(mel3.cpu().numpy(), mel1), "persistent decoder is not bit-repeatable"
    m.set_decoder_engine(0)
    mel0, al0, _, _ = m.decoder(taps["encoder"], 12)
    torch.cuda.synchronize()
    assert maxabs(mel0.cpu().numpy(), mel1) < 2e-5 and maxabs(al0.cpu().numpy(), al1) < 2e-5
    m.check_device_errors()


def test_stop_flags_of_the_persistent_decoder():
    """helpers.py:29: a row is finished when all r*num_mels outputs of a step are exactly 0."""
    import torch
    ohp = O.OracleHParams(max_iters=5)
    w = O.init_weights(ohp, 1, 319)
    w["decoder/frame_projection/kernel"][:] = 0
    w["decoder/frame_projection/bias"][:] = 0
    ids, L = O.synthetic_inputs(3, 16, 320)
    taps = {}
    O.forward(w, ohp, ids, L, taps=taps, honor_stop=False)
    m = build_model(ohp, w)
    mel, al, stop, _ = m.decoder(taps["encoder"], 5)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    assert int(stop.item()) == 1 and not mel.cpu().numpy().any()


@pytest.mark.parametrize("B,T_in,atype", [(2, 16, "bah_mon"), (5, 37, "bah"), (32, 128, "bah_mon"), (9, 200, "bah_norm"), (40, 70, "bah_mon")])
def test_manual_attention_on_the_persistent_decoder(B, T_in, atype):
    """rnn_wrappers.py:313-317: `alignments = manual_alignments[:, time, :]` -- a mode of k_decoder_xcd (the query / score /
    normaliser phases are skipped, the step's row goes straight into LDS): every decoder state of every step against the oracle,
    rows per group 1 / 2 / 4 / 8, input lengths that are not multiples of a wave, and against the launch-per-stage engine."""
    import torch
    n = 5
    ohp = O.OracleHParams(max_iters=n, attention_type=atype)
    w = O.init_weights(ohp, 1, 321)
    ids, L = O.synthetic_inputs(B, T_in, 322 + B, ragged=True)
    man = np.random.RandomState(3 + B).dirichlet(np.ones(T_in), (B, n))
    taps = {}
    ref = O.forward(w, ohp, ids, L, manual_alignments=man, taps=taps, honor_stop=False)
    m = build_model(ohp, w)
    mel, al, _, dbg = m.decoder(taps["encoder"], n, manual_alignments=man, debug=True)
    torch.cuda.synchronize()
    info = m.decoder_engine_info()
    m.check_device_errors()
    assert info["has_pack"] and info["protocol"] in (1, 2), info          # served by the persistent kernel, not by the fallback
    dbg = dbg.cpu().numpy()
    As, D, H = ohp.attention_state_size, 2 * ohp.enc_rnn_size, ohp.dec_rnn_size
    for t, st in enumerate(taps["steps"]):
        assert maxabs(dbg[t, :, :As], st["h_att"]) < 2e-4 and maxabs(dbg[t, :, As:As + D], st["ctx"]) < 2e-4, t
        for i, h in enumerate(st["h"]):
            assert maxabs(dbg[t, :, As + D + i * H:As + D + (i + 1) * H], h) < 2e-4, (t, i)
    assert maxabs(mel.cpu().numpy(), ref["mel"]) < 2e-4
    assert maxabs(al.cpu().numpy(), np.transpose(man, (0, 2, 1))) < 1e-6
    m.set_decoder_engine(0)
    mel0, al0, _, _ = m.decoder(taps["encoder"], n, manual_alignments=man)
    torch.cuda.synchronize()
    assert maxabs(mel0.cpu().numpy(), mel.cpu().numpy()) < 2e-5 and np.array_equal(al0.cpu().numpy(), al.cpu().numpy())


@pytest.mark.parametrize("atype,B", [("bah_mon", 6), ("bah", 33)])
def test_simple_multispeaker_on_the_persistent_decoder(atype, B):
    """model_type 'simple' (rnn_wrappers.py:372-376, 408-413): the speaker embedding is an input segment of the attention GRU and of
    the concat projection; in k_decoder_xcd its (loop-invariant) products enter as per-row biases (k_dx_rowbias).  Every state of
    every step against the oracle, and the whole forward end to end."""
    import torch
    ns, n = 3, 5
    ohp = O.OracleHParams(max_iters=n, model_type="simple", attention_type=atype)
    w = O.init_weights(ohp, ns, 331)
    ids, L = O.synthetic_inputs(B, 29, 332, ragged=True)
    spk = (np.arange(B) % ns).astype(np.int32)
    m, info, _, _ = _decoder_vs_oracle(ohp, w, ids, L, n, spk=spk, ns=ns)
    assert info["has_pack"] and info["protocol"] in (1, 2), info
    lin, al = m.run(inputs=ids, input_lengths=L, speaker_id=spk)
    torch.cuda.synchronize()
    ref = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns)
    k = ref["mel"].shape[1]
    assert maxabs(m.mel_outputs.cpu().numpy()[:, :k], ref["mel"]) < 2e-4 and maxabs(lin.cpu().numpy()[:, :k], ref["linear"]) < 2e-4
    m.check_device_errors()


PRESETS = {   # hparams.py:71-117: the blocks the reference ships switched off (`if False` / `elif False`), field by field
    "single_speaker": dict(attention_size=128, post_bank_channel_size=128, post_rnn_size=128),
    "single_speaker_generalization": dict(attention_size=256, dec_prenet_sizes=[256, 128, 64], post_bank_channel_size=128, post_rnn_size=128),
    "deep_voice_2_first_block": dict(attention_size=512, dec_prenet_sizes=[256, 128, 64], post_bank_channel_size=512, post_rnn_size=256),
    # (the two remaining combinations of the decoder-side fields)
    "attention_128_three_prenet_layers": dict(attention_size=128, dec_prenet_sizes=[256, 128, 64]),
    "attention_512_two_prenet_layers": dict(attention_size=512),
}


@pytest.mark.parametrize("B", [5, 32, 40])
@pytest.mark.parametrize("atype", ["bah_mon", "bah_norm"])
@pytest.mark.parametrize("preset", sorted(PRESETS))
def test_other_presets_on_the_persistent_decoder(preset, atype, B):
    """The other presets of hparams.py:71-117 (attention_size 128 / 512, a third decoder prenet layer of 64) are template parameters
    of k_decoder_xcd: every state of every step against the float64 oracle, at 4 rows per group (B <= 32; smaller batches are padded
    groups) and 8 (B = 40; attention_size 512 has no instantiation there and must say so in engine_plan and fall back)."""
    n = 5
    ohp = O.OracleHParams(max_iters=n, attention_type=atype, **PRESETS[preset])
    w = O.init_weights(ohp, 1, 341)
    ids, L = O.synthetic_inputs(B, 37, 342 + B, ragged=True)
    m, info, _, _ = _decoder_vs_oracle(ohp, w, ids, L, n)
    plan = m.engine_plan(B, 37)
    if ohp.attention_size == 512 and B > 32:
        # no instantiation at 8 rows per group (query registers): round 6 serves such a batch as TWO passes of at most 32 rows on the persistent
        # decoder (the per-step state dump of _decoder_vs_oracle is laid out [step][row] and keeps the whole batch in one launch-per-stage call)
        import torch
        assert info["protocol"] == 0 and "40 rows = 2 passes of 20" in plan and "persistent k_decoder_xcd<4, attention 512" in plan, (info, plan)
        taps = {}
        ref = O.forward(w, ohp, ids, L, n_steps=n, taps=taps, honor_stop=False)
        mel, al, stop, _ = m.decoder(taps["encoder"], n)
        torch.cuda.synchronize()
        assert m.decoder_engine_info()["protocol"] in (1, 2) and int(stop.item()) == n
        assert maxabs(mel.cpu().numpy(), ref["mel"]) < 2e-4 and maxabs(al.cpu().numpy(), ref["alignments"]) < 2e-4
        lin, al2 = m.run(inputs=ids, input_lengths=L, honor_stop=False)
        torch.cuda.synchronize()
        assert m.decoder_engine_info()["protocol"] in (1, 2)
        assert maxabs(m.mel_outputs.cpu().numpy(), ref["mel"]) < 2e-4 and maxabs(lin.cpu().numpy(), ref["linear"]) < 2e-4
        m.check_device_errors()
    else:
        assert info["has_pack"] and info["protocol"] in (1, 2), (info, plan)
        assert "persistent k_decoder_xcd<%d, attention %d, %d prenet layers>" % (4 if B <= 32 else 8, ohp.attention_size, len(ohp.dec_prenet_sizes)) in plan, plan


def test_state_dump_of_40_rows_at_attention_512_in_the_stage_workspace():
    """attention_size 512, 40 rows: the plain decoder call is two passes of 20 on the persistent engine, the call with the per-step state dump ONE
    pass of 40 rows on the launch-per-stage engine -- in a workspace of exactly taco_stage_workspace_bytes(m, 40, 21) bytes (Tacotron._stage_ws),
    which sizes the decoder from the larger of the two plans.  Same function on both engines: mel and alignments to the 2e-5 of
    test_write_through_protocol_and_launch_engine_agree, the stop words equal."""
    import torch
    B, T_in, n = 40, 21, 5
    ohp = O.OracleHParams(max_iters=n, **PRESETS["attention_512_two_prenet_layers"])
    w = O.init_weights(ohp, 1, 343)
    ids, L = O.synthetic_inputs(B, T_in, 344, ragged=True)
    m = build_model(ohp, w)
    assert "no instantiation at 8 rows per group" in m.engine_plan(B, T_in, debug=True) and "40 rows = 2 passes of 20" in m.engine_plan(B, T_in)
    enc = m.encoder(ids, L)
    mel_d, al_d, stop_d, dbg = m.decoder(enc, n, debug=True)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] == 0 and bool(torch.isfinite(dbg).all())
    mel_p, al_p, stop_p, _ = m.decoder(enc, n)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    e_mel, e_al = maxabs(mel_d.cpu().numpy(), mel_p.cpu().numpy()), maxabs(al_d.cpu().numpy(), al_p.cpu().numpy())
    print("state dump vs two passes: max|mel| %.3g  max|alignments| %.3g  stop %d / %d" % (e_mel, e_al, int(stop_d.item()), int(stop_p.item())))
    assert e_mel < 2e-5 and e_al < 2e-5
    assert int(stop_d.item()) == int(stop_p.item())
    m.check_device_errors()


@pytest.mark.parametrize("preset,model_type", [("single_speaker", "simple"), ("deep_voice_2_first_block", "simple"), ("single_speaker_generalization", "deepvoice")])
def test_other_presets_multi_speaker_manual_attention_and_end_to_end(preset, model_type):
    """... with the multi-speaker model types ('simple': the speaker rows of the attention GRU sit behind a 64-row prenet output
    there), with manual alignments (the MAN instantiations), and the whole forward end to end (the feed-forward stages of these
    presets -- other conv-bank / post-net widths -- run the general kernels)."""
    import torch
    ns, n, B, T_in = 3, 11, 6, 29          # 6 x 44 = 264 output frames: from 256 rows on the linear head is the row sweep (csrc/taco_head.h; K = 256 at post_rnn_size 128)
    ohp = O.OracleHParams(max_iters=n, model_type=model_type, **PRESETS[preset])
    w = O.init_weights(ohp, ns, 351)
    ids, L = O.synthetic_inputs(B, T_in, 352, ragged=True)
    spk = (np.arange(B) % ns).astype(np.int32)
    m, info, _, taps = _decoder_vs_oracle(ohp, w, ids, L, n, spk=spk, ns=ns)
    assert info["has_pack"] and info["protocol"] in (1, 2), info
    man = np.random.RandomState(353).dirichlet(np.ones(T_in), (B, n))
    refm = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=n, manual_alignments=man, honor_stop=False)
    mel, al, _, _ = m.decoder(taps["encoder"], n, speaker_id=spk, manual_alignments=man)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    assert maxabs(mel.cpu().numpy(), refm["mel"]) < 2e-4 and maxabs(al.cpu().numpy(), refm["alignments"]) < 2e-4
    lin, al = m.run(inputs=ids, input_lengths=L, speaker_id=spk)
    torch.cuda.synchronize()
    ref = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns)
    k = ref["mel"].shape[1]
    assert maxabs(m.mel_outputs.cpu().numpy()[:, :k], ref["mel"]) < 2e-4 and maxabs(lin.cpu().numpy()[:, :k], ref["linear"]) < 2e-4
    m.check_device_errors()


@pytest.mark.parametrize("model_type,B,atype", [("single", 2, "bah_mon"), ("deepvoice", 19, "bah"), ("simple", 40, "bah_norm")])
def test_teacher_forced_decoding_on_the_persistent_decoder(model_type, B, atype):
    """Teacher-forced frames on an INFERENCE model (helpers.py:35-67 outside the trainer): the TAPE instantiation of k_decoder_xcd
    without a tape, its four prenet-layer-1 frame registers loaded with the raw kernel rows that the model keeps beside its composite
    pack.  Every state of every step against the oracle (rows per group 1 / 4 / 8), and against the launch-per-stage loop."""
    import torch
    ns, n = (1 if model_type == "single" else 3), 6
    ohp = O.OracleHParams(max_iters=n, model_type=model_type, attention_type=atype)
    w = O.init_weights(ohp, ns, 321)
    ids, L = O.synthetic_inputs(B, 16, 322, ragged=True)
    spk = (np.arange(B) % ns).astype(np.int32) if ns > 1 else None
    frames = np.random.RandomState(5).rand(B, n, ohp.num_mels)
    taps = {}
    ref = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=n, teacher_frames=frames, taps=taps, honor_stop=False)
    m = build_model(ohp, w, num_speakers=ns)
    mel, al, _, dbg = m.decoder(taps["encoder"], n, speaker_id=spk, teacher_frames=frames, debug=True)
    torch.cuda.synchronize()
    m.check_device_errors()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    dbg = dbg.cpu().numpy()
    As, D, H = ohp.attention_state_size, 2 * ohp.enc_rnn_size, ohp.dec_rnn_size
    for t, st in enumerate(taps["steps"]):
        assert maxabs(dbg[t, :, :As], st["h_att"]) < 2e-4 and maxabs(dbg[t, :, As:As + D], st["ctx"]) < 2e-4, t
        for i, h in enumerate(st["h"]):
            assert maxabs(dbg[t, :, As + D + i * H:As + D + (i + 1) * H], h) < 2e-4, (t, i)
    assert maxabs(mel.cpu().numpy(), ref["mel"]) < 2e-4 and maxabs(al.cpu().numpy(), ref["alignments"]) < 2e-4
    m.set_decoder_engine(0)
    mel0, al0, _, _ = m.decoder(taps["encoder"], n, speaker_id=spk, teacher_frames=frames)
    torch.cuda.synchronize()
    assert maxabs(mel0.cpu().numpy(), mel.cpu().numpy()) < 2e-5 and maxabs(al0.cpu().numpy(), al.cpu().numpy()) < 2e-5
    # teacher frames TOGETHER with manual alignments (rnn_wrappers.py:313-317 under helpers.py:35-67): the <TAPE, MAN> instantiation (round 6; the
    # launch-per-stage loop until then)
    m.set_decoder_engine(1)
    man = np.random.RandomState(6).dirichlet(np.ones(16), (B, n))
    refm = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=n, teacher_frames=frames, manual_alignments=man, honor_stop=False)
    melm, alm, _, _ = m.decoder(taps["encoder"], n, speaker_id=spk, teacher_frames=frames, manual_alignments=man)
    torch.cuda.synchronize()
    m.check_device_errors()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    assert maxabs(melm.cpu().numpy(), refm["mel"]) < 2e-4 and maxabs(alm.cpu().numpy(), np.transpose(man, (0, 2, 1))) < 1e-6
    # the same model without teacher frames afterwards: the composite registers are back
    free = O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=ns, n_steps=n, honor_stop=False)
    mel1, _, _, _ = m.decoder(taps["encoder"], n, speaker_id=spk)
    torch.cuda.synchronize()
    assert maxabs(mel1.cpu().numpy(), free["mel"]) < 2e-4


def test_C5_real_widths_against_the_oracle():
    """the long-input regime (T_in = 512) at reference widths, 24 steps, B = 2: persistent engine (one row
    per group, 32 members per row) and the launch engine with the split attention forced and automatic."""
    import torch
    ohp = O.OracleHParams(max_iters=24)
    w = O.init_weights(ohp, 1, 1234 + 4)
    ids, L = O.synthetic_inputs(2, 512, 323, ragged=True)
    m, info, (mel1, al1), taps = _decoder_vs_oracle(ohp, w, ids, L, 24)
    assert info["protocol"] in (1, 2)
    ref_mel = O.forward(w, ohp, ids, L, n_steps=24, honor_stop=False)["mel"]
    for split in (-1, 4):
        m.set_decoder_engine(0)
        m._lib.taco_debug_set_att_split(m._handle, split)
        mel0, al0, _, _ = m.decoder(taps["encoder"], 24)
        torch.cuda.synchronize()
        assert maxabs(mel0.cpu().numpy(), ref_mel) < 2e-4, "launch engine, att_split %d" % split
        assert maxabs(al0.cpu().numpy(), al1) < 2e-5
    m._lib.taco_debug_set_att_split(m._handle, -1)


def test_C5_full_horizon_two_rows_against_the_oracle():
    """VERDICT r02 missing 3: the regime C5 exists for -- 1000 feedback steps of the persistent decoder and a T = 4000 post-net scan
    (250 turns of the scan's prefetch ring) -- end to end against the float64 oracle, two ragged rows at T_in = 512
    (rnn_wrappers.py:218-341, modules.py:82-96).  Nine seconds of oracle."""
    import torch
    B, T_in, r, n, ns, mt = O.CONFIGS["C5"]
    ohp = O.OracleHParams(max_iters=n, reduction_factor=r)
    w = O.init_weights(ohp, 1, 1234 + 4)
    ids, L = O.synthetic_inputs(2, T_in, 777, ragged=True)
    m = build_model(ohp, w)
    lin, al = m.run(inputs=ids, input_lengths=L)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    m.check_device_errors()
    ref = O.forward(w, ohp, ids, L)
    mel, lin, al = m.mel_outputs.cpu().numpy(), lin.cpu().numpy(), al.cpu().numpy()
    assert mel.shape == ref["mel"].shape == (2, 4000, 80) and al.shape == (2, 512, 1000)
    e_mel, e_lin, e_al = maxabs(mel, ref["mel"]), maxabs(lin, ref["linear"]), maxabs(al, ref["alignments"])
    late = maxabs(mel[:, 2000:], ref["mel"][:, 2000:])
    print("C5 full horizon: max|mel| %.2e (second half %.2e)  max|linear| %.2e  max|align| %.2e" % (e_mel, late, e_lin, e_al))
    assert e_mel < 1e-3 and e_lin < 1e-3 and e_al < 1e-3
    nchk, bad = argmax_match(al, ref["alignments"])
    assert bad == 0 and nchk > 100


def test_C1_full_length_200_steps():
    """C1 (B=1, T_in=64, r=5) over all 200 decoder steps, end to end."""
    import torch
    B, T_in, r, n, ns, mt = O.CONFIGS["C1"]
    ohp = O.OracleHParams(max_iters=n, reduction_factor=r)
    w = O.init_weights(ohp, 1, 1234)
    ids, L = O.synthetic_inputs(B, T_in, 1234)
    m = build_model(ohp, w)
    lin, al = m.run(inputs=ids, input_lengths=L)
    torch.cuda.synchronize()
    ref = O.forward(w, ohp, ids, L)
    assert maxabs(m.mel_outputs.cpu().numpy(), ref["mel"]) < 1e-3
    assert maxabs(lin.cpu().numpy(), ref["linear"]) < 1e-3
    nchk, bad = argmax_match(al.cpu().numpy(), ref["alignments"])
    print("C1: argmax compared at %d of %d steps" % (nchk, al.shape[0] * al.shape[2]))
    assert bad == 0
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    m.check_device_errors()


def test_C3_full_length_128_steps_on_8_of_the_32_rows():
    """C3 (deepvoice, 4 speakers) at all 128 steps; the float64 oracle runs 8 of the 32 rows (rows are
    independent at inference), the device runs all 32."""
    import torch
    B, T_in, r, n, ns, mt = O.CONFIGS["C3"]
    ohp = O.OracleHParams(max_iters=n, reduction_factor=r, model_type=mt)
    w = O.init_weights(ohp, ns, 1234 + 2)
    ids, L = O.synthetic_inputs(B, T_in, 1234 + 2, ragged=True)
    spk = (np.arange(B) % ns).astype(np.int32)
    m = build_model(ohp, w, num_speakers=ns)
    lin, al = m.run(inputs=ids, input_lengths=L, speaker_id=spk, honor_stop=False)
    torch.cuda.synchronize()
    rows = np.arange(0, 32, 4)
    ref = O.forward(w, ohp, ids[rows], L[rows], speaker_id=spk[rows], num_speakers=ns, honor_stop=False)
    assert maxabs(m.mel_outputs.cpu().numpy()[rows], ref["mel"]) < 1e-3
    assert maxabs(lin.cpu().numpy()[rows], ref["linear"]) < 1e-3
    nchk, bad = argmax_match(al.cpu().numpy()[rows], ref["alignments"])
    print("C3: argmax compared at %d of %d steps" % (nchk, len(rows) * n))
    assert bad == 0
    m.check_device_errors()


@pytest.mark.parametrize("B", [1, 7, 9, 16, 17, 32, 64])
def test_post_net_scan_spread_over_the_chip(B):
    """The whole-chip scans of csrc/taco_bigru_xcd.h at H = 256: k_bigru_oct (round 5, the default from 9 to 32 rows: ONE row per cluster
    of 8 / 16 CUs, both directions pipelined against each other; persist 10 forces it for every B <= 32, i.e. also its 32-CU geometry) and
    k_bigru_duo (persist 11; the default up to 8 and above 32 rows: 8 groups of 32 CUs, BOTH directions of ceil(B/8) rows each).
    Against the oracle's bidirectional GRU (modules.py:82-96, A.6/A.7) with ragged lengths (incl. 0 and T) and an initial state,
    against the one-CU-per-chain kernel they replace, and bit-repeatable."""
    import ctypes as C
    import torch
    import taco_amd
    from util import dev, ptr, stream
    ohp = O.OracleHParams(max_iters=4)
    w = O.init_weights(ohp, 1, 41)
    m = build_model(ohp, w)
    rs = np.random.RandomState(42 + B)
    T, H = 37, ohp.post_rnn_size
    x = rs.randn(B, T, H) * 0.5
    lens = rs.randint(0, T + 1, size=B).astype(np.int32); lens[0] = T
    if B > 1:
        lens[1] = 0
    init = rs.randn(B, 2 * H) * 0.5
    xd, ld, idv = dev(x, torch.float32), dev(lens), dev(init, torch.float32)
    n = int(m._lib.taco_stage_workspace_bytes(m._handle, B, T))
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    got = {}
    # 1: the default; 10: k_bigru_oct wherever it fits; 11: k_bigru_duo; 7: one CU per chain
    for persist in (1, 1, 10, 10, 11, 11, 7):
        m._lib.taco_debug_set_persistent(m._handle, persist)
        for tag, (lp, ip) in (("plain", (ptr(None), ptr(None))), ("ragged", (ptr(ld), ptr(idv)))):
            out = torch.full((B, T, 2 * H), float("nan"), device="cuda")
            taco_amd._lib.check(m._lib.taco_bigru_f32(m._handle, stream(), b"post_cbhg", ptr(xd), lp, ip, B, T, ptr(out), ptr(ws), n))
            torch.cuda.synchronize()
            got.setdefault((persist, tag), []).append(out.cpu().numpy())
    m._lib.taco_debug_set_persistent(m._handle, 1)
    m.check_device_errors()
    v = (C.c_int * 16)()
    taco_amd._lib.check(m._lib.taco_debug_decoder_info(m._handle, v))
    for tag, ref in (("plain", O.bidirectional_gru(x, None, w, "post_cbhg/bigru")), ("ragged", O.bidirectional_gru(x, lens, w, "post_cbhg/bigru", init))):
        for persist, name in ((1, "the default scan"), (10, "k_bigru_oct"), (11, "k_bigru_duo")):
            a, b = got[(persist, tag)]
            assert np.array_equal(a, b), "%s is not bit-repeatable (%s)" % (name, tag)
            assert maxabs(a, ref) < 1e-4, (name, tag)
            assert maxabs(a, got[(7, tag)][0]) < 2e-5, (name, tag)
        a = got[(1, tag)][0]
        # which kernel the default is: k_bigru_oct from 9 to 32 rows (bit-identical to persist 10), k_bigru_duo otherwise (persist 11)
        assert np.array_equal(a, got[(10 if 8 < B <= 32 else 11, tag)][0]), tag


@pytest.mark.parametrize("B,T", [(5, 300), (32, 128), (3, 1000)])
def test_encoder_scan_fast_transcendentals_against_libm_and_the_oracle(B, T):
    """the encoder scan (H = 128) runs k_bigru_quad, whose sigmoid / tanh are rcp / exp2 approximations, where k_bigru_res
    (persist 3) calls libm's expf / tanhf; its outputs are the attention keys and values, i.e. they feed the alignment argmax.  Held here
    directly: k_bigru_quad vs k_bigru_res vs the float64 oracle over LONG ragged inputs (the error of a contractive recurrence does not
    grow with T; measured on MI355X: both kernels sit 5.9e-6 from float64 at T = 300 -- fp32 rounding of the recurrence itself -- and 2.4e-7 from EACH
    OTHER: the budget for the approximations is 2e-6 absolute on |h| < 1) and an initial state, bit-repeatable."""
    import torch
    import taco_amd
    from util import dev, ptr, stream
    ohp = O.OracleHParams(max_iters=4)
    w = O.init_weights(ohp, 1, 51)
    m = build_model(ohp, w)
    rs = np.random.RandomState(52 + B)
    H = ohp.enc_rnn_size
    x = rs.randn(B, T, H) * 0.7
    lens = rs.randint(T // 2, T + 1, size=B).astype(np.int32); lens[0] = T
    if B > 1:
        lens[1] = 0
    init = rs.randn(B, 2 * H) * 0.5
    xd, ld, idv = dev(x, torch.float32), dev(lens), dev(init, torch.float32)
    n = int(m._lib.taco_stage_workspace_bytes(m._handle, B, T))
    ws = torch.empty((n,), dtype=torch.uint8, device="cuda")
    got = {}
    for persist in (1, 1, 3):
        m._lib.taco_debug_set_persistent(m._handle, persist)
        out = torch.full((B, T, 2 * H), float("nan"), device="cuda")
        taco_amd._lib.check(m._lib.taco_bigru_f32(m._handle, stream(), b"encoder_cbhg", ptr(xd), ptr(ld), ptr(idv), B, T, ptr(out), ptr(ws), n))
        torch.cuda.synchronize()
        got.setdefault(persist, []).append(out.cpu().numpy())
    m._lib.taco_debug_set_persistent(m._handle, 1)
    ref = O.bidirectional_gru(x, lens, w, "encoder_cbhg/bigru", init)
    quad, res = got[1][0], got[3][0]
    assert np.array_equal(quad, got[1][1]), "k_bigru_quad is not bit-repeatable"
    e_q, e_r, d = maxabs(quad, ref), maxabs(res, ref), maxabs(quad, res)
    print("encoder scan, B=%d T=%d: k_bigru_quad vs oracle %.2e, k_bigru_res (libm) vs oracle %.2e, quad vs res %.2e" % (B, T, e_q, e_r, d))
    assert e_q < 3e-5 and e_r < 3e-5 and d < 2e-6
    # the error does not accumulate along the recurrence: the last quarter of the longest row is no worse than the first
    L0 = int(lens[0])
    assert maxabs(quad[0, 3 * L0 // 4:L0], ref[0, 3 * L0 // 4:L0]) < 3e-5 and maxabs(quad[0, 3 * L0 // 4:L0], res[0, 3 * L0 // 4:L0]) < 2e-6


def test_engine_plan_says_which_engine_a_call_gets_and_why_not():
    """taco_model_engine_plan (Tacotron.engine_plan): the limits of the persistent engine, told to the caller before a call instead of
    being tripped silently -- and the plan agrees with what a forward then reports."""
    import torch
    from util import tiny_hp
    ohp = O.OracleHParams(max_iters=4)
    m = build_model(ohp, O.init_weights(ohp, 1, 401))
    plan = m.engine_plan(32, 128, 512)
    assert "decoder loop: persistent k_decoder_xcd<4>" in plan and "post-net scan: persistent k_bigru_oct<4>" in plan and "split-bf16" in plan, plan
    assert "encoder prenet: one k_pointwise_chain launch" in plan, plan            # round 5: gather + both layers + the forward's zero fills in one launch
    assert "k_decoder_xcd<1>" in m.engine_plan(2, 512)
    assert "65 rows = 2 passes of 33" in m.engine_plan(65, 64) and "k_decoder_xcd<8>" in m.engine_plan(65, 64), m.engine_plan(65, 64)
    assert "does not fit a member's LDS" in m.engine_plan(64, 2000), m.engine_plan(64, 2000)
    ids, L = O.synthetic_inputs(3, 12, 402)
    m.run(ids, L)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    m.set_decoder_engine(0)
    assert "switched off" in m.engine_plan(32, 128)
    t = build_model(tiny_hp(), O.init_weights(tiny_hp(), 1, 403))
    plan = t.engine_plan(4, 9)
    assert "one launch per stage -- widths outside the presets" in plan and "resident per-row kernels" in plan, plan
    assert "encoder prenet: one GEMM launch per layer" in plan, plan


PLAN_CASES = {   # name: (hparams, engine mode, B, T_in, decoder() / engine_plan() keywords, persistent?, the words of the reason)
    "fits": (dict(), 1, 5, 19, dict(), True, "k_decoder_xcd<1>"),
    "switched_off": (dict(), 0, 5, 19, dict(), False, "switched off"),
    "widths_outside_the_presets": (None, 1, 4, 9, dict(), False, "widths outside the presets"),
    "lds_at_long_t_in": (dict(), 1, 16, 1200, dict(), False, "T_in = 1200 does not fit a member's LDS at 2 rows per group"),
    "attention_512_state_dump_of_40_rows": (PRESETS["attention_512_two_prenet_layers"], 1, 40, 21, dict(debug=True), False, "no instantiation at 8 rows per group"),
    "attention_512_40_rows_as_two_passes": (PRESETS["attention_512_two_prenet_layers"], 1, 40, 21, dict(), True, "40 rows = 2 passes of 20"),
    "teacher_frames_on_an_inference_model": (dict(), 1, 9, 19, dict(teacher=True), True, "k_decoder_xcd<2>"),
    "teacher_frames_outside_the_reference_widths": (PRESETS["single_speaker"], 1, 9, 19, dict(teacher=True), False, "teacher frames on an inference model"),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_engine_plan_agrees_with_the_launch(case):
    """decoder_plan (csrc/taco_lib.hip) is what decoder_forward follows and what engine_plan words: one decoder() call per reason against
    the persistent kernel that a whole MI355X can reach, and the calls that fit, on a fresh model each (the protocol word keeps the last
    persistent launch's answer) -- the plan says "persistent" exactly when the launch reports an exchange protocol."""
    import torch
    from util import tiny_hp
    kw, mode, B, T_in, call, persistent, words = PLAN_CASES[case]
    n = 2
    ohp = tiny_hp(max_iters=n) if kw is None else O.OracleHParams(max_iters=n, **kw)
    m = build_model(ohp, O.init_weights(ohp, 1, 421))
    m.set_decoder_engine(mode)
    plan = m.engine_plan(B, T_in, **call)
    enc = np.random.RandomState(422).uniform(-1, 1, (B, T_in, 2 * ohp.enc_rnn_size)).astype(np.float32)
    teacher = np.random.RandomState(423).rand(B, n, ohp.num_mels).astype(np.float32) if call.get("teacher") else None
    mel, _, stop, _ = m.decoder(enc, n, teacher_frames=teacher, debug=call.get("debug", False))
    torch.cuda.synchronize()
    info = m.decoder_engine_info()
    m.check_device_errors()
    print(case, info["protocol"], plan)
    assert ("decoder loop: persistent" in plan) == persistent and (info["protocol"] in (1, 2)) == persistent, (info, plan)
    assert persistent or info["protocol"] == 0, info
    assert words in plan, plan
    assert np.isfinite(mel.cpu().numpy()).all() and int(stop.item()) == n


@pytest.mark.parametrize("mode", [1, 0])
def test_engine_plan_agrees_with_a_training_step(mode):
    """... and for a training shadow model: the forward loop (k_decoder_xcd, TAPE) and the backward loop (k_decoder_bwd_xcd) of one
    Trainer step against Trainer.engine_plan, with the engine on and switched off."""
    import torch
    import taco_amd
    from util import to_product_hp
    n, B, T_in = 4, 6, 11
    hp = O.OracleHParams(max_iters=n)
    tr = taco_amd.Trainer(to_product_hp(hp), O.init_weights(hp, 1, 431))
    tr.set_decoder_engine(mode)
    ids, L = O.synthetic_inputs(B, T_in, 432, ragged=True)
    rs = np.random.RandomState(433)
    T_out = n * hp.reduction_factor
    tr.train_step(ids, L, rs.rand(B, T_out, hp.num_mels), rs.rand(B, T_out, hp.num_freq), np.ones(B))
    torch.cuda.synchronize()
    tr.check_device_errors()
    info, plan = tr.decoder_engine_info(), tr.engine_plan(B, T_in, T_out)
    print(mode, info, plan)
    assert ("decoder loop: persistent k_decoder_xcd<1>" in plan) == (mode == 1) == (info["protocol"] in (1, 2)), (info, plan)
    assert ("decoder backward loop: persistent k_decoder_bwd_xcd<1>" in plan) == (mode == 1) == (info["bptt_protocol"] in (1, 2)), (info, plan)
    assert mode == 1 or (info["protocol"] == 0 and plan.count("one launch per stage -- switched off") == 2), (info, plan)


def _ff_clauses(plan):
    """The feed-forward clauses of an engine_plan sentence by name, and the launches they state in all."""
    import re
    ff = plan.split("; feed-forward: ")[1].split("; backward scans: ")[0]
    clauses = {c.split(": ")[0]: c for c in re.split(r"; (?=(?:encoder CBHG|post-net CBHG|encoder prenet|linear head): )", "feed-forward: " + ff)}
    assert sorted(clauses) == ["encoder CBHG", "encoder prenet", "feed-forward", "linear head", "post-net CBHG"], plan
    return clauses, sum(int(k) for k in re.findall(r"(\d+) launch", ff))


FF_MODES = {   # taco_debug_set_bf3(on): words that include/taco_debug.h documents for the mode, and words that must be absent
    1: (["three products", "k_cbhg_front<1, 144, 128, 16>", "k_cbhg_front<2, 80, 80, 8>", "k_pointwise_chain<128> (the last projection in its entry)",
         "k_pointwise_chain<256> (the last projection in its entry)", "encoder prenet: one k_pointwise_chain launch", "k_head_sweep<512>"], [" -- no ", "k_front_combine"]),
    5: (["no k_pointwise_chain: taco_debug_set_bf3 bit 2", "point-wise layers on k_gemm_bf3", "k_cbhg_front<", "k_front_combine", "1 projection on k_gemm_bf3",
         "encoder prenet: one GEMM launch per layer", "k_zero_fill in front", "k_head_sweep<512>"], ["k_pointwise_chain<"]),
    9: (["conv bank and proj_1 on k_gemm_bf3", "no k_cbhg_front: taco_debug_set_bf3 bit 3", "k_pointwise_chain<256>", "encoder prenet: one k_pointwise_chain launch"],
        ["k_cbhg_front<", "k_front_combine", "in its entry"]),
    17: (["k_cbhg_front<1, 144, 128, 16> + k_front_combine", "no fused chain entry: taco_debug_set_bf3 bit 4", "k_pointwise_chain<256>"], ["in its entry"]),
    33: (["linear head: 1 launch of k_gemm_bf3 -- no k_head_sweep: taco_debug_set_bf3 bit 5", "k_cbhg_front<", "in its entry"], ["k_head_sweep<"]),
    65: (["six products (k_gemm_bf3<..., X6>", "conv bank and proj_1 on k_gemm_bf3<..., X6>", "point-wise layers on k_gemm_bf3<..., X6>", "the six-product level has no fused kernels",
          "encoder prenet: one GEMM launch per layer", "linear head: 1 launch of k_gemm_bf3<..., X6>"], ["k_cbhg_front<", "k_pointwise_chain<", "k_head_sweep<", "three products"]),
    0: (["exact-fp32 MFMA (k_gemm)", "conv bank and proj_1 on k_gemm,", "point-wise layers on k_gemm ", "exact fp32 is switched on", "encoder prenet: one GEMM launch per layer",
         "linear head: 1 launch of k_gemm "], ["k_gemm_bf3", "k_cbhg_front<", "k_pointwise_chain<", "k_head_sweep<", "split-bf16"]),
}


def test_feed_forward_plan_agrees_with_the_launches():
    """ff_plan / prenet_chain_why / head_sweep_why (csrc/taco_lib.hip) are what the launches follow and what engine_plan words.  There is no
    protocol word for feed-forward kernels, but a captured plan counts its kernel nodes: in every taco_debug_set_bf3 mode the node count moves
    against mode 1 by exactly the launches the sentence states, and the sentence names the kernels include/taco_debug.h documents for the
    mode.  Then a model outside the presets: one launch per layer, with the reason."""
    from util import tiny_hp
    B, T_in = 8, 24
    ohp = O.OracleHParams(max_iters=16)
    assert B * ohp.max_iters * ohp.reduction_factor >= 256          # (the head sweep serves 256 rows and more)
    m = build_model(ohp, O.init_weights(ohp, 1, 451))
    nodes, stated = {}, {}
    for mode in (1, 5, 9, 17, 33, 65, 0, 1):
        m._lib.taco_debug_set_bf3(m._handle, mode, 0)
        m._plans.clear()                                             # a captured plan keeps the kernels it was captured with
        plan = m.engine_plan(B, T_in)
        clauses, count = _ff_clauses(plan)
        n = m.plan_for(B, T_in).num_nodes
        print(mode, n, count, plan.split("; feed-forward: ")[1])
        assert nodes.setdefault(mode, n) == n and stated.setdefault(mode, count) == count, (mode, n, count)      # (mode 1 twice: the hook leaves nothing behind)
        ff = "; ".join(clauses[k] for k in ("feed-forward", "encoder CBHG", "post-net CBHG", "encoder prenet", "linear head")) + " "
        present, absent = FF_MODES[mode]
        assert all(w in ff for w in present) and not any(w in ff for w in absent), (mode, ff)
    m.check_device_errors()
    for mode in nodes:
        assert nodes[mode] - nodes[1] == stated[mode] - stated[1], (mode, nodes, stated)
    assert stated[1] == 2 + 2 + 1 + 1 and len(set(nodes.values())) >= 3, (nodes, stated)      # front + chain per CBHG, prenet, head; the modes do move the count
    # outside the presets: every layer a launch of its own
    thp = tiny_hp()
    t = build_model(thp, O.init_weights(thp, 1, 452))
    tn = {}
    for mode in (1, 0):
        t._lib.taco_debug_set_bf3(t._handle, mode, 0)
        t._plans.clear()
        clauses, count = _ff_clauses(t.engine_plan(3, 9))
        tn[mode] = (t.plan_for(3, 9).num_nodes, count)
        print(mode, tn[mode], clauses)
        kernel = "k_gemm_bf3" if mode else "k_gemm"
        for name in ("encoder CBHG", "post-net CBHG"):
            assert "conv bank and proj_1 on " + kernel in clauses[name] and "point-wise layers on " + kernel in clauses[name], clauses
            assert ("no k_cbhg_front: widths outside the presets" in clauses[name] and "no k_pointwise_chain: widths outside the presets" in clauses[name]) == (mode == 1), clauses
        assert "one GEMM launch per layer" in clauses["encoder prenet"] and "linear head: 1 launch of " + kernel + " -- no k_head_sweep: " in clauses["linear head"], clauses
    assert tn[1] == tn[0], tn
    t.check_device_errors()


def test_engine_plan_tells_a_training_shadow_model_its_gemm_level():
    """A trainer's forward GEMMs run on the six-product split by default (taco_train_set_exact_gemm mode 4), one launch per layer, and on
    k_gemm after set_exact_gemm(1): Trainer.engine_plan names the level and the kernel of each (it said k_gemm for both)."""
    import taco_amd
    from util import to_product_hp
    hp = O.OracleHParams(max_iters=4)
    tr = taco_amd.Trainer(to_product_hp(hp), O.init_weights(hp, 1, 461))
    clauses, _ = _ff_clauses(tr.engine_plan(6, 11, 4 * hp.reduction_factor))
    print(clauses)
    assert "six products (k_gemm_bf3<..., X6>" in clauses["feed-forward"], clauses
    for name in ("encoder CBHG", "post-net CBHG", "encoder prenet", "linear head"):
        assert "of k_gemm_bf3<..., X6>" in clauses[name] and "k_cbhg_front" not in clauses[name] and "k_pointwise_chain" not in clauses[name], clauses
    tr.set_exact_gemm(1)
    clauses, _ = _ff_clauses(tr.engine_plan(6, 11, 4 * hp.reduction_factor))
    print(clauses)
    assert "exact-fp32 MFMA (k_gemm)" in clauses["feed-forward"], clauses
    assert all("of k_gemm" in c and "k_gemm_bf3" not in c for k, c in clauses.items() if k != "feed-forward"), clauses
    tr.close()


def test_training_step_refuses_a_misaligned_workspace():
    """taco_train_forward_backward with the workspace pointer advanced by 4 bytes: TACO_ERR_ARG that names the alignment, before anything is
    enqueued (the tape's four-column kernels rely on the 16-byte alignment of what Carver hands out); the next, aligned step of the same
    trainer equals the step of a fresh trainer to the bit."""
    import torch
    import taco_amd
    from util import to_product_hp
    n, B, T_in = 3, 4, 9
    hp = O.OracleHParams(max_iters=n)
    w = O.init_weights(hp, 1, 471)
    ids, L = O.synthetic_inputs(B, T_in, 472, ragged=True)
    rs = np.random.RandomState(473)
    T_out = n * hp.reduction_factor
    batch = (ids, L, rs.rand(B, T_out, hp.num_mels).astype(np.float32), rs.rand(B, T_out, hp.num_freq).astype(np.float32), np.ones(B, np.float32))
    tr = taco_amd.Trainer(to_product_hp(hp), w)
    nb = int(tr._lib.taco_train_workspace_bytes(tr._h, B, T_in, T_out))
    big = torch.empty(nb + 64, dtype=torch.uint8, device=tr.device)
    assert big.data_ptr() % 16 == 0
    tr._ws = big[4:]                                     # large enough, so forward_backward hands it on as it is
    assert tr._ws.data_ptr() % 16 == 4 and tr._ws.numel() >= nb
    before = tr.params.clone()
    with pytest.raises(taco_amd._lib.TacoError) as e:
        tr.forward_backward(*batch)
    assert e.value.code == taco_amd._lib.TACO_ERR_ARG and "not 16-byte aligned" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    tr.check_device_errors()
    assert torch.equal(tr.params, before)
    tr._ws = None
    fresh = taco_amd.Trainer(to_product_hp(hp), w)
    outs = []
    for t in (tr, fresh):
        step, loss = t.train_step(*batch)
        torch.cuda.synchronize()
        t.check_device_errors()
        outs.append((step, float(loss), t.grads.cpu().numpy().copy(), t.params.cpu().numpy().copy()))
    assert outs[0][0] == outs[1][0] == 1 and outs[0][1] == outs[1][1] and np.isfinite(outs[0][1])
    assert np.array_equal(outs[0][2], outs[1][2]) and np.array_equal(outs[0][3], outs[1][3])
    tr.close(); fresh.close()


def test_decoder_engine_hook_refuses_other_rows_per_group():
    """taco_debug_set_decoder_persist accepts 0 (automatic), 1, 2, 4, 8 rows per group; any other number is TACO_ERR_ARG and changes
    nothing: the model still decodes, on the engine and rows it had."""
    import torch
    import taco_amd
    n, B = 3, 8
    ohp = O.OracleHParams(max_iters=n)
    m = build_model(ohp, O.init_weights(ohp, 1, 441))
    enc = np.random.RandomState(442).uniform(-1, 1, (B, 17, 2 * ohp.enc_rnn_size)).astype(np.float32)
    m.set_decoder_engine(1, 2)
    assert "k_decoder_xcd<2>" in m.engine_plan(B, 17)
    mel0, al0, _, _ = m.decoder(enc, n)
    for rows in (3, 5, 6, 7, 16, -1):
        with pytest.raises(taco_amd._lib.TacoError):
            m.set_decoder_engine(1, rows)
        with pytest.raises(taco_amd._lib.TacoError):
            m.set_decoder_engine(0, rows)      # (nor does a refused call switch the engine off)
    for rows in (0, 1, 2, 4, 8):
        m.set_decoder_engine(1, rows)
    m.set_decoder_engine(1, 2)
    assert "k_decoder_xcd<2>" in m.engine_plan(B, 17)
    mel1, al1, _, _ = m.decoder(enc, n)
    torch.cuda.synchronize()
    assert m.decoder_engine_info()["protocol"] in (1, 2)
    m.check_device_errors()
    assert np.array_equal(mel1.cpu().numpy(), mel0.cpu().numpy()) and np.array_equal(al1.cpu().numpy(), al0.cpu().numpy())


def test_a_device_fault_is_reported_by_the_forward_that_saw_it():
    """the sticky device error word, raised by hand here (taco_debug_raise_device_error), comes back in the stop word
    of the next forward (negative), Tacotron.run and PlanPool.result raise on it and acknowledge it, and the forward after that is
    clean and equal to the one before the fault."""
    import torch
    import taco_amd
    ohp = O.OracleHParams(max_iters=6)
    m = build_model(ohp, O.init_weights(ohp, 1, 411))
    ids, L = O.synthetic_inputs(4, 10, 412)
    lin0, al0 = m.run(ids, L, honor_stop=False)
    lin0 = lin0.clone()
    m.raise_device_error_for_test()
    with pytest.raises(taco_amd._lib.TacoError):
        m.run(ids, L, honor_stop=False)
    lin1, _ = m.run(ids, L, honor_stop=False)            # acknowledged by the failed call: clean again
    torch.cuda.synchronize()
    assert torch.equal(lin1, lin0)
    pool = taco_amd.tacotron.PlanPool(m, 4, 10, lanes=1)
    t = pool.submit(ids, L); ok = pool.result(t)
    m.raise_device_error_for_test()
    t = pool.submit(ids, L)
    with pytest.raises(taco_amd._lib.TacoError):
        pool.result(t)
    t = pool.submit(ids, L); again = pool.result(t)
    assert torch.equal(again["linear"], ok["linear"])
    pool.close()
