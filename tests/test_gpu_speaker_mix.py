"""Speaker mixtures at inference (include/taco_abi.h, "speaker mixtures"; the *_mix entry points, k_mix_rows) against the oracle.

The oracle knows speaker ids only.  A mixture is indistinguishable from an extra trained speaker whose table row is the mixed row, so
the reference of a run with weights W [B, NS] is the oracle on tables with the B rows (W @ table, formed in float64, rounded to
float32) appended, asked for speakers NS .. NS + B - 1.  Mixed rows differ from either parent by 0.15 .. 0.25 in mel at these
sizes, three orders above the tolerances, which are the project's own for the same widths (tests/test_gpu_e2e.py): 2e-4 at the tiny
widths, 1e-3 at full width, alignment argmax identical."""
import ctypes as C

import numpy as np
import pytest

import taco_oracle as O
from util import tiny_hp, build_model, to_product_hp, maxabs, argmax_match, dev, ptr, stream

pytestmark = pytest.mark.gpu

NS = 3
W3 = np.array([[.5, .5, 0], [.25, 0, .75], [0, 1, 0]], np.float32)
CONFIGS = [("deepvoice", {}), ("simple", {"attention_type": "bah_mon"}), ("simple", {"attention_type": "bah"}),
           ("deepvoice", {"speaker_embedding_size": 1})]
CONFIG_IDS = ["deepvoice", "simple-bah_mon", "simple-bah", "deepvoice-tables"]


def _is_table(name):
    return name == "speaker_embedding" or (name.startswith("spk/") and name.endswith("/table"))


def augmented(w, W):
    """The weights with one more speaker per row of W: its table rows are the mixed rows."""
    out = dict(w)
    for k, v in w.items():
        if _is_table(k):
            out[k] = np.concatenate([v, (np.asarray(W, np.float64) @ v.astype(np.float64)).astype(np.float32)], 0)
    return out


def mix_ref(w, ohp, ids, L, W, ns, **kw):
    B = len(W)
    return O.forward(augmented(w, W), ohp, ids, L, speaker_id=(ns + np.arange(B)).astype(np.int32), num_speakers=ns + B, **kw)


def _run(m, ids, L, **kw):
    import torch
    lin, al = m.run(inputs=ids, input_lengths=L, **kw)
    torch.cuda.synchronize()
    return m.mel_outputs.cpu().numpy(), lin.cpu().numpy(), al.cpu().numpy()


def _check(hip, ref, tol):
    mel, lin, al = hip
    assert mel.shape == ref["mel"].shape and lin.shape == ref["linear"].shape and al.shape == ref["alignments"].shape
    e = maxabs(mel, ref["mel"]), maxabs(lin, ref["linear"]), maxabs(al, ref["alignments"])
    print("max|err| mel %.3g linear %.3g alignments %.3g (tolerance %g)" % (e + (tol,)))
    assert e[0] < tol, "mel"
    assert e[1] < tol, "linear"
    assert e[2] < tol, "alignments"
    n, bad = argmax_match(al, ref["alignments"])
    assert bad == 0, "alignment argmax differs at %d of %d steps" % (bad, n)


def _tiny(model_type, kw, seed=61, ns=NS):
    ohp = tiny_hp(model_type=model_type, **kw)
    w = O.init_weights(ohp, ns, seed)
    return ohp, w, build_model(ohp, w, num_speakers=ns)


@pytest.mark.parametrize("model_type,kw", CONFIGS, ids=CONFIG_IDS)
def test_mixtures_against_the_augmented_oracle(model_type, kw):
    ohp, w, m = _tiny(model_type, kw)
    ids, L = O.synthetic_inputs(3, 9, 62, ragged=True)
    ref = mix_ref(w, ohp, ids, L, W3, NS)
    hip = _run(m, ids, L, speaker_weights=W3)
    _check(hip, ref, 2e-4)
    # the mixture is a voice of its own: rows 0 and 1 are far from both parents, row 2 (one-hot) is speaker 1
    for parent in ([0, 0, 1], [1, 2, 1]):
        mel_p = _run(m, ids, L, speaker_id=np.array(parent, np.int32))[0]
        n = min(mel_p.shape[1], hip[0].shape[1])
        for b in range(2):
            assert np.abs(mel_p[b, :n] - hip[0][b, :n]).max() > 1e-2, (parent, b)
    m.close()


@pytest.mark.parametrize("model_type,kw", [CONFIGS[0], CONFIGS[1], CONFIGS[3]], ids=[CONFIG_IDS[0], CONFIG_IDS[1], CONFIG_IDS[3]])
def test_one_hot_weights_equal_ids_bit_for_bit(model_type, kw):
    ohp, w, m = _tiny(model_type, kw)
    ids, L = O.synthetic_inputs(3, 9, 63, ragged=True)
    spk = np.array([2, 0, 1], np.int32)
    by_id = _run(m, ids, L, speaker_id=spk)
    by_w = _run(m, ids, L, speaker_weights=np.eye(NS, dtype=np.float32)[spk])
    for name, a, b in zip(("mel", "linear", "alignments"), by_id, by_w):
        assert np.array_equal(a, b), name
    m.close()


@pytest.mark.parametrize("model_type", ["deepvoice", "simple"])
def test_stage_entry_points_with_weights(model_type):
    """encoder / decoder (fed the oracle's encoder output) / postnet (fed the oracle's mel) with speaker_weights; the tolerances of
    test_gpu_e2e.py::test_stage_level_encoder_decoder_postnet."""
    import torch
    ohp, w, m = _tiny(model_type, {}, seed=64)
    ids, L = O.synthetic_inputs(3, 10, 65, ragged=True)
    taps = {}
    ref = mix_ref(w, ohp, ids, L, W3, NS, taps=taps)
    enc = m.encoder(ids, L, speaker_weights=W3)
    torch.cuda.synchronize()
    assert maxabs(enc.cpu().numpy(), taps["encoder"]) < 1e-4
    mel, al, stop, dbg = m.decoder(taps["encoder"], ohp.max_iters, speaker_weights=W3, debug=True)
    torch.cuda.synchronize()
    assert int(stop.item()) == ohp.max_iters
    dbg = dbg.cpu().numpy()
    As, D = ohp.attention_state_size, 2 * ohp.enc_rnn_size
    for t, st in enumerate(taps["steps"]):
        assert maxabs(dbg[t, :, :As], st["h_att"]) < 2e-4, "h_att step %d" % t
        assert maxabs(dbg[t, :, As:As + D], st["ctx"]) < 2e-4, "ctx step %d" % t
        for i, h in enumerate(st["h"]):
            o = As + D + i * ohp.dec_rnn_size
            assert maxabs(dbg[t, :, o:o + ohp.dec_rnn_size], h) < 2e-4, "h_%d step %d" % (i + 1, t)
    assert maxabs(mel.cpu().numpy(), ref["mel"]) < 2e-4
    assert maxabs(al.cpu().numpy(), ref["alignments"]) < 2e-4
    lin, post = m.postnet(ref["mel"], return_post=True, speaker_weights=W3)
    torch.cuda.synchronize()
    # ('simple': the oracle's tap is concat(tiled speaker_embed, post), tacotron.py:226-233 -- the post-net output is its last columns)
    assert maxabs(post.cpu().numpy(), taps["post"][..., -post.shape[-1]:]) < 2e-4
    assert maxabs(lin.cpu().numpy(), ref["linear"]) < 2e-4
    m.close()


@pytest.mark.parametrize("model_type", ["simple", "deepvoice"])
def test_full_width_on_the_persistent_decoder(model_type):
    """The reference widths: the persistent decoder loop, whose 'simple' speaker term comes from k_dx_rowbias fed with mixed rows."""
    ns = 4
    ohp = O.OracleHParams(max_iters=8, model_type=model_type)
    w = O.init_weights(ohp, ns, 66)
    ids, L = O.synthetic_inputs(5, 40, 67, ragged=True)
    W = np.array([[.2, .3, 0, .5], [0, 0, 1, 0], [.6, 0, .4, 0], [.1, .2, .3, .4], [0, 1.5, -.5, 0]], np.float32)
    m = build_model(ohp, w, num_speakers=ns)
    _check(_run(m, ids, L, speaker_weights=W), mix_ref(w, ohp, ids, L, W, ns), 1e-3)
    assert m.decoder_engine_info()["has_pack"]
    m.check_device_errors()
    m.close()


def test_more_than_64_rows_advance_the_weights_with_the_passes():
    """67 rows run as two passes; rows of the second pass read weights from b0 * num_speakers on."""
    B, T_in = 67, 7
    ohp, w, m = _tiny("deepvoice", {"max_iters": 4}, seed=68)
    ids, L = O.synthetic_inputs(B, T_in, 69, ragged=True)
    W = np.random.RandomState(70).uniform(0, 1, (B, NS)).astype(np.float32)
    W /= W.sum(1, keepdims=True)
    assert len({tuple(r) for r in W.tolist()}) == B
    ref = mix_ref(w, ohp, ids, L, W, NS)
    hip = _run(m, ids, L, speaker_weights=W)
    for b0, b1 in ((0, 34), (34, 64), (64, 67)):
        for a, r in zip(hip, (ref["mel"], ref["linear"], ref["alignments"])):
            assert maxabs(a[b0:b1], r[b0:b1]) < 2e-4, (b0, b1)
    _check(hip, ref, 2e-4)
    m.close()


def test_replays_of_one_plan_read_the_weights_buffer():
    ohp, w, m = _tiny("simple", {}, seed=71)
    B, T_in = 3, 9
    ids, L = O.synthetic_inputs(B, T_in, 72, ragged=True)
    W2 = np.array([[0, .3, .7], [1, 0, 0], [.4, .4, .2]], np.float32)
    refs = [mix_ref(w, ohp, ids, L, W, NS) for W in (W3, W2)]
    first = _run(m, ids, L, speaker_weights=W3)
    plan = m.plan_for(B, T_in, mix=True)
    second = _run(m, ids, L, speaker_weights=W2)
    assert m.plan_for(B, T_in, mix=True) is plan and len(m._plans) == 1
    assert plan.speaker_weights.shape == (B, NS)
    _check(first, refs[0], 2e-4)
    _check(second, refs[1], 2e-4)
    spk = np.array([1, 2, 0], np.int32)
    by_id = _run(m, ids, L, speaker_id=spk)
    assert m.plan_for(B, T_in) is not plan and len(m._plans) == 2
    _check(by_id, O.forward(w, ohp, ids, L, speaker_id=spk, num_speakers=NS), 2e-4)
    m.close()


def test_plan_pool_submit_with_weights():
    ohp, w, m = _tiny("deepvoice", {}, seed=73)
    B, T_in = 3, 8
    pool = m.plan_pool(B, T_in, lanes=1, speaker_mix=True)
    W2 = np.array([[.1, .1, .8], [0, 0, 1], [.5, .25, .25]], np.float32)
    for k, W in enumerate((W3, W2)):
        ids, L = O.synthetic_inputs(B, T_in, 74 + k, ragged=True)
        r = pool.result(pool.submit(ids, L, speaker_weights=W))
        got = tuple(r[key].cpu().numpy() for key in ("mel", "linear", "alignments"))
        _check(got, mix_ref(w, ohp, ids, L, W, NS, honor_stop=False), 2e-4)
    with pytest.raises(Exception):
        pool.submit(ids, L, speaker_id=np.zeros(B, np.int32), speaker_weights=W3)
    pool.close()
    ids_pool = m.plan_pool(B, T_in, lanes=1)
    with pytest.raises(Exception):
        ids_pool.submit(ids, L, speaker_weights=W3)
    ids_pool.close()
    m.check_device_errors()
    m.close()


def test_errors_raise_before_anything_is_launched():
    import torch
    import taco_amd
    from taco_amd import _lib
    B, T_in = 3, 9
    ids, L = O.synthetic_inputs(B, T_in, 76, ragged=True)
    # weights on a single-speaker model: refused by the Python surface and by the library itself
    ohp1 = tiny_hp()
    w1 = O.init_weights(ohp1, 1, 77)
    single = build_model(ohp1, w1)
    with pytest.raises(_lib.TacoError):
        single.run(inputs=ids, input_lengths=L, speaker_weights=np.ones((B, 1), np.float32))
    for call in (single.encoder, ):
        with pytest.raises(_lib.TacoError):
            call(ids, L, speaker_weights=np.ones((B, 1), np.float32))
    lib = single._lib
    some = dev(np.ones((B, 1), np.float32))
    z = C.c_void_p(0)
    rc = lib.taco_forward_infer_mix(single._handle, stream(), z, z, ptr(some), B, T_in, 4, z, z, z, z, z, z, 0)
    assert rc == _lib.TACO_ERR_ARG and b"single-speaker" in lib.taco_last_error()
    rc = lib.taco_encoder_forward_mix(single._handle, stream(), z, z, ptr(some), B, T_in, z, z, 0)
    assert rc == _lib.TACO_ERR_ARG and b"single-speaker" in lib.taco_last_error()
    _check(_run(single, ids, L), O.forward(w1, ohp1, ids, L), 2e-4)
    single.close()
    # a multi-speaker model: null weights, both selectors at once, one column too many
    ohp, w, m = _tiny("simple", {}, seed=78)
    for fn, args in ((lib.taco_forward_infer_mix, (z, z, z, B, T_in, 4, z, z, z, z, z, z, 0)),
                     (lib.taco_decoder_forward_mix, (z, z, B, T_in, 4, z, z, z, z, z, z, z, 0)),
                     (lib.taco_postnet_forward_mix, (z, z, B, 12, z, z, z, 0))):
        rc = fn(m._handle, stream(), *args)
        assert rc == _lib.TACO_ERR_ARG and b"speaker_weights required" in lib.taco_last_error()
    plan = C.c_void_p()
    rc = lib.taco_plan_create_mix(m._handle, z, z, z, B, T_in, 4, z, z, z, z, z, z, 0, C.byref(plan))
    assert rc == _lib.TACO_ERR_ARG and not plan.value
    spk = np.array([0, 1, 2], np.int32)
    with pytest.raises(_lib.TacoError):
        m.run(inputs=ids, input_lengths=L, speaker_id=spk, speaker_weights=W3)
    with pytest.raises(_lib.TacoError):
        m.postnet(np.zeros((B, 6, ohp.num_mels), np.float32), speaker_id=spk, speaker_weights=W3)
    with pytest.raises(_lib.TacoError):
        m.run(inputs=ids, input_lengths=L, speaker_weights=np.ones((B, NS + 1), np.float32))
    assert len(m._plans) == 0          # none of the refused calls got as far as a plan
    torch.cuda.synchronize()
    m.check_device_errors()
    _check(_run(m, ids, L, speaker_weights=W3), mix_ref(w, ohp, ids, L, W3, NS), 2e-4)
    m.close()
    assert taco_amd.speaker_weights is not None


def test_synthesizer_blends_speakers(tmp_path):
    import taco_amd
    ohp = tiny_hp(model_type="simple", num_freq=65, max_iters=20)
    hp = to_product_hp(ohp)
    hp.add_hparam("sample_rate", 1600)
    hp.add_hparam("griffin_lim_iters", 3)
    w = O.init_weights(ohp, NS, 79)
    taco_amd.save_hparams(str(tmp_path), hp)
    taco_amd.weights.save_weights(str(tmp_path / "model.ckpt-1.safetensors"), w)
    s = taco_amd.Synthesizer().load(str(tmp_path), num_speakers=NS)
    ids, L = O.synthetic_inputs(2, 9, 80)
    lin, al = s.synthesize(tokens=ids, speaker_ids={0: 0.5, 2: 0.5})
    W = np.array([[.5, 0, .5]] * 2, np.float32)
    lin_m, al_m = s.model.run(inputs=ids.astype(np.int32), input_lengths=L, speaker_weights=W)
    assert np.array_equal(lin, lin_m.cpu().numpy()) and np.array_equal(al, al_m.cpu().numpy())
    ref = mix_ref(w, ohp, ids, L, W, NS)
    assert maxabs(lin, ref["linear"]) < 2e-4 and maxabs(al, ref["alignments"]) < 2e-4
    # per-row list: the same tokens three times, so the rows differ by voice alone
    same = np.repeat(ids[:1], 3, 0)
    kw = dict(tokens=same, attention_trim=False, pcm=False, vocoder="tensorflow")      # the deterministic vocoder: no per-row random phases
    wavs = s.synthesize_audio(speaker_ids=[0, {0: .5, 1: .5}, 1], **kw)
    assert len(wavs) == 3 and len({len(x) for x in wavs}) == 1 and all(np.isfinite(x).all() for x in wavs)
    d0, d2 = np.abs(wavs[1] - wavs[0]).max(), np.abs(wavs[1] - wavs[2]).max()
    print("middle row vs row 0: %.3g, vs row 2: %.3g (peak %.3g)" % (d0, d2, np.abs(wavs[1]).max()))
    assert d0 > 0 and d2 > 0
    by_id = s.synthesize_audio(speaker_ids=[0, 0, 1], **kw)      # an all-int list stays on the id path; rows are independent
    assert np.array_equal(by_id[0], wavs[0]) and np.array_equal(by_id[2], wavs[2]) and np.array_equal(by_id[1], by_id[0])
    s.close()
