"""The two ENDS of the training step alone against float64 autograd (tests/ends_reference.py, checked on the CPU by
tests/test_ends_reference_host.py): through taco_train_debug_front the embedding gather, the encoder prenet and the speaker conditioning with
their backward (k_relu_bwd, run_wgrad with gathered rows, run_colsum, run_dgrad, k_embed_bwd_det / k_embed_bwd, the deepvoice speaker
layers and tables, the 'simple' speaker rows); through taco_train_debug_head the teacher-frame gather, the linear head at its odd width,
taco_loss_f32, k_l1_grad with loss_coeff and the priority band, the head's weight / bias / data gradients, the speaker rows of 'simple' and
dmel += dmel_post.  The upstream gradients are inputs, the seeds keep the prenet's ReLUs at a distance and the targets keep the L1 kinks at
a distance, so EVERY tensor on its own is held to 8 x the float32 restatement's own error against float64.  The whole-model tests of
tests/test_gpu_train.py bound these tensors by 2e-3 of max(max|g_k|, 1e-3 * |g|).

Measured ratios (max|hip - f64| / bar_k, and the default engines -- also with every eligible weight gradient from pre-split planes -- against
the exact ones over 1e-3 * s_k): profiles/r24_ends_block_ratios.txt."""
import ctypes as C

import numpy as np
import pytest

import ends_reference as R
from util import to_product_hp, dev, ptr, stream

pytestmark = pytest.mark.gpu

DEFAULT_VS_EXACT = 1e-3       # of s_k: the project's figure for the split-bf16 engines against the exact ones (tests/test_gpu_train.py)
DEFAULT_LOSS = 1e-5           # of max(1, |l64|): test_training_forward_matches_oracle's


def _grad_buffer(tr, kind):
    import torch
    grads = torch.full((tr.num_params,), float("nan"), dtype=torch.float32, device="cuda")
    inside = np.zeros(tr.num_params, bool)
    for name, (o, c) in tr.offsets.items():
        if R.in_scope(kind, name):
            grads[o:o + c] = 0.0
            inside[o:o + c] = True
    return grads, inside


def _workspace(nb):
    import torch
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ws[:] = 0xFF                  # nothing is read that was not written: NaN bit patterns in front
    return ws


def _finish(tr, kind, ref, got, grads, inside):
    import torch
    torch.cuda.synchronize()
    tr.check_device_errors()
    g = grads.cpu().numpy()
    assert np.isnan(g[~inside]).all(), "the hook wrote gradients outside its scope"
    assert np.isfinite(g[inside]).all()
    got = {k: v.cpu().numpy().astype(np.float64).reshape(ref.ref64[k].shape) for k, v in got.items()}
    for name, (o, c) in tr.offsets.items():
        if R.in_scope(kind, name):
            got[name] = g[o:o + c].astype(np.float64).reshape(ref.ref64[name].shape)
    assert set(got) == set(ref.ref64)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return got, g


def _call_front(tr, case, ref):
    """One call of taco_train_debug_front on the case's inputs: ({tensor name: float64 array}, paths word, the gradient buffer as downloaded)."""
    import torch
    import taco_amd
    inp, hp, B, T_in = ref.inp, ref.hp, case.B, case.T
    grads, inside = _grad_buffer(tr, "front")
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    ids, dpre = dev(inp["ids"].astype(np.int32)), dev(inp["dpre"].reshape(B * T_in, -1))
    sid = None if inp["speaker_id"] is None else dev(inp["speaker_id"].astype(np.int32))
    dvec = None if inp["dvec"] is None else [dev(a) for a in inp["dvec"]]
    vec = None if dvec is None else [nan(*a.shape) for a in inp["dvec"]]
    dspk = None if inp["dspk_emb"] is None else dev(inp["dspk_emb"])
    spk = nan(B, hp.speaker_embedding_size) if "spk_emb" in ref.ref64 else None
    table = lambda ts: None if ts is None else (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    pre = nan(B * T_in, hp.enc_prenet_sizes[-1])
    nb = int(tr._lib.taco_train_debug_front_workspace_bytes(tr._h, B, T_in))
    ws = _workspace(nb)
    word = np.zeros(1, np.uint32)
    args = (tr._h, stream(), ptr(tr.params), ptr(grads), ptr(ids), ptr(sid), ptr(dpre), table(dvec), ptr(dspk), B, T_in, ptr(pre), table(vec), ptr(spk))
    # too small a workspace and a misaligned one are refused, as the step refuses them
    assert tr._lib.taco_train_debug_front(*args, ptr(ws), nb - 1, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_STATE
    assert tr._lib.taco_train_debug_front(*args, C.c_void_p(ws.data_ptr() + 4), nb - 4, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_ARG
    taco_amd._lib.check(tr._lib.taco_train_debug_front(*args, ptr(ws), nb, C.c_void_p(word.ctypes.data)))
    got = {"pre": pre}
    if spk is not None:
        got["spk_emb"] = spk
    for nm, t in zip(R.vector_names(hp), vec or []):
        got["vec/" + nm] = t
    got, g = _finish(tr, "front", ref, got, grads, inside)
    # rows that no id of the batch names: exact zeros (the bars alone would let 8 bars of noise through)
    for k, rows in ref.zero_rows.items():
        assert rows and not got[k][rows].any(), k
    # gathers are copies
    for k in ("spk_emb",) + tuple("vec/" + nm for nm in R.vector_names(hp) if hp.speaker_embedding_size == 1):
        if k in got:
            assert np.array_equal(got[k], ref.ref32[k]), k
    return got, int(word[0]), g


def _call_head(tr, case, ref):
    """One call of taco_train_debug_head: ({tensor name: float64 array, 'losses': [4]}, 0, the gradient buffer as downloaded)."""
    import torch
    import taco_amd
    inp, hp, B, T_out = ref.inp, ref.hp, case.B, case.T
    Mm, Fq, Hp2, r = hp.num_mels, hp.num_freq, 2 * hp.post_rnn_size, hp.reduction_factor
    grads, inside = _grad_buffer(tr, "head")
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    opt = lambda a: None if a is None else dev(a)
    post, mel, mel_tgt, lin_tgt = dev(inp["post_out"]), dev(inp["mel"]), dev(inp["mel_tgt"]), dev(inp["lin_tgt"])
    coeff, dmel_post, spk = opt(inp["coeff"]), opt(inp["dmel_post"]), opt(inp["spk_emb"])
    dspk = None if spk is None else nan(*spk.shape)
    teacher, lin, losses, dmel, dpost = nan(B, T_out // r, Mm), nan(B * T_out, Fq), nan(4), nan(B * T_out, Mm), nan(B * T_out, Hp2)
    nb = int(tr._lib.taco_train_debug_head_workspace_bytes(tr._h, B, T_out))
    ws = _workspace(nb)
    args = (tr._h, stream(), ptr(tr.params), ptr(grads), ptr(post), ptr(mel), ptr(mel_tgt), ptr(lin_tgt), ptr(coeff), ptr(dmel_post), ptr(spk), B, T_out,
            int(inp["prioritize"]), int(inp["sample_rate"]), ptr(teacher), ptr(lin), ptr(losses), ptr(dmel), ptr(dpost), ptr(dspk))
    assert tr._lib.taco_train_debug_head(*args, ptr(ws), nb - 1) == taco_amd._lib.TACO_ERR_STATE
    assert tr._lib.taco_train_debug_head(*args, C.c_void_p(ws.data_ptr() + 4), nb - 4) == taco_amd._lib.TACO_ERR_ARG
    taco_amd._lib.check(tr._lib.taco_train_debug_head(*args, ptr(ws), nb))
    got = {"teacher": teacher, "lin": lin, "dmel": dmel, "dpost": dpost}
    if dspk is not None:
        got["dspk"] = dspk
    got, g = _finish(tr, "head", ref, got, grads, inside)
    # the teacher frames are the targets' frames, bit for bit
    assert np.array_equal(got["teacher"].astype(np.float32), inp["mel_tgt"][:, r - 1::r]), "teacher frames"
    got["losses"] = losses.cpu().numpy().astype(np.float64)
    assert np.isfinite(got["losses"]).all()
    return got, 0, g


def _twice(call, tr, case, ref, bit_equal=True):
    got, word, g = call(tr, case, ref)
    got2, word2, g2 = call(tr, case, ref)
    assert word2 == word
    if bit_equal:      # ordered sums (taco_train_set_deterministic, the default): two calls give the same bits
        assert g.tobytes() == g2.tobytes() and all(np.array_equal(got[k], got2[k]) for k in got)
    return got, word


def _table(tag, case, ratios):
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])
    print("ends-ratios %-30s %-26s worst %.3f (%s)" % (case.id, tag, worst[0][1], worst[0][0]))
    for k, r in worst:
        print("ends-ratios     %-30s %-26s %-44s %.3f" % (case.id, tag, k, r))


def _three_arms(call, tr, case, ref):
    """default (twice), planes 2 (twice), exact (twice); returns (default, planes, exact) and prints the planes count."""
    det = not case.atomic
    if case.atomic:
        tr.set_deterministic(False)
    params_before = tr.params.cpu().numpy().copy()
    want = case.paths if case.kind == "front" else 0
    dflt, w_dflt = _twice(call, tr, case, ref, det)
    tr.set_wgrad_planes(2)                          # every eligible weight gradient from pre-split planes (k_wp_split / k_wp_gemm)
    planes, w_planes = _twice(call, tr, case, ref, det)
    n_planes = tr.planes_problems()
    tr.set_wgrad_planes(1)
    tr.set_exact_gemm(1)
    tr.set_exact_wgrad(True)
    exact, w_exact = _twice(call, tr, case, ref, det)
    for tag, word in (("default", w_dflt), ("planes 2", w_planes), ("exact", w_exact)):
        assert word == want, "%s: paths %#x, expected %#x" % (tag, word, want)
    print("ends-planes %-30s weight gradients from pre-split planes at mode 2: %d" % (case.id, n_planes))
    assert np.array_equal(tr.params.cpu().numpy(), params_before)          # nothing of the parameters is touched
    return dflt, planes, exact


def _hold(case, ref, dflt, planes, exact):
    tensors = lambda d: {k: v for k, v in d.items() if k != "losses"}
    # ---- exact engines against float64, per tensor ----
    _table("exact/f64 over bar", case, R.ratios(tensors(exact), ref.ref64, ref.bars))
    over = R.compare(tensors(exact), ref.ref64, ref.bars, R.COMMON_MARGIN, case.margins)
    assert over == [], ("exact", over[:6])
    # ---- the default engines held against the exact ones, per tensor, no global-norm floor ----
    unit = {k: DEFAULT_VS_EXACT * s for k, s in ref.scale.items()}
    for tag, got in (("default/exact over 1e-3 s", dflt), ("planes 2/exact over 1e-3 s", planes)):
        _table(tag, case, R.ratios(tensors(got), tensors(exact), unit))
        over = R.compare(tensors(got), tensors(exact), unit, 1.0)
        assert over == [], (tag, over[:6])


@pytest.mark.parametrize("case", R.FRONT_CASES, ids=[c.id for c in R.FRONT_CASES])
def test_front_block_against_float64_autograd(case):
    import taco_amd
    ref = R.reference(case)
    assert ref.admissible()
    tr = taco_amd.Trainer(to_product_hp(ref.hp), ref.inp["w"], num_speakers=case.speakers)
    try:
        _hold(case, ref, *_three_arms(_call_front, tr, case, ref))
    finally:
        tr.close()


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=[c.id for c in R.HEAD_CASES])
def test_head_block_against_float64_autograd(case):
    """8000 Hz cases: before the priority band was clamped to num_freq as the reference's slice clamps it, the band term of the loss and of
    every d(linear) element was divided by the unclamped width (1239 instead of 983 columns at F = 1025; 44 instead of 35 at F = 36): the
    three 8000 Hz cases then stood at 1.1e5 bars on linear/kernel, linear/bias, dpost, d(speaker rows) and the loss, every other case passed
    (profiles/r24_ends_block_ratios.txt)."""
    import taco_amd
    ref = R.reference(case)
    assert ref.admissible()
    tr = taco_amd.Trainer(to_product_hp(ref.hp), ref.inp["w"], num_speakers=case.speakers)
    try:
        dflt, planes, exact = _three_arms(_call_head, tr, case, ref)
        names = ("loss", "mel_loss", "linear_loss", "loss_without_coeff")
        for i, nm in enumerate(names):
            print("ends-ratios     %-30s %-26s %-44s %.3f   (default: %.3e of max(1, |l64|))" % (
                case.id, "exact/f64 over bar", "losses/" + nm, abs(exact["losses"][i] - ref.losses64[i]) / ref.loss_bars[i],
                abs(dflt["losses"][i] - ref.losses64[i]) / max(1.0, abs(ref.losses64[i]))))
        _hold(case, ref, dflt, planes, exact)
        for i, nm in enumerate(names):
            assert abs(exact["losses"][i] - ref.losses64[i]) <= R.COMMON_MARGIN * ref.loss_bars[i], (nm, exact["losses"][i], ref.losses64[i])
            for got in (dflt, planes):
                assert abs(got["losses"][i] - ref.losses64[i]) <= DEFAULT_LOSS * max(1.0, abs(ref.losses64[i])), (nm, got["losses"][i], ref.losses64[i])
    finally:
        tr.close()
