"""The training block of the decoder alone (decoder_forward_train + decoder_backward through taco_train_debug_decoder) against float64
autograd of tests/torch_formulation.py::decoder: at the reference widths the two persistent whole-chip kernels, k_decoder_xcd<RG, true> and
k_decoder_bwd_xcd<RG>, at every rows-per-group; elsewhere, and again at the reference widths, the launch-per-stage engines.  The upstream
gradient is an input and the seeds keep the prenet's ReLUs and the monotonic clips at a distance (tests/decoder_reference.py, checked on
the CPU by tests/test_decoder_reference_host.py), so EVERY tensor on its own -- mel, alignments, d(encoder output), d(initial states),
d(speaker rows) and each parameter gradient -- is held to 8 x the float32 restatement's own error against float64.  The whole-model
tests of tests/test_gpu_train.py bound a tensor by 2e-3 of max(max|g_k|, 1e-3 * |g|), |g| the norm of the whole model's gradient: a floor
that lies hundreds of times above the whole gradient of the attention's query layer.

Measured ratios (max|hip - f64| / bar_k, and the default engines -- also with every eligible weight gradient from pre-split planes -- against
the exact ones over 1e-3 * s_k): profiles/r22_decoder_block_ratios.txt."""
import ctypes as C

import numpy as np
import pytest

import decoder_reference as R
from util import to_product_hp, dev, ptr, stream

pytestmark = pytest.mark.gpu

DEFAULT_VS_EXACT = 1e-3       # of s_k: the project's figure for the split-bf16 engines against the exact ones (tests/test_gpu_train.py)


def _call(tr, case, ref):
    """One call of the hook on the case's inputs: ({tensor name: float64 array}, paths word, the gradient buffer as downloaded)."""
    import torch
    import taco_amd
    inp, hp, B, T_in, n = ref.inp, ref.hp, case.B, case.T_in, case.n
    D, As, Hd, rM = R.dims(hp)
    L = hp.dec_layer_num
    grads = torch.full((tr.num_params,), float("nan"), dtype=torch.float32, device="cuda")
    inside = np.zeros(tr.num_params, bool)
    for name, (o, c) in tr.offsets.items():
        if R.in_scope(name):
            grads[o:o + c] = 0.0
            inside[o:o + c] = True
    enc, teacher, dmel = dev(inp["enc"].reshape(B * T_in, D)), dev(inp["teacher"]), dev(inp["dmel"])
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    att_init = None if inp["att_init"] is None else dev(inp["att_init"])
    datt_init = None if att_init is None else nan(B, As)
    dec_inits = None if inp["dec_inits"] is None else [dev(a) for a in inp["dec_inits"]]
    ddec_inits = None if dec_inits is None else [nan(B, Hd) for _ in range(L)]
    spk = None if inp["spk"] is None else dev(inp["spk"])
    dspk = None if spk is None else nan(*spk.shape)
    table = lambda ts: None if ts is None else (C.c_void_p * L)(*[t.data_ptr() for t in ts])
    dec_tab, ddec_tab = table(dec_inits), table(ddec_inits)
    mel, align, denc = nan(B, n, rM), nan(B, T_in, n), nan(B * T_in, D)
    nb = int(tr._lib.taco_train_debug_decoder_workspace_bytes(tr._h, B, T_in, n))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ws[:min(nb, 64 << 20)] = 0xFF                 # the tape reads nothing it did not write: NaN bit patterns in front
    word = np.zeros(1, np.uint32)
    args = (tr._h, stream(), ptr(tr.params), ptr(grads), ptr(enc), ptr(teacher), ptr(dmel), ptr(att_init), dec_tab, ptr(spk), B, T_in, n,
            ptr(mel), ptr(align), ptr(denc), ptr(datt_init), ddec_tab, ptr(dspk))
    # too small a workspace and a misaligned one are refused, as the step refuses them
    assert tr._lib.taco_train_debug_decoder(*args, ptr(ws), nb - 1, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_STATE
    assert tr._lib.taco_train_debug_decoder(*args, C.c_void_p(ws.data_ptr() + 4), nb - 4, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_ARG
    taco_amd._lib.check(tr._lib.taco_train_debug_decoder(*args, ptr(ws), nb, C.c_void_p(word.ctypes.data)))
    torch.cuda.synchronize()
    tr.check_device_errors()
    g = grads.cpu().numpy()
    assert np.isnan(g[~inside]).all(), "the hook wrote gradients outside decoder/ and attention/"
    assert np.isfinite(g[inside]).all()
    got = {"mel": mel, "alignments": align, "denc": denc}
    if datt_init is not None:
        got["datt_init"] = datt_init
    for i, t in enumerate(ddec_inits or []):
        got["ddec_init_%d" % (i + 1)] = t
    if dspk is not None:
        got["dspk"] = dspk
    got = {k: v.cpu().numpy().astype(np.float64).reshape(ref.ref64[k].shape) for k, v in got.items()}
    for name, (o, c) in tr.offsets.items():
        if R.in_scope(name):
            got[name] = g[o:o + c].astype(np.float64).reshape(ref.ref64[name].shape)
    assert set(got) == set(ref.ref64)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return got, int(word[0]), g


def _twice(tr, case, ref):
    got, word, g = _call(tr, case, ref)
    got2, word2, g2 = _call(tr, case, ref)
    assert word2 == word
    # ordered sums (taco_train_set_deterministic, the default): two calls give the same bits
    assert g.tobytes() == g2.tobytes() and all(np.array_equal(got[k], got2[k]) for k in got)
    return got, word


def _table(tag, case, ratios):
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])
    print("decoder-ratios %-30s %-26s worst %.3f (%s)" % (case.id, tag, worst[0][1], worst[0][0]))
    for k, r in worst:
        print("decoder-ratios     %-30s %-26s %-44s %.3f" % (case.id, tag, k, r))


def _check_word(case, word, want, persistent_launches, tag):
    """The engine bits are the case's; of the protocol bits a call with a persistent launch shows what the census found -- write-through
    alone where it is forced -- and a call without one shows none."""
    assert word & ~R.P_PROTOCOLS == want, "%s: paths %#x, expected %#x" % (tag, word, want)
    proto = word & R.P_PROTOCOLS
    if not persistent_launches:
        assert proto == 0, (tag, hex(word))
    elif case.write_through:
        assert proto == R.P_WRITE_THROUGH, (tag, hex(word))
    else:
        assert proto != 0, (tag, hex(word))
    print("decoder-paths %-30s %-26s %#06x%s%s" % (case.id, tag, word, " xcd-local" if proto & R.P_XCD_LOCAL else "",
                                                  " write-through" if proto & R.P_WRITE_THROUGH else ""))


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_decoder_training_block_against_float64_autograd(case):
    import taco_amd
    ref = R.reference(case)
    assert ref.admissible()
    tr = taco_amd.Trainer(to_product_hp(ref.hp), ref.inp["w"], num_speakers=case.speakers)
    try:
        whole_chip = tr.decoder_engine_info()["compute_units"] >= 256
        word_a = case.paths if whole_chip else case.paths_partition
        on_chip = bool(word_a & R.P_FWD_PERSISTENT)
        if case.write_through:
            tr.set_decoder_engine(2)
        params_before = tr.params.cpu().numpy().copy()
        # ---- (b) the trainer as created: six-product forward, split-bf16 data and weight gradients, planes for large problems ----
        dflt, w_dflt = _twice(tr, case, ref)
        _check_word(case, w_dflt, word_a, on_chip, "default")
        tr.set_wgrad_planes(2)                      # every eligible weight gradient from pre-split planes (k_wp_split / k_wp_gemm)
        planes, w_planes = _twice(tr, case, ref)
        _check_word(case, w_planes, word_a, on_chip, "planes 2")
        n_planes = tr.planes_problems()
        tr.set_wgrad_planes(1)
        # ---- (a) exact engines against float64 ----
        tr.set_exact_gemm(1)
        tr.set_exact_wgrad(True)
        exact, w_exact = _twice(tr, case, ref)
        _check_word(case, w_exact, word_a, on_chip, "exact")
        _table("exact/f64 over bar", case, R.ratios(exact, ref.ref64, ref.bars))
        arms = [("exact", exact)]
        # ---- (c) reference widths: each loop on the launch-per-stage engine as well, held to float64 on its own ----
        if case.reference_widths:
            rg = (case.paths >> R.P_FWD_RG_SHIFT) & 15
            tr.set_bptt_engine(False)
            got, word = _twice(tr, case, ref)
            _check_word(case, word, R.forward_only(rg) if whole_chip else R.STAGES, on_chip, "exact, bptt per stage")
            _table("exact,bptt per stage/f64", case, R.ratios(got, ref.ref64, ref.bars))
            arms.append(("exact, bptt per stage", got))
            tr.set_decoder_engine(0)
            got, word = _twice(tr, case, ref)
            _check_word(case, word, R.STAGES, False, "exact, per stage")
            _table("exact,per stage/f64", case, R.ratios(got, ref.ref64, ref.bars))
            arms.append(("exact, per stage", got))
        for tag, got in arms:
            over = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN, case.margins)
            assert over == [], (tag, over[:6])
        # ---- (b) held against (a), per tensor, no global-norm floor ----
        unit = {k: DEFAULT_VS_EXACT * s for k, s in ref.scale.items()}
        print("decoder-planes %-30s weight gradients from pre-split planes at mode 2: %d" % (case.id, n_planes))
        for tag, got in (("default/exact over 1e-3 s", dflt), ("planes 2/exact over 1e-3 s", planes)):
            _table(tag, case, R.ratios(got, exact, unit))
            over = R.compare(got, exact, unit, 1.0)
            assert over == [], (tag, over[:6])
        # nothing of the parameters is touched
        assert np.array_equal(tr.params.cpu().numpy(), params_before)
    finally:
        tr.close()
