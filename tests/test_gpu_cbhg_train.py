"""The training block of one CBHG alone (cbhg_forward_train + cbhg_backward through taco_train_debug_cbhg) against float64 autograd of
tests/torch_formulation.py::cbhg, widths that are no multiple of 4 included.  The upstream gradient is an input, the seeds keep the
ReLU / max-pool kinks at a distance (tests/cbhg_reference.py, checked on the CPU by tests/test_cbhg_reference_host.py), so every tensor
is held to 8 x the float32 restatement's own error against float64 -- about a hundred times tighter than the whole-model gradient tests
of tests/test_gpu_train.py, whose 2e-3 bound is owed to the kinks of the L1 loss.

Measured ratios (max|hip - f64| / bar_k, and the default engines against the exact ones over 1e-3 * s_k): profiles/r15_cbhg_block_ratios.txt."""
import ctypes as C

import numpy as np
import pytest

import cbhg_reference as R
from util import to_product_hp, dev, ptr, stream

pytestmark = pytest.mark.gpu

DEFAULT_VS_EXACT = 1e-3       # of s_k: the project's figure for the split-bf16 engines against the exact ones (tests/test_gpu_train.py)


def _call(tr, case, ref):
    """One call of the hook on the case's inputs: ({tensor name: float64 array}, paths word, the gradient buffer as uploaded back)."""
    import torch
    import taco_amd
    inp, B, T = ref.inp, case.B, case.T
    which = 0 if case.scope == R.ENC else 1
    in_dim, rnn = R.scope_dims(ref.hp, case.scope)[:2]
    grads = torch.full((tr.num_params,), float("nan"), dtype=torch.float32, device="cuda")
    inside = np.zeros(tr.num_params, bool)
    for name, (o, n) in tr.offsets.items():
        if name.startswith(case.scope + "/"):
            grads[o:o + n] = 0.0
            inside[o:o + n] = True
    x, dout = dev(inp["x"].reshape(B * T, in_dim)), dev(inp["dout"].reshape(B * T, 2 * rnn))
    lens = None if inp["lengths"] is None else dev(inp["lengths"])
    h0 = None if inp["h0"] is None else dev(inp["h0"])
    before = None if inp["before"] is None else dev(inp["before"])
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    out, din = nan(B * T, 2 * rnn), nan(B * T, in_dim)
    dh0 = None if h0 is None else nan(B, 2 * rnn)
    dbefore = None if before is None else nan(B, in_dim)
    nb = int(tr._lib.taco_train_debug_cbhg_workspace_bytes(tr._h, which, B, T))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    ws[:min(nb, 64 << 20)] = 0xFF                 # the tape reads nothing it did not write: NaN bit patterns in front
    word = np.zeros(1, np.uint32)
    args = (tr._h, stream(), which, ptr(tr.params), ptr(grads), ptr(x), ptr(lens), ptr(h0), ptr(before), ptr(dout), B, T, ptr(out), ptr(din),
            ptr(dh0), ptr(dbefore))
    # too small a workspace and a misaligned one are refused, as the step refuses them
    assert tr._lib.taco_train_debug_cbhg(*args, ptr(ws), nb - 1, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_STATE
    assert tr._lib.taco_train_debug_cbhg(*args, C.c_void_p(ws.data_ptr() + 4), nb - 4, C.c_void_p(word.ctypes.data)) == taco_amd._lib.TACO_ERR_ARG
    taco_amd._lib.check(tr._lib.taco_train_debug_cbhg(*args, ptr(ws), nb, C.c_void_p(word.ctypes.data)))
    torch.cuda.synchronize()
    tr.check_device_errors()
    g = grads.cpu().numpy()
    assert np.isnan(g[~inside]).all(), "the hook wrote gradients outside %s" % case.scope
    assert np.isfinite(g[inside]).all()
    got = {"out": out, "din": din}
    if dh0 is not None:
        got["dh0"] = dh0
    if dbefore is not None:
        got["dbefore"] = dbefore
    got = {k: v.cpu().numpy().astype(np.float64).reshape(ref.ref64[k].shape) for k, v in got.items()}
    for name, (o, n) in tr.offsets.items():
        if name.startswith(case.scope + "/"):
            if name.endswith(("/moving_mean", "/moving_variance")):
                assert not g[o:o + n].any(), name
            else:
                got[name] = g[o:o + n].astype(np.float64).reshape(ref.ref64[name].shape)
    assert set(got) == set(ref.ref64)
    for k, v in got.items():
        assert np.isfinite(v).all(), k
    return got, int(word[0]), g


def _twice(tr, case, ref, deterministic=True):
    got, word, g = _call(tr, case, ref)
    got2, word2, g2 = _call(tr, case, ref)
    assert word2 == word
    if deterministic:        # ordered sums: two calls give the same bits
        assert g.tobytes() == g2.tobytes() and all(np.array_equal(got[k], got2[k]) for k in got)
    return got, word


def _table(tag, case, ratios):
    worst = sorted(ratios.items(), key=lambda kv: -kv[1])
    print("cbhg-ratios %-28s %-22s worst %.3f (%s)" % (case.id, tag, worst[0][1], worst[0][0]))
    for k, r in worst:
        print("cbhg-ratios     %-28s %-22s %-48s %.3f" % (case.id, tag, k, r))


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_cbhg_training_block_against_float64_autograd(case):
    import taco_amd
    ref = R.reference(case)
    assert ref.admissible()
    params_before = None
    tr = taco_amd.Trainer(to_product_hp(ref.hp), ref.inp["w"])
    try:
        whole_chip = tr.decoder_engine_info()["compute_units"] >= 256
        word_a = case.paths if whole_chip else case.paths_partition
        params_before = tr.params.cpu().numpy().copy()
        # ---- (b) the trainer as created: six-product forward, split-bf16 data and weight gradients, planes for large problems ----
        dflt, w_dflt = _twice(tr, case, ref)
        assert w_dflt == word_a, "paths %#x, expected %#x" % (w_dflt, word_a)
        tr.set_wgrad_planes(2)                      # every eligible weight gradient from pre-split planes (k_wp_split / k_wp_gemm)
        planes, w_planes = _twice(tr, case, ref)
        word_p = (word_a & ~R.P_BANK_WG_EACH) | R.P_BANK_WG_PLANES if case.planes2 else word_a
        assert w_planes == word_p, "paths %#x, expected %#x" % (w_planes, word_p)
        assert tr.planes_problems() > 0
        tr.set_wgrad_planes(1)
        # ---- (a) exact engines against float64 ----
        tr.set_exact_gemm(1)
        tr.set_exact_wgrad(True)
        exact, w_exact = _twice(tr, case, ref)
        assert w_exact == word_a, "paths %#x, expected %#x" % (w_exact, word_a)
        _table("exact/f64 over bar", case, R.ratios(exact, ref.ref64, ref.bars))
        arms = [("exact", exact)]
        if case.name == "tiles":                    # the same sums leaving through atomics
            tr.set_deterministic(False)
            atomics, w_at = _twice(tr, case, ref, deterministic=False)
            assert w_at == word_a
            _table("exact,atomics/f64 over bar", case, R.ratios(atomics, ref.ref64, ref.bars))
            arms.append(("exact, atomics", atomics))
        for tag, got in arms:
            over = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN, case.margins)
            assert over == [], (tag, over[:6])
        # ---- (b) held against (a), per tensor, no global-norm floor ----
        unit = {k: DEFAULT_VS_EXACT * s for k, s in ref.scale.items()}
        for tag, got in (("default/exact over 1e-3 s", dflt), ("planes 2/exact over 1e-3 s", planes)):
            _table(tag, case, R.ratios(got, exact, unit))
            over = R.compare(got, exact, unit, 1.0)
            assert over == [], (tag, over[:6])
        # the moving statistics are frozen, and nothing else of the parameters is touched
        assert np.array_equal(tr.params.cpu().numpy(), params_before)
    finally:
        tr.close()
