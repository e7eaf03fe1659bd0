"""taco_forward_infer computes, bit for bit, what it computed at the commit before the chunked post-net overlap was retired -- the commit
that took the time-window mode out of k_gemm / k_gemm_bf3 (csrc/taco_kernels.h).  Until then every per-layer CBHG GEMM ran in that mode
with the window set to the whole row: nb * ceil(T / BM) tiles, each inside one batch row.  Now those launches are flat, ceil(B * T / BM)
tiles over the rows m = b * T + t, so a tile starts inside a batch row and crosses row borders; every output element keeps its K order.
Three models, ragged lengths, mel / linear / alignments of one eager forward per taco_debug_set_bf3 mode:
  tiny     widths outside the presets, so every CBHG layer is a launch of its own: B 5, T_in 11, T_mel 21 -- M = 105 (post-net) and 55
           (encoder), so every 32- and 64-row tile after the first starts inside a batch row, and the conv-bank taps, the max-pool window in
           proj_1's staging and the length-reversed xproj columns all cross a border inside a tile.  Modes 1 (k_gemm_bf3) and 0 (k_gemm).
  ref      the reference widths, B 8, T_in 24, T_mel 76 (no multiple of 64).  Mode 1: front + chain (these launches did not move); 29: front,
           entry and chain off, per-layer k_gemm_bf3; 65: six products; 0: exact k_gemm.
  wide     the reference widths with a 512-wide encoder CBHG behind 256-wide prenet and projections, B 8, T_in 32 (256 rows): the chain has no
           512-wide instantiation, so the per-layer path runs, and the CBHG's dense layer (256 -> 512) has the shape of a linear head.  It
           ran on k_gemm_bf3's tiles before, because a time-window call never took k_head_sweep, and stays there (GemmCall::tiles_only).
(The training step's X6 launches are held by test_gpu_scan_bitexact.py.)

tests/golden/forward_bitexact.json holds the sha256 of every complete array, recorded from a build of that earlier commit
(tools/make_forward_bitexact_golden.py); forward_bitexact.npz the first and last frames of the first and last row, which says WHERE two
builds differ when the digests do not agree.  Every comparison is for equality."""
import json
import os

import numpy as np
import pytest

from test_gpu_scan_bitexact import digest, sample

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, T_in, seed, {taco_debug_set_bf3 mode: words the feed-forward part of engine_plan must / must not hold})
CASES = {
    "tiny": (5, 11, 9100, {1: (["conv bank and proj_1 on k_gemm_bf3,", "point-wise layers on k_gemm_bf3 "], ["X6", "k_cbhg_front<", "k_pointwise_chain<"]),
                           0: (["conv bank and proj_1 on k_gemm,", "point-wise layers on k_gemm "], ["k_gemm_bf3", "k_cbhg_front<", "k_pointwise_chain<"])}),
    "ref": (8, 24, 9200, {1: (["k_cbhg_front<", "(the last projection in its entry)", "k_head_sweep<"], [" -- no "]),
                          29: (["conv bank and proj_1 on k_gemm_bf3,", "point-wise layers on k_gemm_bf3 "], ["X6", "k_cbhg_front<", "k_pointwise_chain<"]),
                          65: (["conv bank and proj_1 on k_gemm_bf3<..., X6>", "point-wise layers on k_gemm_bf3<..., X6>"], ["k_cbhg_front<", "k_pointwise_chain<"]),
                          0: (["exact-fp32 MFMA (k_gemm)", "conv bank and proj_1 on k_gemm,", "point-wise layers on k_gemm "], ["k_gemm_bf3", "k_cbhg_front<", "k_pointwise_chain<"])}),
    "wide": (8, 32, 9300, {1: (["6 point-wise layers on k_gemm_bf3 ", "no k_pointwise_chain: widths outside the presets"], ["X6"])}),
}
ARRAYS = ("mel", "linear", "alignments")


def _ohp(name):
    import taco_oracle as O
    from util import tiny_hp
    if name == "tiny":
        return tiny_hp(max_iters=7, reduction_factor=3)
    if name == "wide":
        return O.OracleHParams(max_iters=4, enc_prenet_sizes=[256, 256], enc_proj_sizes=[128, 256], enc_rnn_size=512)
    ohp = O.OracleHParams(max_iters=19)
    assert (ohp.max_iters * ohp.reduction_factor) % 64 != 0
    return ohp


def run_case(name):
    """{mode: (mel [B, T_mel, num_mels], linear [B, T_mel, num_freq], alignments [B, T_in, n])} of one model, float32 on the host"""
    import torch
    import taco_amd
    import taco_oracle as O
    from util import dev, ptr, stream, to_product_hp
    B, T_in, seed, modes = CASES[name]
    ohp = _ohp(name)
    hp = to_product_hp(ohp)
    n, T_mel = ohp.max_iters, ohp.max_iters * ohp.reduction_factor
    m = taco_amd.create_model(hp)
    m.load_weights(taco_amd.weights.random_weights(hp, 1, seed=seed))
    m.initialize(None, None, 1, None, device="cuda:0")
    ids, L = O.synthetic_inputs(B, T_in, seed + 1, ragged=True)
    idd, Ld = dev(ids), dev(L)
    nb = int(m._lib.taco_workspace_bytes(m._handle, B, T_in, n))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    got = {}
    for mode, (present, absent) in modes.items():
        taco_amd._lib.check(m._lib.taco_debug_set_bf3(m._handle, mode, 0))
        ff = m.engine_plan(B, T_in).split("; feed-forward: ")[1] + " "
        assert all(w in ff for w in present) and not any(w in ff for w in absent), (name, mode, ff)
        mel = torch.zeros((B, T_mel, ohp.num_mels), device="cuda")
        lin = torch.zeros((B, T_mel, ohp.num_freq), device="cuda")
        al = torch.zeros((B, T_in, n), device="cuda")
        stop = torch.zeros((1,), dtype=torch.int32, device="cuda")
        taco_amd._lib.check(m._lib.taco_forward_infer(m._handle, stream(), ptr(idd), ptr(Ld), ptr(None), B, T_in, n,
                                                      ptr(None), ptr(mel), ptr(lin), ptr(al), ptr(stop), ptr(ws), nb))
        torch.cuda.synchronize()
        m.check_device_errors()
        got[mode] = tuple(t.cpu().numpy() for t in (mel, lin, al))
        assert all(np.isfinite(a).all() for a in got[mode]), (name, mode)
    m.close()
    return got


def key(name, mode, array):
    return "%s/bf3_%d/%s" % (name, mode, array)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_is_bit_identical_to_the_build_before_the_gemm_window_mode_left(name):
    doc = json.load(open(os.path.join(GOLDEN, "forward_bitexact.json")))
    z = np.load(os.path.join(GOLDEN, "forward_bitexact.npz"))
    got = run_case(name)
    for mode in CASES[name][3]:
        for array, a in zip(ARRAYS, got[mode]):
            k = key(name, mode, array)
            assert list(a.shape) == doc[k + "_shape"], k
            s, g = sample(a).view(np.uint32), z[k].view(np.uint32)
            assert np.array_equal(s, g), "%s: %d of %d sampled words differ (first / last frames of the first / last row)" % (k, int((s != g).sum()), s.size)
            assert digest(a) == doc[k + "_sha256"], "%s differs outside the sampled frames" % k
