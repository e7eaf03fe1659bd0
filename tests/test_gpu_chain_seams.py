"""The point-wise chain (csrc/taco_chain.h) computes, bit for bit, what it computed before its seams were rebuilt: two plane sets and one
barrier per layer, the next product's first weight fragments and biases requested ahead of the seam, the entry's operands requested ahead
of the partial sums, the last link's passes from the upper column groups down and its reversed stores in a loop per branch.  None of that
may move a bit: every FMA chain, every summation order and the K rotation (CH_ROT) are what they were.

One eager taco_forward_infer per case at the reference widths, ragged lengths, mel / linear / alignments compared for equality with
digests recorded ONCE from a build of the commit before the change (tools/make_chain_seams_golden.py -> tests/golden/chain_seams.json, .npz:
sha256 of the complete arrays; first and last frames of the first and last row, which says where two builds differ):
  t68      B 3, T_in 70, n 17 (T_mel 68): T >= 64 with a partial last tile, and the time-reversed columns of the last link cross a
           batch-row border inside a tile (encoder 210 rows, post-net 204).
  t20      B 5, T_in 20, n 5 (T_mel 20): T < 64, a tile spans up to four batch rows -- the other branch of the reversed store.
  t140     B 8, T_in 24, n 35 (T_mel 140, 18 post-net tiles): workgroup ids >= 16, so the K rotation takes 0, 1 and 2.
  dv       a deepvoice model, three speakers: the entry adds the per-row vector to the residual.
  noentry  t68's shapes with taco_debug_set_bf3 bit 4: no fused entry, the chain stages its input rows in front of the doubled planes.
t140 runs a second time over poisoned device memory (NaN in whatever the allocator hands out next, as conftest.py's TACO_POISON=nan does
for a whole session): plane set B and the entry's planes laid over it are LDS the kernel did not use before.
Biases and BatchNorm statistics are drawn at random too (weights.random_weights leaves most of them 0 / 1, which would hide a bias taken
from the wrong layer)."""
import json
import os

import numpy as np
import pytest

from test_gpu_scan_bitexact import digest, sample

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, T_in, n_steps, model_type, speakers, taco_debug_set_bf3 mode, seed, words the feed-forward part of engine_plan must / must not hold)
NOT_OFF = ["no k_pointwise_chain", "no k_cbhg_front", "no fused chain entry"]      # (the linear head below 256 rows is a k_gemm_bf3 launch: not this test's matter)
CASES = {
    "t68": (3, 70, 17, "single", 1, 1, 9400, (["k_pointwise_chain<128> (the last projection in its entry)", "k_pointwise_chain<256> (the last projection in its entry)"], NOT_OFF)),
    "t20": (5, 20, 5, "single", 1, 1, 9410, (["(the last projection in its entry)"], NOT_OFF)),
    "t140": (8, 24, 35, "single", 1, 1, 9420, (["(the last projection in its entry)"], NOT_OFF)),
    "dv": (4, 33, 9, "deepvoice", 3, 1, 9430, (["(the last projection in its entry)"], NOT_OFF)),
    "noentry": (3, 70, 17, "single", 1, 17, 9440, (["no fused chain entry: taco_debug_set_bf3 bit 4", "k_pointwise_chain<256>"], ["in its entry"])),
}
ARRAYS = ("mel", "linear", "alignments")


def _weights(hp, ns, seed):
    """random_weights, with every bias and BatchNorm statistic moved off its initial 0 / 1 (uniform draws only: no libm in the recipe)"""
    import taco_amd
    w = taco_amd.weights.random_weights(hp, ns, seed=seed)
    rs = np.random.RandomState(seed + 5)
    for name in sorted(w):
        leaf = name.rsplit("/", 1)[-1]
        if leaf in ("bias", "beta", "moving_mean"):
            w[name] = (w[name] + rs.uniform(-0.2, 0.2, w[name].shape)).astype(np.float32)
        elif leaf in ("gamma", "moving_variance"):
            w[name] = (w[name] + rs.uniform(0.0, 0.5, w[name].shape)).astype(np.float32)
    return w


def poison_device_memory(gb=2):
    """what conftest.py's TACO_POISON=nan does before a test: NaN into memory that goes back to the caching allocator"""
    import torch
    torch.cuda.empty_cache()
    x = torch.empty(gb << 30, dtype=torch.uint8, device="cuda").view(torch.float32)
    x.fill_(float("nan"))
    torch.cuda.synchronize()
    del x


def run_case(name, poison=False):
    """(mel [B, T_mel, num_mels], linear [B, T_mel, num_freq], alignments [B, T_in, n]) of one eager forward, float32 on the host"""
    import torch
    import taco_amd
    import taco_oracle as O
    from util import dev, ptr, stream, to_product_hp
    B, T_in, n, model_type, ns, mode, seed, (present, absent) = CASES[name]
    ohp = O.OracleHParams(max_iters=n, model_type=model_type)
    hp = to_product_hp(ohp)
    T_mel = n * ohp.reduction_factor
    m = taco_amd.create_model(hp)
    m.load_weights(_weights(hp, ns, seed))
    m.initialize(None, None, ns, None, device="cuda:0")
    ids, L = O.synthetic_inputs(B, T_in, seed + 1, ragged=True)
    idd, Ld = dev(ids), dev(L)
    spk = dev((np.arange(B) % ns).astype(np.int32)) if ns > 1 else None
    taco_amd._lib.check(m._lib.taco_debug_set_bf3(m._handle, mode, 0))
    ff = m.engine_plan(B, T_in).split("; feed-forward: ")[1] + " "
    assert all(w in ff for w in present) and not any(w in ff for w in absent), (name, ff)
    if poison:
        poison_device_memory()
    nb = int(m._lib.taco_workspace_bytes(m._handle, B, T_in, n))
    ws = torch.empty((nb,), dtype=torch.uint8, device="cuda")
    mel = torch.zeros((B, T_mel, ohp.num_mels), device="cuda")
    lin = torch.zeros((B, T_mel, ohp.num_freq), device="cuda")
    al = torch.zeros((B, T_in, n), device="cuda")
    stop = torch.zeros((1,), dtype=torch.int32, device="cuda")
    taco_amd._lib.check(m._lib.taco_forward_infer(m._handle, stream(), ptr(idd), ptr(Ld), ptr(spk), B, T_in, n,
                                                  ptr(None), ptr(mel), ptr(lin), ptr(al), ptr(stop), ptr(ws), nb))
    torch.cuda.synchronize()
    m.check_device_errors()
    got = tuple(t.cpu().numpy() for t in (mel, lin, al))
    m.close()
    assert all(np.isfinite(a).all() for a in got), name
    return got


def key(name, array):
    return "%s/%s" % (name, array)


def _compare(name, got):
    doc = json.load(open(os.path.join(GOLDEN, "chain_seams.json")))
    z = np.load(os.path.join(GOLDEN, "chain_seams.npz"))
    for array, a in zip(ARRAYS, got):
        k = key(name, array)
        assert list(a.shape) == doc[k + "_shape"], k
        s, g = sample(a).view(np.uint32), z[k].view(np.uint32)
        assert np.array_equal(s, g), "%s: %d of %d sampled words differ (first / last frames of the first / last row)" % (k, int((s != g).sum()), s.size)
        assert digest(a) == doc[k + "_sha256"], "%s differs outside the sampled frames" % k


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_forward_is_bit_identical_to_the_build_before_the_seams_changed(name):
    _compare(name, run_case(name))


@pytest.mark.gpu
def test_eighteen_tiles_over_poisoned_device_memory():
    _compare("t140", run_case("t140", poison=True))
