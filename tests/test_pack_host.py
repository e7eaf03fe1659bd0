"""CPU: the model build -- model_pack_host of csrc/taco_pack.h, everything taco_model_finalize does before it touches a device --
through taco_debug_pack_host.  For eight models (and a ninth, see CASES) it holds the arena, the GemmVar table and the split-bf16 index
lists to the digests in tests/golden/pack_digests.json, which tools/make_pack_digests.py recorded from the packing code as it stood
BEFORE it moved into taco_pack.h (the parent commit plus the hook alone, tools/pack_hook_only.patch): the packs may not change by a byte.

Weights are a closed formula, no RNG: element i of the tensor with ordinal t in the spec is a 32-bit integer hash of (t, i) mapped to
[-0.5, 0.5); moving_variance and gamma are shifted to [0.5, 1.5); attention_g is 1.25.

The expected masks (out[4]) are worked out by hand from the rules of the builders, never read from the library:
  dx     bits 0, 3-6: dx_widths_ok -- attention_state_size = dec_rnn_size = 2 enc_rnn_size = 256, attention_size 128 / 256 / 512, dec_prenet
         [256, 128] or [256, 128, 64], two decoder GRUs, num_mels * reduction_factor <= 512; a shadow model only at the reference widths
         (attention_size 256, prenet depth 2).  Query pack q (bit 3 + q) serves 2^q rows per group: Pc = min(32 / 2^q, 8) channel blocks of
         DS = attention_size / Pc columns, built where 8 <= DS <= 64: 128 -> DS 16, 16, 16, 32 (all four), 256 -> 32, 32, 32, 64 (all four),
         512 -> 64, 64, 64, 128 (the first three).
  bit 1  dx_p1o_raw: dx pack built, not a shadow model, reference widths.       bit 2  dx_spkw: dx pack built and model_type 'simple'.
  bit 7  dbx_pack: shadow model with a dx pack.
  8 / 9  gd and go packs: the CBHG's rnn size is 256.  Every case with a dx pack has enc_rnn_size 128, so bit 8 needs a case without one.
  10/11  gb and gob packs: the same on a shadow model.
  12/13  fused front: not a shadow model, max-pool 2, projection width 3, bank channels a multiple of 128, and (input padded to 16) either
         80 wide with K <= 8, proj_1 <= 256 and a multiple of 32 (post-net) or 128 wide with K <= 16, proj_1 <= 128 (encoder).
  bit 14 wtail: a dense layer on the split-bf16 path with N >= 512, 1 <= N % 32 <= 4, 256 or 512 inputs: the linear head at num_freq 513
         over a 256-wide post-net BiGRU (512 inputs; 'simple': after its speaker rows are split off).
  15/16  deepvoice with speaker_embedding_size 1 / larger.      17 / 18  attention bah_norm / bah_mon.
  bit 19 gru1_fold: every model that is not a shadow model.      bit 20  res_g2p: a CBHG whose rnn size is 256."""
import ctypes as C
import json
import os
import time

import numpy as np
import pytest

import taco_oracle as O
from taco_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pack_digests.json")


def bits(*b):
    return sum(1 << i for i in b)


def _ref(**kw):
    """Reference decoder / attention / post-net widths (the persistent packs need them); everything else cut: three and two bank widths,
    one highway layer, a 16-wide embedding, num_freq 513 (513 % 32 = 1: the head's vector tail).  The encoder CBHG keeps its 128-wide
    input and channels (the fused front's shape), the post-net its 256 channels."""
    base = dict(embedding_size=16, enc_prenet_sizes=[32, 128], enc_bank_size=3, post_bank_size=2, enc_highway_depth=1, post_highway_depth=1,
                num_mels=80, num_freq=513, reduction_factor=4, attention_type="bah_mon")
    base.update(kw)
    return O.OracleHParams(**base)


_DEEPVOICE = dict(model_type="deepvoice", attention_size=128, dec_prenet_sizes=[256, 128, 64], attention_type="bah_norm")
# 'luong_mon' is not an attention type of this library (taco_model_create refuses everything but bah / bah_norm / bah_mon); the monotonic
# type that has the score bias of bit 18 is bah_mon
_SIMPLE = dict(model_type="simple", attention_type="bah_mon")
_SMOKE = dict(num_mels=8, num_freq=36, enc_bank_size=5, post_bank_size=4, max_iters=6, reduction_factor=3)

# name -> (hparams, speakers, shadow, expected mask)
CASES = {
    # dx pack at the reference widths (0, 1, 3-6); enc_rnn_size 128: no bit 8; post-net 256 wide: 9, 13, 20; encoder input 128: 12;
    # num_freq 513: 14; bah_mon: 18; not a shadow: 19
    "1_single": (_ref(), 1, 0, bits(0, 1, 3, 4, 5, 6, 9, 12, 13, 14, 18, 19, 20)),
    # attention_size 128 and three prenet layers: a dx pack (PD = 3 registers) but not the reference widths (no bit 1); all four query packs
    "2_deepvoice": (_ref(speaker_embedding_size=16, **_DEEPVOICE), 3, 0, bits(0, 3, 4, 5, 6, 9, 12, 13, 14, 16, 17, 19, 20)),
    # the widths of this case are free: enc_rnn_size 256 -- no dx pack (2 * 256 != 256), but the only way to the encoder's gd / go packs
    # (bit 8); its CBHG then has a dense layer in front of the highway (128 -> 256) and both CBHGs carry res_g2p
    "3_deepvoice_table": (_ref(speaker_embedding_size=1, enc_rnn_size=256, **_DEEPVOICE), 3, 0, bits(8, 9, 12, 13, 14, 15, 17, 19, 20)),
    # attention_size 512: query packs 0-2 only; speaker rows (2); the head's 528 rows re-split into 16 + 512, so the tail is still built
    "4_simple": (_ref(speaker_embedding_size=16, attention_size=512, **_SIMPLE), 3, 0, bits(0, 2, 3, 4, 5, 9, 12, 13, 14, 18, 19, 20)),
    # everything / 8: no persistent pack, no front (16 / 32 channels), post-net proj_2 8 != rnn 32: has_dense; bah_mon by default: 18
    "5_smoke": (O.OracleHParams.scaled(8, **_SMOKE), 1, 0, bits(18, 19)),
    # shadow models: no dx_p1o_raw, no front, no gru1_fold; the dx pack in teacher form, dbx_pack, the post-net's gb / gob packs
    "6_shadow_single": (_ref(), 1, 1, bits(0, 3, 4, 5, 6, 7, 9, 11, 14, 18, 20)),
    "7_shadow_simple": (_ref(speaker_embedding_size=16, attention_size=256, **_SIMPLE), 3, 1, bits(0, 2, 3, 4, 5, 6, 7, 9, 11, 14, 18, 20)),
    "8_shadow_smoke": (O.OracleHParams.scaled(8, **_SMOKE), 1, 1, bits(18)),
    # a ninth case: bit 10 needs a shadow model whose ENCODER is 256 wide, which none of the shadows above can be (they follow cases 1, 4
    # and 5): the shadow of case 3.  Not at the reference widths: no dx / dbx pack.  The speaker tables (15) do not depend on the shadow.
    "9_shadow_deepvoice_table": (_ref(speaker_embedding_size=1, enc_rnn_size=256, **_DEEPVOICE), 3, 1, bits(8, 9, 10, 11, 14, 15, 17, 20)),
}


def spec_of(chp):
    """[(name, shape)] in spec order, from the library's own list (no device is touched)."""
    lib = _lib.load_library()
    h = C.c_void_p()
    _lib.check(lib.taco_model_create(C.byref(chp), 0, C.byref(h)))
    out = []
    try:
        buf, shape, nd = C.create_string_buffer(256), (C.c_int64 * 4)(), C.c_int()
        for i in range(lib.taco_model_num_weights(h)):
            _lib.check(lib.taco_model_weight_name(h, i, buf, 256, shape, C.byref(nd)))
            out.append((buf.value.decode(), tuple(shape[d] for d in range(nd.value))))
    finally:
        lib.taco_model_destroy(h)
    return out


def formula_weights(spec):
    """The flat weights: tensors in spec order, element i of tensor t = hash32(t, i) / 2^32 - 0.5, exact in float32 (24 bits kept)."""
    parts = []
    for t, (name, shape) in enumerate(spec):
        n = int(np.prod(shape, dtype=np.int64)) if shape else 1
        m32 = np.uint64(0xFFFFFFFF)
        h = (np.arange(n, dtype=np.uint64) * np.uint64(0x85EBCA6B) + np.uint64((t * 0x9E3779B1 + 0x165667B1) & 0xFFFFFFFF)) & m32
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x2C1B3C6D)) & m32
        h ^= h >> np.uint64(12)
        h = (h * np.uint64(0x297A2D39)) & m32
        h ^= h >> np.uint64(15)
        v = ((h >> np.uint64(8)).astype(np.float64) / float(1 << 24) - 0.5).astype(np.float32)
        leaf = name.rsplit("/", 1)[-1]
        if leaf in ("moving_variance", "gamma"):
            v += np.float32(1.0)
        if leaf == "attention_g":
            v[:] = 1.25
        parts.append(v)
    return np.ascontiguousarray(np.concatenate(parts))


def pack(name, n_floats=None):
    """(rc, {arena_floats, arena, vars, bf3, mask}, seconds) of one case."""
    ohp, speakers, shadow, _ = CASES[name]
    lib = _lib.load_library()
    chp = _lib.to_c_hparams(ohp, speakers)
    out = (C.c_uint64 * 5)()
    if shadow:
        w, ptr, n = None, C.c_void_p(0), 0
    else:
        w = formula_weights(spec_of(chp))
        ptr, n = C.c_void_p(w.ctypes.data), w.size if n_floats is None else n_floats
    t0 = time.perf_counter()
    rc = lib.taco_debug_pack_host(C.byref(chp), shadow, ptr, n, out)
    dt = time.perf_counter() - t0
    return rc, {"arena_floats": int(out[0]), "arena": "%016x" % out[1], "vars": "%016x" % out[2], "bf3": "%016x" % out[3], "mask": int(out[4])}, dt


@pytest.mark.parametrize("name", sorted(CASES))
def test_packs_match_the_parent_commit(name):
    rc, got, dt = pack(name)
    assert rc == 0, _lib.load_library().taco_last_error()
    print("%s: %.2f s, %d floats, mask %#x" % (name, dt, got["arena_floats"], got["mask"]))
    want_mask = CASES[name][3]
    assert got["mask"] == want_mask, "mask %#x, by the rules %#x" % (got["mask"], want_mask)
    want = json.load(open(GOLDEN))[name]
    assert {k: got[k] for k in ("arena_floats", "arena", "vars", "bf3")} == want
    assert (got["bf3"] != "%016x" % 0) == bool(CASES[name][2])          # index lists: on a shadow model, and only there


def test_the_cases_reach_every_pack():
    union = 0
    for _, _, _, mask in CASES.values():
        union |= mask
    assert union == (1 << 21) - 1


def test_bad_arguments_are_refused():
    rc, _, _ = pack("5_smoke", n_floats=17)
    assert rc == _lib.TACO_ERR_SHAPE
    ohp, speakers, _, _ = CASES["5_smoke"]
    chp = _lib.to_c_hparams(ohp, speakers)
    w = np.zeros(4, np.float32)
    out = (C.c_uint64 * 5)()
    lib = _lib.load_library()
    assert lib.taco_debug_pack_host(C.byref(chp), 1, C.c_void_p(w.ctypes.data), 4, out) == _lib.TACO_ERR_ARG     # a shadow model takes no weights
    assert lib.taco_debug_pack_host(C.byref(chp), 0, C.c_void_p(0), 0, out) == _lib.TACO_ERR_ARG
