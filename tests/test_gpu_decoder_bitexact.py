"""The persistent decoder (csrc/taco_decoder_xcd.h) computes, bit for bit, what it computed before its step loop was put on an instruction
diet (round 7: hoisted addresses, shorter poll path, stores behind the publish -- no arithmetic touched).  The decoder stage alone, fixed
weights and a fixed encoder output, against arrays recorded from the kernel of the commit before the diet (tools/make_decoder_bitexact_golden.py):
C2, a five-row batch that leaves three of the eight groups empty (one row per group), and a 64-row pass at eight rows per group.
tests/golden/decoder_bitexact.json holds the sha256 of the complete mel and alignment arrays of every case; decoder_bitexact_<case>.npz a
fixed sample of their steps, which says WHERE two builds differ when the digests do not agree."""
import hashlib
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# name -> (B, T_in, reduction factor, decoder steps, rows per group expected)
CASES = {"C2": (32, 128, 4, 128, 4), "ragged5": (5, 37, 4, 24, 1), "rg8_64rows": (64, 128, 4, 32, 8)}
SAMPLED_STEPS = 4


def run_case(name):
    """mel [B, n*r, M], alignments [B, T_in, n], stop step of the decoder stage on the persistent engine; float32 arrays on the host"""
    import torch
    import taco_amd
    B, T_in, r, n, rg = CASES[name]
    hp = taco_amd.hparams.copy(max_iters=n, reduction_factor=r, model_type="single")
    m = taco_amd.create_model(hp)
    m.load_weights(taco_amd.weights.random_weights(hp, 1, seed=1234))
    m.initialize(None, None, 1, None, device="cuda:0")
    # a stand-in for the encoder's output (bidirectional GRU states: inside (-1, 1)); uniform draws only, no libm in the recipe
    enc = np.random.RandomState(7000 + B).uniform(-1.0, 1.0, size=(B, T_in, 2 * hp.enc_rnn_size)).astype(np.float32)
    m.set_decoder_engine(1, 0)
    assert "k_decoder_xcd<%d" % rg in m.engine_plan(B, T_in, n * r), m.engine_plan(B, T_in, n * r)
    mel, al, stop, _ = m.decoder(enc, n)
    torch.cuda.synchronize()
    info = m.decoder_engine_info()
    m.check_device_errors()
    assert info["has_pack"] and info["protocol"] in (1, 2), info
    out = mel.cpu().numpy(), al.cpu().numpy(), int(stop.item())
    m.close()
    return out


def sampled_steps(name):
    n = CASES[name][3]
    return np.sort(np.random.RandomState(len(name)).choice(n, SAMPLED_STEPS, replace=False))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def sample(name, mel, al):
    r, steps = CASES[name][2], sampled_steps(name)
    frames = (steps[:, None] * r + np.arange(r)[None, :]).reshape(-1)
    return steps, mel[:, frames], al[:, :, steps]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_decoder_stage_is_bit_identical_to_the_kernel_before_the_diet(name):
    mel, al, stop = run_case(name)
    gold = json.load(open(os.path.join(GOLDEN, "decoder_bitexact.json")))[name]
    z = np.load(os.path.join(GOLDEN, "decoder_bitexact_%s.npz" % name))
    steps, mel_s, al_s = sample(name, mel, al)
    assert np.array_equal(steps, z["steps"])
    assert list(mel.shape) == gold["mel_shape"] and list(al.shape) == gold["alignments_shape"]
    # the sample first: a failure names the first step that differs
    for k, t in enumerate(steps):
        r = CASES[name][2]
        a, b = mel_s[:, k * r:(k + 1) * r].view(np.uint32), z["mel"][:, k * r:(k + 1) * r].view(np.uint32)
        assert np.array_equal(a, b), "mel of step %d differs in %d of %d words" % (t, int((a != b).sum()), a.size)
        a, b = al_s[:, :, k].view(np.uint32), z["alignments"][:, :, k].view(np.uint32)
        assert np.array_equal(a, b), "alignments of step %d differ in %d of %d words" % (t, int((a != b).sum()), a.size)
    assert stop == gold["stop_step"]
    assert digest(mel) == gold["mel_sha256"], "mel differs outside the sampled steps"
    assert digest(al) == gold["alignments_sha256"], "alignments differ outside the sampled steps"
