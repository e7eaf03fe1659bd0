"""Second-pass manual alignments built on the device (k_manual_alignments / taco_manual_alignments; synthesizer.py:171-205, modes 1 and 3).
Every comparison is on the bits: the kernel copies and selects, it does no arithmetic.  References: the reference's own run
(tests/golden/manual_vectors.npz), the host restatement taco_amd.synthesizer.manual_alignments_of, and NumPy's argmax."""
import os

import numpy as np
import pytest

import taco_oracle as O
from util import tiny_hp, to_product_hp, dev, ptr, stream

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ONE = np.float32(1.0).view(np.uint32)


def same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def numpy_ref(a, mode):
    """[B, E, D] -> [B, D, E] with np.argmax over decoder steps (first maximum, NaN as the maximum, +0 == -0), on the bits."""
    a = np.ascontiguousarray(a, np.float32)
    out = np.zeros((a.shape[0], a.shape[2], a.shape[1]), np.uint32) if mode == 1 else np.transpose(a.view(np.uint32), [0, 2, 1]).copy()
    for b in range(a.shape[0]):
        out[b][(a[b].argmax(1), np.arange(a.shape[1]))] = ONE
    return out.view(np.float32)


def device_call(a, mode, fill=np.nan):
    """The C entry point on a [B, E, D] host array; the output buffer holds `fill` before the call."""
    import torch
    from taco_amd import _lib
    lib = _lib.load_library()
    a = np.ascontiguousarray(a, np.float32)
    B, E, D = a.shape
    ad = dev(a)
    out = torch.full((B, D, E), fill, dtype=torch.float32, device="cuda")
    rc = lib.taco_manual_alignments(stream(), ptr(ad), B, E, D, mode, ptr(out))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def check(a, label=""):
    from taco_amd.synthesizer import manual_alignments_of
    a = np.ascontiguousarray(a, np.float32)
    for mode in (1, 3):
        rc, got = device_call(a, mode)
        assert rc == 0 and same_bits(got, numpy_ref(a, mode)), (label, mode, a.shape)
        assert same_bits(got, manual_alignments_of(a, mode)), (label, mode, a.shape)
        if mode == 1:                                # every element written, none left over from the NaN the buffer held
            assert not np.isnan(got).any() and set(np.unique(got.view(np.uint32))) <= {0, int(ONE)}
            assert np.all(got.sum(1) == 1)           # one decoder step per encoder position


def test_the_reference_runs_first_passes():
    """The 24 first passes the reference's own synthesize(manual_attention_mode=1|3) produced, [1,11,2] .. [3,13,16]: the kernel's output
    equals what the reference fed to its second pass, and the host restatement."""
    from taco_amd.synthesizer import manual_alignments_of
    mv = np.load(os.path.join(GOLD, "manual_vectors.npz"))
    assert len(mv["first_pass"]) == 24
    tied = 0
    for fp, m1, m3, (N, E, D) in zip(mv["first_pass"], mv["mode1"], mv["mode3"], mv["dims"]):
        al = np.ascontiguousarray(fp[:N, :E, :D])
        tied += int(((al == al.max(2, keepdims=True)).sum(2) > 1).sum())
        for mode, gold in ((1, m1), (3, m3)):
            rc, got = device_call(al, mode)
            assert rc == 0 and got.shape == (N, D, E)
            assert same_bits(got, gold[:N, :D, :E]) and same_bits(got, manual_alignments_of(al, mode)), (N, E, D, mode)
    assert tied == 0                                 # the reference's runs hold no tied maximum: the ties below are hand-written


def test_hand_written_ties():
    rs = np.random.RandomState(5)
    a = (rs.randint(0, 4, size=(3, 37, 150)) / 4).astype(np.float32)                # most rows tie
    assert ((a == a.max(2, keepdims=True)).sum(2) > 1).mean() > 0.9
    check(a, "quarters")
    a = rs.rand(2, 6, 200).astype(np.float32) * 0.5
    a[0, 0, :] = 0.25                                                                # a constant row: step 0
    a[0, 1, :] = 0.0
    a[0, 2, -1] = 0.75                                                               # the maximum only at the last step
    a[0, 3, 70] = a[0, 3, 6] = 0.75                                                  # 64 apart: the same lane of a strided wave
    a[0, 4, 72] = a[0, 4, 7] = 0.75                                                  # 65 apart: neighbouring lanes
    a[0, 5, 199] = a[0, 5, 135] = a[0, 5, 134] = 0.75
    a[1, 0, :] = -0.0
    a[1, 0, 5] = 0.0                                                                 # +0 against -0: equal, step 0 wins
    a[1, 1, :] = -1.0
    a[1, 1, 3] = -0.0
    a[1, 1, 130] = 0.0                                                               # -0 first, +0 later: still the first
    a[1, 2, 140] = np.nan
    a[1, 2, 9] = np.nan                                                              # two NaNs: the first NaN wins over every number
    a[1, 2, 3] = 0.9
    a[1, 3, :] = -np.inf                                                             # all -inf: step 0, not an unwritten index
    a[1, 4, 1] = np.inf
    a[1, 4, 65] = np.inf
    assert numpy_ref(a, 1)[0, :, 3].argmax() == 6 and numpy_ref(a, 1)[0, :, 4].argmax() == 7 and numpy_ref(a, 1)[1, :, 2].argmax() == 9
    assert numpy_ref(a, 1)[1, :, 0].argmax() == 0 and numpy_ref(a, 1)[1, :, 1].argmax() == 3 and numpy_ref(a, 1)[0, :, 2].argmax() == 199
    check(a, "hand")
    rc, got = device_call(a, 3)
    assert np.isnan(got[1, 140, 2]) and got[1, 9, 2] == 1.0                          # mode 3 keeps the later NaN's bits
    assert got.view(np.uint32)[1, 1, 0] == np.float32(-0.0).view(np.uint32)          # ... and the sign of a zero


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 5, 7), (2, 65, 129), (1, 130, 1), (2, 3, 4099), (1, 2048, 5), (33, 128, 128)],
                         ids=lambda s: "x".join(map(str, s)))
def test_shapes_across_every_boundary_of_the_kernel(shape):
    """One element; below one tile both ways; one past a tile of positions and two tiles of steps; several tiles of positions with a single
    step; a row longer than 64 strided passes of a wave; the widest T_in the forward takes; more workgroups than one batch row's tiles."""
    B, E, D = shape
    rs = np.random.RandomState(E * 131 + D)
    a = rs.rand(B, E, D).astype(np.float32)
    check(a, "random")
    check(np.floor(a * 3) / 3, "tied")


def test_capture_and_replay():
    """The call is captured into one graph on a side stream and replayed on two inputs: each replay equals the eager result."""
    import torch
    from taco_amd import _lib
    lib = _lib.load_library()
    B, E, D = 2, 70, 131
    rs = np.random.RandomState(9)
    x = [np.floor(rs.rand(B, E, D) * 5).astype(np.float32) / 5 for _ in range(2)]
    for mode in (1, 3):
        eager = [device_call(v, mode)[1] for v in x]
        assert not same_bits(eager[0], eager[1])
        src = torch.zeros((B, E, D), dtype=torch.float32, device="cuda")
        out = torch.full((B, D, E), float("nan"), dtype=torch.float32, device="cuda")
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):       # the side stream is the current stream inside
            rc = lib.taco_manual_alignments(stream(), ptr(src), B, E, D, mode, ptr(out))
        assert rc == 0
        torch.cuda.synchronize()
        assert np.isnan(out.cpu().numpy()).all()     # captured, not run
        for v, want in zip(x, eager):
            src.copy_(dev(v))
            out.fill_(float("nan"))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert same_bits(out.cpu().numpy(), want), mode
        del g


def test_the_model_call_takes_the_current_stream_eagerly_and_in_a_capture(tmp_path):
    """Tacotron.manual_alignments_from goes through the package's device-call layer: on a side stream it runs there, and inside a graph
    capture it takes the capturing stream -- a call that took another stream could not be captured (the runtime refuses, the layer
    raises).  The replay writes the same bits as the eager call."""
    import torch
    s = _synth(tmp_path)
    a = np.array([[[0.25, 0.5], [0.75, 0.125], [0.5, 0.5]]], np.float32)              # [B = 1, T_in = 3, n_steps = 2], one tie
    src = dev(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = s.model.manual_alignments_from(src, 1).clone()
    side.synchronize()
    assert same_bits(eager.cpu().numpy(), numpy_ref(a, 1))
    out = torch.full((1, 2, 3), float("nan"), dtype=torch.float32, device="cuda")
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        assert s.model.manual_alignments_from(src, 1, out=out) is out
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()         # captured, not run
    g.replay()
    torch.cuda.synchronize()
    assert same_bits(out.cpu().numpy(), eager.cpu().numpy())
    del g
    s.close()


def test_refused_modes_leave_the_output_untouched():
    from taco_amd import _lib
    lib = _lib.load_library()
    a = np.random.RandomState(2).rand(2, 5, 9).astype(np.float32)
    for mode, code in ((2, _lib.TACO_ERR_UNSUPPORTED), (0, _lib.TACO_ERR_ARG)):
        rc, got = device_call(a, mode, fill=7.0)
        assert rc == code and lib.taco_last_error() and np.all(got == 7.0), mode


# ---- end to end: Tacotron.run / Synthesizer.synthesize / synthesize_audio ----
def _synth(tmp_path, model_type="single", ns=1, seed=31):
    """The tiny model of test_gpu_e2e.py::test_synthesizer_surface with the audio keys of test_gpu_audio_rows.py's surface test."""
    import taco_amd
    ohp = tiny_hp(num_freq=65, max_iters=20, model_type=model_type)
    hp = to_product_hp(ohp)
    hp.add_hparam("sample_rate", 1600)
    hp.add_hparam("griffin_lim_iters", 3)
    taco_amd.save_hparams(str(tmp_path), hp)
    taco_amd.weights.save_weights(str(tmp_path / "model.ckpt-100.safetensors"), O.init_weights(ohp, ns, seed))
    return taco_amd.Synthesizer().load(str(tmp_path), num_speakers=ns)


@pytest.mark.parametrize("model_type,ns,speaker_ids", [("single", 1, None), ("deepvoice", 2, {0: 0.25, 1: 0.75})], ids=["single", "deepvoice-mix"])
def test_two_pass_synthesis_equals_the_host_built_route(tmp_path, model_type, ns, speaker_ids):
    """synthesize / synthesize_audio with manual_attention_mode against the route through the host: first pass, manual_alignments_of, a
    forward with manual_alignments.  With a dict of speaker ids the mix plan takes the path."""
    import taco_amd
    from taco_amd import _lib
    from taco_amd.synthesizer import manual_alignments_of
    s = _synth(tmp_path, model_type, ns)
    ids, L = O.synthetic_inputs(2, 9, 41)
    feed = s._speaker_feed(speaker_ids, len(ids))
    run = lambda **kw: s.model.run(inputs=ids.astype(np.int32), input_lengths=L, **feed, **kw)
    lin0, al0 = [t.cpu().numpy() for t in run()]
    assert al0.shape == (2, 9, 20)                   # the stop rule did not cut the first pass
    for mode in (1, 3):
        host = manual_alignments_of(al0, mode)
        want_lin, want_al = [t.cpu().numpy() for t in run(manual_alignments=host, is_manual_attention=True)]
        # the device-built alignments themselves, into a buffer of the caller's and into a fresh one
        built = s.model.manual_alignments_from(dev(al0), mode)
        assert same_bits(built.cpu().numpy(), host)
        into = built.new_full(built.shape, float("nan"))
        assert s.model.manual_alignments_from(dev(al0), mode, out=into) is into and same_bits(into.cpu().numpy(), host)
        lin, al = s.synthesize(tokens=ids, speaker_ids=speaker_ids, manual_attention_mode=mode)
        assert same_bits(lin, want_lin) and same_bits(al, want_al), mode
        assert same_bits(s.model.first_pass_alignments.cpu().numpy(), al0)              # the reference saves both passes
        assert not same_bits(lin, lin0)
        lin_r, al_r = run(manual_attention_mode=mode)
        assert same_bits(lin_r.cpu().numpy(), want_lin) and same_bits(al_r.cpu().numpy(), want_al)
    host = manual_alignments_of(al0, 1)
    a = s.synthesize_audio(tokens=ids, speaker_ids=speaker_ids, manual_attention_mode=1, seed=3)
    end_a, lin_a = np.array(s.spec_end_idx), s.model.linear_outputs.cpu().numpy()
    b = s.synthesize_audio(tokens=ids, speaker_ids=speaker_ids, manual_alignments=host, seed=3)
    end_b, lin_b = np.array(s.spec_end_idx), s.model.linear_outputs.cpu().numpy()
    assert len(a) == len(b) == 2 and all(x.dtype == np.int16 and np.array_equal(x, y) for x, y in zip(a, b))
    assert np.array_equal(end_a, end_b) and same_bits(lin_a, lin_b)
    plain = s.synthesize_audio(tokens=ids, speaker_ids=speaker_ids, seed=3)
    assert s.model.first_pass_alignments is None     # a one-pass call leaves no first pass behind
    assert not all(len(x) == len(y) and np.array_equal(x, y) for x, y in zip(a, plain))
    with pytest.raises(_lib.TacoError) as e:
        s.synthesize_audio(tokens=ids, speaker_ids=speaker_ids, manual_attention_mode=1, manual_alignments=host)
    assert e.value.code == _lib.TACO_ERR_ARG
    for call in (s.synthesize, s.synthesize_audio):
        with pytest.raises(Exception) as e:
            call(tokens=ids, speaker_ids=speaker_ids, manual_attention_mode=2)
        assert "np.pow" in str(e.value) and not isinstance(e.value, _lib.TacoError)
    s.close()
