"""Resampling to the model's sample rate on the device (taco_wav_resample, audio.Resampler, split_on_silence(orig_sr=)) against the
float64 restatement tests/resample_reference.py with exact positions.  UNPINNED on resampy and librosa (see the restatement's header):
what is held here is the kernel against that restatement.

Values are held to a DERIVED bound, per output: |y_gpu - y_ref| <= (taps + channels + 3) * 2^-24 * A_t + FLOOR, A_t = sum |w_j| |x_j|
from the restatement on the fp32-rounded inputs -- the forward-error bound of an fp32 dot product of `taps` terms in any summation
order ((taps + 2) roundings of products and sums to first order), one rounding for each weight (the fp32 bank), one for the channel
mean, and one to spare for the second-order terms.  FLOOR = 4 * 2^-149, four fp32 denormals: a sum whose terms underflow is not
covered by a relative bound.  Lengths, the zeros past computed_len and out_samples are compared for EQUALITY.  The largest observed
ratio to the bound is printed per case (-s).  Measured on an MI355X: at most 0.29 (the 7-tap filter at 2 -> 3), 0.061 at 44100 -> 24000
and 0.084 at 16000 -> 24000 with kaiser_best (profiles/r09_resample_tests.txt)."""
import functools

import numpy as np
import pytest

import resample_reference as R

pytestmark = pytest.mark.gpu

FLOOR = 4 * 2.0 ** -149
L = 2500
CASES = [("small", 3, 2), ("small", 2, 3), ("small", 80, 147), ("small", 147, 80), ("kaiser_best", 44100, 24000), ("kaiser_best", 16000, 24000)]
FILTER = {"small": R.SMALL, "kaiser_best": R.KAISER_BEST}


@functools.lru_cache(maxsize=None)
def _half(name):
    half, nt = R.sinc_window(**FILTER[name])
    half.setflags(write=False)
    return half, nt


@functools.lru_cache(maxsize=None)
def _case(name, so, sn):
    """The rectangle, its row lengths and the restatement of every row (float32 inputs; 16-bit PCM; two-channel PCM), computed once."""
    half, nt = _half(name)
    bank, LW = R.bank(so, sn, half, nt)
    Q = R.setup(so, sn, half, nt)["Q"]
    lengths = [L, L - 1, max(1, 1900 // Q) * Q, LW - 1, 1, 0]      # full, odd, a multiple of Q, one fewer than the left half of the filter, 1, 0
    x = R.chirp_rows(L, lengths, 7).astype(np.float32)
    rs = np.random.RandomState(11)
    q = np.round(x * 8000).astype(np.int16)                        # the same samples quantised (|x| < 4: no clipping)
    q2 = np.stack([q, np.round(8000 * 0.5 * rs.randn(len(lengths), L)).astype(np.int16)], axis=2)      # [B, L, 2]: two different channels
    for b, n in enumerate(lengths):
        q2[b, n:] = 0
    ref = lambda rows: [R.resample_bank(rows[b, :n], so, sn, half, nt, weights=(bank, LW)) for b, n in enumerate(lengths)]
    out = dict(x=x, q=q, q2=q2, lengths=lengths, taps=bank.shape[1], f32=ref(x.astype(np.float64)), pcm=ref(q.astype(np.float64) / 32768.0),
               stereo=ref(q2.astype(np.float64).mean(axis=2) / 32768.0))
    return out


@functools.lru_cache(maxsize=None)
def _resampler(name, so, sn):
    import taco_amd
    half, nt = _half(name)
    return taco_amd.Resampler(so, sn, filter=np.array(half), num_table=nt)


def _check(tag, rs, out, out_samples, refs, lengths, taps, channels, so, sn):
    out, out_samples = out.cpu().numpy(), out_samples.cpu().numpy()
    assert out.shape == (len(lengths), R.out_len(L, so, sn)) and out.dtype == np.float32
    worst = 0.0
    for b, n in enumerate(lengths):
        y, A = refs[b]
        c = R.computed_len(n, so, sn)
        assert len(y) == c == rs.computed_len(n) and out_samples[b] == R.out_len(n, so, sn) == rs.out_len(n)
        assert not out[b, c:].any() and not np.signbit(out[b, c:]).any()                                # exact zeros past computed_len
        if c:
            bound = (taps + channels + 3) * 2.0 ** -24 * A + FLOOR
            ratio = np.abs(out[b, :c].astype(np.float64) - y) / bound
            worst = max(worst, float(ratio.max()))
    print("%s %d -> %d (%d taps, %d channel(s)): largest |y_gpu - y_ref| over its bound %.4f" % (tag, so, sn, taps, channels, worst))
    assert worst <= 1.0


@pytest.mark.parametrize("name,so,sn", CASES)
def test_rows_of_a_rectangle_against_the_restatement(name, so, sn):
    import torch
    c, rs = _case(name, so, sn), _resampler(name, so, sn)
    assert rs.taps == c["taps"] and rs.phases == R.setup(so, sn, *_half(name))["P"]
    ns = np.array(c["lengths"], np.int32)
    args = (c["lengths"], c["taps"])
    out, on = rs.resample(c["x"], ns)
    _check("float32", rs, out, on, c["f32"], *args, 1, so, sn)
    _check("pcm16", rs, *rs.resample(c["q"], ns), c["pcm"], *args, 1, so, sn)
    _check("pcm16 stereo", rs, *rs.resample(c["q2"], ns, channels=2), c["stereo"], *args, 2, so, sn)
    twice = np.repeat(c["x"][:, :, None], 2, axis=2)                                                   # float32 stereo, identical channels
    o2, n2 = rs.resample(twice, ns, channels=2)
    assert torch.equal(o2.view(torch.int32), out.view(torch.int32)) and torch.equal(n2, on)           # the mono result on the bits


@pytest.mark.parametrize("name,so,sn", [CASES[0], CASES[4]])
def test_null_num_samples_is_a_vector_of_L(name, so, sn):
    import torch
    c, rs = _case(name, so, sn), _resampler(name, so, sn)
    a, an = rs.resample(c["x"], None)
    b, bn = rs.resample(c["x"], np.full(len(c["lengths"]), L, np.int32))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(an, bn) and an.tolist() == [rs.out_len(L)] * len(c["lengths"])


@pytest.mark.parametrize("name,so,sn", [CASES[1], CASES[4]])
def test_tiles_inside_a_row_equal_the_row_alone(name, so, sn):
    """Rows long enough for three tiles of outputs each (the tile comes from the handle), in a rectangle of three and alone."""
    import torch
    rs = _resampler(name, so, sn)
    n_in = int(np.ceil((2 * rs.tile + 77) * so / sn))
    assert rs.computed_len(n_in) > 2 * rs.tile
    lengths = [n_in, n_in - rs.tile // 3, n_in // 2]
    x = torch.from_numpy(R.chirp_rows(n_in, lengths, 3).astype(np.float32)).cuda()
    ns = torch.tensor(lengths, dtype=torch.int32, device="cuda")
    out, on = rs.resample(x, ns)
    for b in range(3):
        o1, n1 = rs.resample(x[b:b + 1].contiguous(), ns[b:b + 1].contiguous())
        assert torch.equal(o1.view(torch.int32), out[b:b + 1].view(torch.int32)) and torch.equal(n1, on[b:b + 1])
    # and the first row against the restatement, so that "equal" is not "equally wrong" past the first tile
    half, nt = _half(name)
    y, A = R.resample_bank(x[0].cpu().numpy().astype(np.float64), so, sn, half, nt)
    ratio = np.abs(out[0, :len(y)].cpu().numpy().astype(np.float64) - y) / ((rs.taps + 4) * 2.0 ** -24 * A + FLOOR)
    print("three tiles %d -> %d: largest |y_gpu - y_ref| over its bound %.4f" % (so, sn, ratio.max()))
    assert ratio.max() <= 1.0


def test_capture_and_replay_equal_the_eager_call():
    import torch
    name, so, sn = CASES[4]
    c, rs = _case(name, so, sn), _resampler(name, so, sn)
    x = torch.from_numpy(np.array(c["q2"])).cuda()
    ns = torch.tensor(c["lengths"], dtype=torch.int32, device="cuda")
    eager = rs.resample(x, ns, channels=2)                      # (the handle's first call uploads the bank: before the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        rs.resample(x, ns, channels=2)                          # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = rs.resample(x, ns, channels=2)
    for t in captured:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(eager, captured))


class _HP(object):
    sample_rate, num_freq, frame_length_ms, frame_shift_ms = 24000, 65, 5, 1.25


def test_split_on_silence_with_orig_sr_is_resample_then_split():
    """A short synthetic recording at 44.1 kHz (0.25 s: three bursts over a noise floor), small frame parameters."""
    import taco_amd
    so, n = 44100, 11025
    rs_ = np.random.RandomState(5)
    x44 = 1e-4 * rs_.randn(n)
    for lo, hi in ((1000, 3500), (4800, 7000), (8200, 10500)):
        x44[lo:hi] = 0.3 * rs_.randn(hi - lo)
    x44 = x44.astype(np.float32)
    kw = dict(top_db=40, frame_length=64, hop_length=16, min_segment_length=0.01, max_segment_length=1.0)
    a_nb, a_seg = taco_amd.split_on_silence(x44, _HP(), orig_sr=so, **kw)
    rs = taco_amd.Resampler(so, _HP.sample_rate)
    y, yn = rs.resample(x44.reshape(1, -1))
    assert yn.tolist() == [rs.out_len(n)] == [y.shape[1]] == [len(a_nb)]
    b_nb, b_seg = taco_amd.split_on_silence(y[0].cpu().numpy(), _HP(), **kw)
    rs.close()
    assert len(a_seg) >= 2 and [s[:3] for s in a_seg] == [s[:3] for s in b_seg]                       # the intervals
    assert np.array_equal(a_nb.view(np.uint32), b_nb.view(np.uint32))
    assert all(np.array_equal(p[3].view(np.uint32), q[3].view(np.uint32)) for p, q in zip(a_seg, b_seg))   # the bits of the segments
