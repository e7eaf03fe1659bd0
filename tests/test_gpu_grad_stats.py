"""Training summaries on the device (add_stats, train.py:50-77): the segmented norms of taco_segment_norms against float64 NumPy -- every
norm, the maximum, its index and the global norm to one fp32 ulp --, their specified edge behaviour, their determinism across
streams and in a replayed graph, the trainer's per-variable gradient norms against grad_dict(), and Tacotron.add_stats on the models
of train.py:145-168.

Why one ulp: squares and sums are doubles.  A sum of n exact squares carries a relative error of at most n * 2^-53 (n < 2^17 here:
below 2^-36), the square root and NumPy's own sum add a few 2^-53 more; all of it is far below the 2^-24 of the one rounding to
fp32 that follows, so the result is the correctly rounded float or, when the exact value lies within ~2^-36 of a rounding boundary, its
neighbour."""
import ctypes as C

import numpy as np
import pytest

import taco_oracle as O
from util import tiny_hp, to_product_hp

pytestmark = pytest.mark.gpu

_CACHE = {}


def _lens(P):
    return [0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, P - 1, P, P + 1, 2 * P + 3, 1, 0, 3 * P]


SKIPPED = (3, 9, 12, 14, 16)          # a short one, a middle one, a whole piece, the three-piece one, an empty one


def _layout():
    """The one layout of the op-level tests: its offsets, seeded values, float64 reference and two device plans (made once)."""
    if _CACHE:
        return _CACHE
    import torch
    from taco_amd import _lib
    lib = _lib.load_library()
    P = lib.taco_segnorm_piece_floats()
    lens = _lens(P)
    off = np.concatenate([[1], 1 + np.cumsum(lens)]).astype(np.uint64)          # starts at element 1: the first segment is unaligned
    n = int(off[-1]) + 5                                                        # five elements behind the last segment belong to none
    assert n < 100000
    rs = np.random.RandomState(11)
    scales = np.logspace(-20, 15, len(lens))[rs.permutation(len(lens))]
    x = np.zeros(n, np.float32)
    for s, ln in enumerate(lens):
        x[int(off[s]):int(off[s + 1])] = (rs.standard_normal(ln) * scales[s]).astype(np.float32)
    x[0] = np.nan
    x[int(off[-1]):] = np.nan                                                   # outside every segment: never read
    skip = np.zeros(len(lens), np.uint8)
    skip[list(SKIPPED)] = 1
    plans = []
    for sk in (None, skip):
        h = C.c_void_p()
        _lib.check(lib.taco_segnorm_plan_create(off.ctypes.data_as(C.POINTER(C.c_uint64)), len(lens),
                                                None if sk is None else sk.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                torch.cuda.current_device(), C.byref(h)))
        plans.append(h)
    _CACHE.update(lib=lib, P=P, lens=lens, off=off.astype(np.int64), n=n, x=x, skip=skip, plan=plans[0], plan_skip=plans[1])
    return _CACHE


def _reference(x, off, skip=None):
    """float64 NumPy: (norms [n_seg] as float32, max, argmax, global norm as float32)"""
    n_seg = len(off) - 1
    sq = np.array([np.sum(x[off[s]:off[s + 1]].astype(np.float64) ** 2) for s in range(n_seg)])
    counted = np.ones(n_seg, bool) if skip is None else skip == 0
    sq = np.where(counted, sq, 0.0)
    with np.errstate(over="ignore"):
        norms = np.sqrt(sq).astype(np.float32)
        glob = np.float32(np.sqrt(np.sum(sq[counted])))
    idx = np.flatnonzero(counted)
    nan = idx[np.isnan(norms[idx])]
    am = int(nan[0]) if len(nan) else int(idx[np.argmax(norms[idx])])           # np.argmax: the first index of the maximum
    return norms, norms[am], am, glob


def _run(plan, xd, out=None):
    """taco_segment_norms on the current stream -> (norms, stats, argmax) device tensors"""
    import torch
    from taco_amd import _lib
    L = _layout()
    if out is None:
        out = (torch.full((len(L["lens"]),), -1.0, device="cuda"), torch.full((2,), -1.0, device="cuda"),
               torch.full((1,), -9, dtype=torch.int32, device="cuda"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L["lib"].taco_segment_norms(plan, st, C.c_void_p(xd.data_ptr()), xd.numel(), C.c_void_p(out[0].data_ptr()),
                                          C.c_void_p(out[1].data_ptr()), C.c_void_p(out[2].data_ptr())))
    return out


def _host(out):
    import torch
    torch.cuda.synchronize()
    return out[0].cpu().numpy(), out[1].cpu().numpy(), int(out[2].cpu().numpy()[0])


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _within_one_ulp(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want)).astype(np.float64)


def test_segment_norms_against_float64_numpy():
    import torch
    L = _layout()
    want, wmax, wam, wglob = _reference(L["x"], L["off"])
    norms, stats, am = _host(_run(L["plan"], torch.from_numpy(L["x"]).cuda()))
    equal = int(np.sum(_bits(norms) == _bits(want)))
    print("segment norms: %d of %d bit-equal to float32(sqrt(float64 sum)); max %r / %r, global %r / %r"
          % (equal, len(want), stats[0], wmax, stats[1], wglob))
    assert np.all(np.isfinite(want)) and np.all(np.isfinite(norms))
    ok = _within_one_ulp(norms, want)
    assert ok.all(), [(s, norms[s], want[s]) for s in np.flatnonzero(~ok)]
    assert norms[0] == 0 and norms[16] == 0                                     # the empty segments
    assert am == wam and _bits(stats[0]) == _bits(norms[am])                    # the maximum IS one of the norms
    assert _within_one_ulp(stats[0], wmax) and _within_one_ulp(stats[1], wglob)


def test_skipped_segments_are_not_read_and_count_nowhere():
    """NaN only inside skipped segments: every output is finite, their norms are 0, and maximum, index and global norm are those of
    the counted segments."""
    import torch
    L = _layout()
    x, off = L["x"].copy(), L["off"]
    for s in SKIPPED:
        x[off[s]:off[s + 1]] = np.nan
    want, wmax, wam, wglob = _reference(x, off, L["skip"])
    norms, stats, am = _host(_run(L["plan_skip"], torch.from_numpy(x).cuda()))
    assert np.all(np.isfinite(norms)) and np.all(np.isfinite(stats))
    assert all(norms[s] == 0 for s in SKIPPED)
    assert _within_one_ulp(norms, want).all()
    assert am == wam and am not in SKIPPED and _bits(stats[0]) == _bits(norms[am])
    assert _within_one_ulp(stats[0], wmax) and _within_one_ulp(stats[1], wglob)


def test_edge_cases_on_the_same_layout():
    import torch
    L = _layout()
    off, n = L["off"], L["n"]
    seg = lambda s: slice(int(off[s]), int(off[s + 1]))
    base = L["x"].copy()
    base_norms = _host(_run(L["plan"], torch.from_numpy(base).cuda()))[0]

    # all zero: every norm 0, the first index holds the maximum
    norms, stats, am = _host(_run(L["plan"], torch.zeros(n, device="cuda")))
    assert not norms.any() and not stats.any() and am == 0 and not np.signbit(norms).any()

    # ties go to the first index: 5 in segments 11 and 13 (one element each -- in 13 its last, a piece of its own), 3 in segments 4 and 7
    x = np.zeros(n, np.float32)
    x[off[14] - 1], x[off[11] + 17], x[off[7] + 7], x[off[4]] = 5.0, -5.0, 3.0, 3.0
    norms, stats, am = _host(_run(L["plan"], torch.from_numpy(x).cuda()))
    assert norms[11] == 5 and norms[13] == 5 and norms[4] == 3 and norms[7] == 3 and np.count_nonzero(norms) == 4
    assert stats[0] == 5 and am == 11 and _within_one_ulp(stats[1], np.float32(np.sqrt(68.0)))

    # one NaN in a counted segment: the maximum is NaN and points at it; a second NaN segment behind it changes nothing
    x = base.copy()
    x[off[9] + 100] = np.nan
    for extra in (False, True):
        if extra:
            x[off[13] + 1] = np.nan
        norms, stats, am = _host(_run(L["plan"], torch.from_numpy(x).cuda()))
        assert np.isnan(stats[0]) and am == 9 and np.isnan(norms[9]) and np.isnan(stats[1])
        others = [s for s in range(len(norms)) if s != 9 and not (extra and s == 13)]
        assert np.array_equal(_bits(norms[others]), _bits(base_norms[others]))
    # ... also when it is the very first element of the first non-empty segment (where k_train_latch puts it)
    x = base.copy()
    x[off[1]] = np.nan
    norms, stats, am = _host(_run(L["plan"], torch.from_numpy(x).cuda()))
    assert np.isnan(stats[0]) and am == 1

    # one inf
    x = base.copy()
    x[off[6] + 3] = -np.inf
    norms, stats, am = _host(_run(L["plan"], torch.from_numpy(x).cuda()))
    assert norms[6] == np.inf and stats[0] == np.inf and am == 6 and stats[1] == np.inf
    assert np.array_equal(_bits(np.delete(norms, 6)), _bits(np.delete(base_norms, 6)))

    # four values of 3e38: the sum of squares is fine in double, the norm 6e38 is beyond fp32: +inf
    x = base.copy()
    x[seg(4)] = 3e38
    norms, stats, am = _host(_run(L["plan"], torch.from_numpy(x).cuda()))
    assert norms[4] == np.inf and stats[0] == np.inf and am == 4 and stats[1] == np.inf and np.isfinite(np.delete(norms, 4)).all()


def test_two_streams_and_a_replayed_graph_give_the_same_bits():
    import torch
    L = _layout()
    xd = torch.from_numpy(L["x"]).cuda()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        a = _run(L["plan"], xd)
    s2.wait_stream(s1)                                                          # calls on one plan are ordered among themselves
    with torch.cuda.stream(s2):
        b = _run(L["plan"], xd)
    a, b = _host(a), _host(b)
    assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[2] == b[2]

    # capture the call, overwrite the buffer in place, replay: the new buffer's values, bit-equal to an eager call
    static = xd.clone()
    out = _run(L["plan"], static)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _run(L["plan"], static, out)
    rs = np.random.RandomState(12)
    y = (rs.standard_normal(L["n"]) * 3).astype(np.float32)
    static.copy_(torch.from_numpy(y).cuda())
    for t in out:
        t.fill_(-3)
    g.replay()
    replayed = _host(out)
    eager = _host(_run(L["plan"], static))
    assert np.array_equal(_bits(replayed[0]), _bits(eager[0])) and np.array_equal(_bits(replayed[1]), _bits(eager[1])) and replayed[2] == eager[2]
    want = _reference(y, L["off"])
    assert _within_one_ulp(replayed[0], want[0]).all() and replayed[2] == want[2] and _within_one_ulp(replayed[1][1], want[3])
    assert np.array_equal(_bits(a[0]), _bits(_host(_run(L["plan"], xd))[0]))    # and the first buffer still gives its own bits


# ---- the trainer ----
def _train_setup(config, B=3, T_in=9, T_out=12, seed=5):
    kw, ns = {"bah_mon": (dict(attention_type="bah_mon"), 1), "bah_norm": (dict(attention_type="bah_norm"), 1),
              "deepvoice": (dict(model_type="deepvoice", speaker_embedding_size=4, attention_type="bah_mon"), 2)}[config]
    hp = tiny_hp(**kw)
    w = O.init_weights(hp, ns, seed)
    ids, L = O.synthetic_inputs(B, T_in, seed + 6, ragged=True)
    rs = np.random.RandomState(seed + 1)
    mt, lt = rs.rand(B, T_out, hp.num_mels), rs.rand(B, T_out, hp.num_freq)
    co = rs.uniform(0.5, 1.5, size=B)
    spk = np.array([1, 0, 1], np.int32) if ns > 1 else None
    return hp, w, ns, (ids, L, mt, lt, co), spk


@pytest.mark.parametrize("config,scalar", [("bah_mon", "attention/attention_score_bias"), ("bah_norm", "attention/attention_g"),
                                           ("deepvoice", "spk/before_highway/bias")])
def test_trainer_gradient_norms_match_grad_dict(config, scalar):
    import torch
    import taco_amd
    from taco_amd import _lib
    hp, w, ns, batch, spk = _train_setup(config)
    tr = taco_amd.Trainer(to_product_hp(hp), w, num_speakers=ns)
    twin = taco_amd.Trainer(to_product_hp(hp), w, num_speakers=ns)                # never asks for a gradient norm
    names = [n for n, _ in tr.spec]
    moving = [n for n in names if n.endswith("/moving_mean") or n.endswith("/moving_variance")]
    assert moving and tr.trainable == [n for n in names if n not in moving] and scalar in tr.trainable
    if config == "deepvoice":
        assert [n for n in tr.trainable if n.startswith("spk/")] and "speaker_embedding" in tr.trainable

    tr.forward_backward(*batch, speaker_id=spk, freeze_moving_averages=True)
    stats = tr.gradient_stats()
    dev_norms, dev_stats, dev_am = (t.cpu().numpy() for t in tr.gradient_norms())
    g = tr.grad_dict()
    want = {n: np.float32(np.sqrt(np.sum(g[n].astype(np.float64) ** 2))) for n in tr.trainable}
    assert list(stats["norms"]) == tr.trainable                                 # the moving statistics are absent ...
    assert all(dev_norms[names.index(n)] == 0 for n in moving)                  # ... and their slots in the device vector are 0
    bad = [(n, stats["norms"][n], want[n]) for n in tr.trainable if not _within_one_ulp(stats["norms"][n], want[n])]
    assert not bad, bad
    assert all(np.float32(stats["norms"][n]) == dev_norms[names.index(n)] for n in tr.trainable)
    assert stats["norms"][scalar] > 0
    if g[scalar].size == 1:                                                     # the norm of a scalar is its magnitude, exactly
        assert np.float32(stats["norms"][scalar]) == np.abs(np.float32(g[scalar]).reshape(-1)[0])
    # maximum and its variable against NumPy
    order = sorted(tr.trainable, key=lambda n: -want[n])
    assert _within_one_ulp(stats["max_gradient_norm"], want[order[0]])
    assert stats["max_gradient_norm"] == stats["norms"][stats["argmax"]] and names[int(dev_am[0])] == stats["argmax"]
    first_max = tr.trainable[int(np.argmax([dev_norms[names.index(n)] for n in tr.trainable]))]
    assert stats["argmax"] == first_max
    if want[order[0]] - want[order[1]] > 2 * np.spacing(want[order[0]]):        # (no near-tie at the top: the name is NumPy's too)
        assert stats["argmax"] == order[0]
    glob = np.float32(np.sqrt(np.sum([np.sum(g[n].astype(np.float64) ** 2) for n in tr.trainable])))
    assert _within_one_ulp(stats["global_norm"], glob) and np.float32(stats["global_norm"]) == dev_stats[1]

    # the argument errors that need the trainer's size: outputs inside the gradient buffer
    lib, P = tr._lib, lambda t, o=0: C.c_void_p(t.data_ptr() + o)
    ok_n, ok_s = torch.empty(len(names), device="cuda"), torch.empty(2, device="cuda")
    for dn, ds in ((P(tr.grads), P(ok_s)), (P(tr.grads, 4 * (tr.num_params - 1)), P(ok_s)), (P(ok_n), P(tr.grads, 8))):
        assert lib.taco_train_grad_norms(tr._h, None, P(tr.grads), dn, ds, None) == _lib.TACO_ERR_ARG
        assert b"overlap" in lib.taco_last_error()

    # the step: clip_by_global_norm's norm is the same number (both double sums, in different orders: 2 ulp), and asking for the
    # norms touches nothing of the step
    tr.train_step(*batch, speaker_id=spk)
    twin.train_step(*batch, speaker_id=spk)
    after = tr.gradient_stats()                                                 # (the update reads the gradients, it does not change them)
    gnorm = np.float32(tr.adam.gnorm.cpu().numpy()[0])
    for v in (stats["global_norm"], after["global_norm"]):
        assert abs(np.float64(np.float32(v)) - np.float64(gnorm)) <= 2 * np.float64(np.spacing(gnorm)), (v, gnorm)
    torch.cuda.synchronize()
    assert torch.equal(tr.params.view(torch.int32), twin.params.view(torch.int32))
    assert torch.equal(tr.adam.m.view(torch.int32), twin.adam.m.view(torch.int32))
    tr.close()
    twin.close()


def test_a_poisoned_step_shows_in_the_summary():
    """k_train_latch writes NaN into grads[0] after a device fault: the maximum is NaN and names the first variable."""
    import taco_amd
    hp, w, ns, batch, spk = _train_setup("bah_mon")
    tr = taco_amd.Trainer(to_product_hp(hp), w)
    tr.forward_backward(*batch, freeze_moving_averages=True)
    tr.grads[0] = float("nan")
    s = tr.gradient_stats()
    assert np.isnan(s["max_gradient_norm"]) and s["argmax"] == tr.spec[0][0] and np.isnan(s["global_norm"])
    assert np.isnan(s["norms"][tr.spec[0][0]]) and all(np.isfinite(v) for n, v in s["norms"].items() if n != tr.spec[0][0])
    tr.close()


def test_add_stats_mirrors_train_py():
    """train.py:145-168 through the model objects: `add_stats(model)` and `add_stats(test_model, model, 'test')`."""
    import taco_amd
    hp, w, ns, (ids, L, mt, lt, co), spk = _train_setup("bah_mon", seed=21)
    php = to_product_hp(hp)
    model = taco_amd.create_model(php)
    model.load_weights(w)
    model.initialize(ids, L, 1, None, mel_targets=mt, linear_targets=lt, loss_coeff=co, is_randomly_initialized=True)
    model.add_loss()
    model.add_optimizer(0)
    test_model = taco_amd.create_model(php).share_variables_with(model)
    test_model.initialize(ids, L, 1, None, mel_targets=mt, linear_targets=lt, loss_coeff=co, rnn_decoder_test_mode=True)
    test_model.add_loss()
    with pytest.raises(taco_amd._lib.TacoError) as e:                           # no backward pass yet: nothing to take a norm of
        model.add_stats()
    assert e.value.code == taco_amd._lib.TACO_ERR_STATE
    assert list(model.add_stats(scope_name="stats")) == ["stats/loss_mel", "stats/loss_linear", "stats/loss"]      # train.py:156
    step, lwc = model.train_step()
    s = model.add_stats()
    assert list(s) == ["train/loss_mel", "train/loss_linear", "train/loss", "train/learning_rate", "train/max_gradient_norm"]
    assert all(type(v) is float for v in s.values())
    assert (s["train/loss_mel"], s["train/loss_linear"], s["train/loss"]) == (float(model.mel_loss), float(model.linear_loss), float(model.loss_without_coeff))
    assert s["train/loss"] == float(lwc) and s["train/learning_rate"] == model._trainer.learning_rate == model.learning_rate
    gs = model._trainer.gradient_stats()
    assert s["train/max_gradient_norm"] == gs["max_gradient_norm"] and np.isfinite(gs["max_gradient_norm"]) and gs["max_gradient_norm"] > 0
    t = test_model.add_stats(model, "test")                                     # train.py:168
    assert list(t) == ["test/loss_mel", "test/loss_linear", "test/loss", "gap_test-train/loss_mel", "gap_test-train/loss_linear",
                       "gap_test-train/loss"]
    assert t["test/loss"] == float(test_model.loss_without_coeff)
    assert t["gap_test-train/loss_mel"] == float(test_model.mel_loss) - float(model.mel_loss)
    assert t["gap_test-train/loss_linear"] == float(test_model.linear_loss) - float(model.linear_loss)
    assert t["gap_test-train/loss"] == float(test_model.loss_without_coeff) - float(model.loss_without_coeff)
    assert t["gap_test-train/loss"] != 0                                        # the two models do differ (one is fed its own outputs)
