"""The yardstick of tests/test_gpu_trained_like.py, checked on the float64 oracle alone (no GPU).

For every forward case of that file:
  * the gap, kept as a record: on init_weights every index mistake on a GRU gate bias or a highway T bias (r / u halves swapped, one column
    off: trained_like.mutations) changes mel, linear and alignments by exactly 0 -- the vectors are constant;
  * on trained_like weights every such mistake, and a candidate bias one column off, moves mel, linear or alignments by at least ten times
    the bar the GPU test puts on that array -- a kernel that makes it cannot pass;
  * the alignment criterion compares every step (none masked by util.ARGMAX_FLOOR), and in the bah_mon cases the top two positions of every
    step are at least 1e-4 of the peak apart: five times util.ARGMAX_TIE, so no step of the oracle is a tie at fp32 resolution."""
import numpy as np
import pytest

import taco_oracle as O
from test_gpu_trained_like import ARRAYS, FORWARD_CASES, forward_case, oracle_forward, oracle_reference
from trained_like import mutations, trained_like
from util import argmax_detail, maxabs


def test_trained_like_recipe():
    """random_weights' constants (zero biases, identity BatchNorm) and init_weights' (gate and T biases): no vector of more than one
    element stays constant, the two halves of every gate bias differ, kernels and embeddings are untouched, all float32, seeded."""
    import taco_amd
    ohp = O.OracleHParams(max_iters=2, attention_type="bah_norm", model_type="deepvoice")
    for w in (O.init_weights(ohp, 3, 5), taco_amd.weights.random_weights(taco_amd.HParams(**ohp.to_dict()), 3, seed=5)):
        t = trained_like(w, 6)
        assert sorted(t) == sorted(w) and all(t[k].dtype == np.float32 and t[k].shape == np.shape(w[k]) for k in w)
        for k in w:
            leaf = k.rsplit("/", 1)[-1]
            if leaf in ("kernel", "table", "attention_v") or k in ("embedding", "speaker_embedding"):
                assert np.array_equal(t[k], w[k]), k
            elif t[k].size > 1:
                assert np.unique(t[k]).size > t[k].size // 2, k
        g = t["decoder/gru_1/gates/bias"]
        assert 0.5 <= g.min() and g.max() <= 1.5 and not np.array_equal(g[:256], g[256:])
        b = t["post_cbhg/highway_3/T/bias"]
        assert -1.5 <= b.min() and b.max() <= -0.5
        assert np.isclose(t["attention/attention_g"], 1.3 * w["attention/attention_g"])
        again = trained_like(w, 6)
        assert all(np.array_equal(t[k], again[k]) for k in t)
        assert not np.array_equal(t["decoder/gru_1/gates/bias"], trained_like(w, 7)["decoder/gru_1/gates/bias"])
    ohp = O.OracleHParams(max_iters=2)
    sb = trained_like(O.init_weights(ohp, 1, 5), 6)["attention/attention_score_bias"]
    assert sb.shape == () and 0.5 <= float(sb) <= 1.5
    names = [(n, how) for n, how, _ in mutations(O.init_weights(ohp, 1, 5))]
    assert len(names) == 7 * 2 + 8 + 7 and len(set(names)) == len(names)      # seven GRUs (swap, roll), eight T biases, seven candidate biases


@pytest.mark.parametrize("name", sorted(FORWARD_CASES))
def test_bias_index_mistakes_are_invisible_on_init_weights_and_worth_ten_bars_on_trained_like(name):
    ohp, ns, w0, w, ids, L, spk, bar = forward_case(name)
    base0, base = oracle_forward(name, w0), oracle_reference(name)
    worst = {}
    for vec, how, wm in mutations(w0):
        if vec.endswith("/candidate/bias"):
            continue                      # (init_weights draws these; only the gate and T biases are constants)
        out = oracle_forward(name, wm)
        assert all(maxabs(out[k], base0[k]) == 0.0 for k in ARRAYS), (vec, how)
    for vec, how, wm in mutations(w):
        out = oracle_forward(name, wm)
        moved = max(maxabs(out[k], base[k]) for k in ARRAYS)
        kind = vec.rsplit("/", 2)[-2]
        worst[kind] = min(worst.get(kind, np.inf), moved / bar)
        assert moved >= 10 * bar, (vec, how, moved, bar)
    print("%s: the least a mutation moves mel / linear / alignments, in bars of %.0e: %s" % (name, bar, {k: round(v, 1) for k, v in sorted(worst.items())}))


@pytest.mark.parametrize("name", sorted(FORWARD_CASES))
def test_the_oracles_alignments_leave_nothing_to_the_floor_or_to_ties(name):
    al = oracle_reference(name)["alignments"]
    d = argmax_detail(al, al)
    peak = al.max(axis=1)
    assert d["masked_by_floor"] == 0 and d["compared"] == d["steps"] == peak.size
    top = np.sort(al, axis=1)[:, -2:, :]
    gap = float(((top[:, 1] - top[:, 0]) / top[:, 1]).min())
    print("%s: smallest peak %.3g, smallest top-two gap %.3g of the peak" % (name, peak.min(), gap))
    assert peak.min() > 1e-2
    if FORWARD_CASES[name][2] == "bah_mon":
        assert gap >= 1e-4
