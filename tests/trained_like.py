"""Weights without a constant vector, and the index mistakes such weights make visible (NumPy only).

oracle/taco_oracle.py::init_weights and weights.random_weights follow the reference's initialisers: every GRU */gates/bias is 1.0 in all
2H entries, every highway */T/bias is -1.0, attention_score_bias is 0.  A trained checkpoint has none of these constants, and a kernel that
reads such a vector through the wrong index (r and u halves swapped, one column off, the other direction's or layer's vector) computes
exactly the same on the constant ones.  trained_like() moves them, mutations() lists the index mistakes as weight sets the float64 oracle
can run: tests/test_trained_like_host.py measures what each of them does to the outputs, tests/test_gpu_trained_like.py holds the kernels
to the oracle on the moved weights."""
import numpy as np

VECTOR_LEAVES = ("bias", "beta", "gamma", "moving_mean", "moving_variance", "attention_b")


def _constant(a):
    return a.size > 0 and bool(np.all(a == a.flat[0]))


def trained_like(w, seed):
    """A float32 copy of the weight dict `w`: every */gates/bias 1 + U(-0.5, 0.5) per element, every */T/bias -1 + U(-0.5, 0.5),
    attention_score_bias U(0.5, 1.5), attention_g times 1.3; any other bias / beta / moving_mean that is constant (random_weights leaves
    them at 0) gets U(-0.2, 0.2) added, a constant gamma / moving_variance U(0, 0.5).  Names in sorted order, uniform draws only."""
    rs = np.random.RandomState(seed)
    out = {}
    for name in sorted(w):
        a = np.array(w[name], dtype=np.float32)
        leaf = name.rsplit("/", 1)[-1]
        if name.endswith("/gates/bias"):
            a = 1.0 + rs.uniform(-0.5, 0.5, size=a.shape)
        elif name.endswith("/T/bias"):
            a = -1.0 + rs.uniform(-0.5, 0.5, size=a.shape)
        elif name == "attention/attention_score_bias":
            a = rs.uniform(0.5, 1.5, size=a.shape)
        elif name == "attention/attention_g":
            a = a * 1.3
        elif leaf in ("bias", "beta", "moving_mean", "attention_b") and _constant(a):      # (attention_b: the bias inside the score's tanh)
            a = a + rs.uniform(-0.2, 0.2, size=a.shape)
        elif leaf in ("gamma", "moving_variance") and _constant(a):
            a = a + rs.uniform(0.0, 0.5, size=a.shape)
        out[name] = np.asarray(a, dtype=np.float32)
    for name, a in out.items():
        if name.rsplit("/", 1)[-1] in VECTOR_LEAVES and a.size > 1:
            assert not _constant(a), name
        if name.endswith("/gates/bias"):
            h = a.shape[0] // 2
            assert not np.array_equal(a[:h], a[h:]), name
    return out


def _swap(a):
    h = a.shape[0] // 2
    return np.concatenate([a[h:], a[:h]])


def _roll(a):
    return np.roll(a, 1)


def mutations(w):
    """(name, how, w') for every index mistake on a bias vector of `w`: the r and u halves of a */gates/bias swapped ('swap'), and a
    */gates/bias, */T/bias or */candidate/bias read one column off ('roll').  w' shares every other array with w."""
    for name in sorted(w):
        if name.endswith("/gates/bias"):
            hows = (("swap", _swap), ("roll", _roll))
        elif name.endswith(("/T/bias", "/candidate/bias")):
            hows = (("roll", _roll),)
        else:
            continue
        for how, fn in hows:
            m = dict(w)
            m[name] = np.ascontiguousarray(fn(np.asarray(w[name])))
            yield name, how, m
