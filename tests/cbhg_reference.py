"""One CBHG in training mode on the CPU, float64 and float32, with reverse-mode autograd -- the yardstick of the block tests
(tests/test_cbhg_reference_host.py, tests/test_gpu_cbhg_train.py).  No GPU, no library: tests/torch_formulation.py::cbhg only.

The upstream gradient `dout` is an input, so the loss sum(out * dout) has no kink of its own; what kinks remain (ReLU of the conv
bank, of all projections but the last and of the highway H branch; the width-2 max-pool) are kept at a distance by the choice of
the seed:

  error bar of tensor k      bar_k = max(max|g32_k - g64_k|, 2^-20 * s_k),  s_k = max|g64_k|
                             (the float32 restatement's own error; the floor is 8 fp32 ulps of the largest element)
  structural zero            the bias of the LAST projection: no activation lies between it and the batch-statistics BatchNorm,
                             which removes any per-channel constant, so its float64 gradient is ~1e-16; its scale is max|g64| of
                             the same layer's beta.  (With ONE frame per row the beta of the projection before it is a second one,
                             see Reference; its scale is its layer's gamma's.)
  kink condition             with delta = 32 * max|z32 - z64| of a pre-activation tensor z: every ReLU pre-activation has
                             |z64| > delta, and the two candidates of every max-pool window differ by more than delta (delta of
                             the pool's input) -- except where both candidates come from a switched-off ReLU of the bank: those
                             are the same number in every arithmetic (see Reference), a tie that goes to the first frame
                             everywhere.  A seed is admissible when all of them hold; find_seed() returns the first admissible
                             seed from a base, and CASES pins what it returned."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import taco_oracle as O
import torch_formulation as TF
from util import tiny_hp

FLOOR = 2.0 ** -20
KINK_FACTOR = 32.0

# taco_train_debug_cbhg's `paths` word (include/taco_debug.h)
P_BANK_FWD_FUSED, P_BANK_FWD_PLAIN = 1 << 0, 1 << 1
P_POOL_BWD_FUSED, P_POOL_BWD_PLAIN = 1 << 2, 1 << 3
P_PROJ_BN_V4, P_PROJ_BN_PLAIN = 1 << 4, 1 << 5
P_BN_BWD_V4, P_BN_BWD_PLAIN = 1 << 6, 1 << 7
P_BANK_DZ_ONE, P_BANK_DZ_EACH = 1 << 8, 1 << 9
P_BANK_WG_PLANES, P_BANK_WG_EACH = 1 << 10, 1 << 11
P_HW_BWD_V4, P_HW_BWD_PLAIN = 1 << 12, 1 << 13
FWD_ROWS, FWD_RES, FWD_QUAD, FWD_DUO, FWD_OCT = (v << 16 for v in (1, 2, 3, 5, 6))
BWD_ROWS, BWD_RESB, BWD_DUO, BWD_OCT = (v << 20 for v in (1, 2, 3, 4))

_FUSED = P_BANK_FWD_FUSED | P_POOL_BWD_FUSED | P_BANK_DZ_ONE | P_HW_BWD_V4        # a bank whose channels are a multiple of 4
_UNFUSED = P_BANK_FWD_PLAIN | P_POOL_BWD_PLAIN | P_BANK_DZ_EACH | P_BN_BWD_PLAIN | P_HW_BWD_V4
_PROJ_V4 = P_PROJ_BN_V4 | P_BN_BWD_V4
_PROJ_PLAIN = P_PROJ_BN_PLAIN | P_BN_BWD_PLAIN
_TINY_SCAN = FWD_ROWS | BWD_ROWS


class Case(object):
    """One row of the table: `paths` is the word of the exact arm and of the default arm (bank kernel gradients one width at a time);
    planes2: with taco_train_set_wgrad_planes(2) the bank's kernel gradients come from pre-split planes (channels = 0 mod 32).
    paths_partition: the word on a partitioned device, where the whole-chip scans do not run (None: the same word).
    margins: tensors with a stated margin of their own over the common one, {name: (margin, reason)}."""

    def __init__(self, name, hp, scope, B, T, seed, paths, ragged=False, extras=False, planes2=False, paths_partition=None, margins=None):
        self.name, self.hp_fn, self.scope, self.B, self.T, self.seed = name, hp, scope, B, T, seed
        self.paths, self.ragged, self.extras, self.planes2 = paths, ragged, extras, planes2
        self.paths_partition = paths if paths_partition is None else paths_partition
        self.margins = margins or {}
        self.id = "%s-%s-B%d-T%d" % (name, scope.split("_")[0], B, T)

    def hp(self):
        return self.hp_fn()


def _odd_bank():
    return tiny_hp(enc_bank_channel_size=6, post_bank_channel_size=10)


def _odd_proj():
    return tiny_hp(enc_prenet_sizes=[32, 18], enc_proj_sizes=[14, 18], post_proj_sizes=[22, 8])


ENC, POST = "encoder_cbhg", "post_cbhg"
# seeds: find_seed(case, base=3), printed by `python tests/cbhg_reference.py` -- see tests/test_cbhg_reference_host.py::test_every_case_is_admissible_at_its_pinned_seed
CASES = [
    Case("aligned", tiny_hp, ENC, 3, 9, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True),
    Case("aligned", tiny_hp, POST, 3, 12, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("odd_bank", _odd_bank, ENC, 5, 13, 3, _UNFUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("odd_bank", _odd_bank, POST, 5, 13, 4, _UNFUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN),
    Case("odd_proj", _odd_proj, ENC, 5, 13, 5, _FUSED | _PROJ_PLAIN | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("odd_proj", _odd_proj, POST, 5, 13, 5, _FUSED | _PROJ_PLAIN | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("short", tiny_hp, ENC, 4, 1, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("short", tiny_hp, POST, 4, 1, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("short", tiny_hp, ENC, 3, 3, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("short", tiny_hp, POST, 3, 3, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("tiles", tiny_hp, ENC, 5, 13, 3, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("tiles", tiny_hp, POST, 5, 13, 5, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("tiles", tiny_hp, ENC, 7, 37, 29, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, ragged=True, extras=True),
    Case("tiles", tiny_hp, POST, 7, 37, 161, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | _TINY_SCAN, planes2=True),
    Case("reference", O.OracleHParams, ENC, 2, 12, 846, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | FWD_QUAD | BWD_RESB, ragged=True, extras=True,
         planes2=True),
    Case("reference", O.OracleHParams, POST, 2, 12, 2870, _FUSED | _PROJ_V4 | P_BANK_WG_EACH | FWD_DUO | BWD_DUO, planes2=True,
         paths_partition=_FUSED | _PROJ_V4 | P_BANK_WG_EACH | FWD_RES | BWD_ROWS),
]
COMMON_MARGIN = 8.0


def scope_dims(hp, scope):
    """(in_dim, rnn, bank widths K, highway depth, number of projections)"""
    if scope == ENC:
        return hp.enc_prenet_sizes[-1], hp.enc_rnn_size, hp.enc_bank_size, hp.enc_highway_depth, len(hp.enc_proj_sizes)
    return hp.num_mels, hp.post_rnn_size, hp.post_bank_size, hp.post_highway_depth, len(hp.post_proj_sizes)


def make_inputs(hp, scope, B, T, seed, ragged, extras):
    """Weights of the whole model from O.init_weights(seed) and the block's data from RandomState(seed + 1): x, dout ~ randn; lengths in
    [1, T] (row 0 full) when ragged; h0 / before (what a deepvoice model feeds the encoder) when extras."""
    in_dim, rnn, _, _, _ = scope_dims(hp, scope)
    w = O.init_weights(hp, 1, seed)
    rs = np.random.RandomState(seed + 1)
    d = {"w": w, "x": rs.randn(B, T, in_dim).astype(np.float32), "dout": rs.randn(B, T, 2 * rnn).astype(np.float32),
         "lengths": None, "h0": None, "before": None}
    if ragged:
        L = rs.randint(1, T + 1, size=B).astype(np.int32)
        L[0] = T
        d["lengths"] = L
    if extras:
        d["h0"] = (rs.randn(B, 2 * rnn) * 0.5).astype(np.float32)
        d["before"] = (rs.randn(B, in_dim) * 0.5).astype(np.float32)
    return d


class _Recorder(object):
    """Stands in for torch.nn.functional inside torch_formulation for one call: records every ReLU input and the two candidates of
    every max-pool window, and passes everything through."""

    def __init__(self):
        self.relu_in, self.pool_pairs = [], []

    def __getattr__(self, name):
        return getattr(F, name)

    def relu(self, y):
        self.relu_in.append(y)
        return F.relu(y)

    def max_pool1d(self, x, k, s):
        assert k == 2 and s == 1          # x is right-padded with -inf: window t = (x[t], x[t + 1]); the last window has one finite candidate
        self.pool_pairs.append((x[..., :-2], x[..., 1:-1]))
        return F.max_pool1d(x, k, s)


def evaluate(hp, scope, inp, dtype):
    """torch_formulation.cbhg(training=True) at `dtype` + autograd of sum(out * dout).  Returns (tensors, relu, pool): tensors = out, din,
    dh0, dbefore (where given) and every parameter gradient of the scope by its name; relu = the ReLU pre-activations in call order (bank
    widths, projections but the last, highway H); pool = (first, second) candidates of the max-pool windows.  All float64 NumPy."""
    _, _, K, depth, nproj = scope_dims(hp, scope)
    old_dt, old_F, old_nt = TF.DT, TF.F, torch.get_num_threads()
    rec = _Recorder()
    TF.DT, TF.F = dtype, rec
    torch.set_num_threads(1)          # one summation order for the float32 run, whatever the host
    try:
        w = {}
        for k, v in inp["w"].items():
            if k.startswith(scope + "/"):
                t = torch.tensor(np.asarray(v), dtype=dtype)
                if not k.endswith(("/moving_mean", "/moving_variance")):
                    t.requires_grad_(True)
                w[k] = t
        x = torch.tensor(inp["x"], dtype=dtype, requires_grad=True)
        h0 = None if inp["h0"] is None else torch.tensor(inp["h0"], dtype=dtype, requires_grad=True)
        before = None if inp["before"] is None else torch.tensor(inp["before"], dtype=dtype, requires_grad=True)
        out = TF.cbhg(x, inp["lengths"], w, scope, K, depth, nproj, before=before, init=h0, training=True)
        (out * torch.tensor(inp["dout"], dtype=dtype)).sum().backward()
    finally:
        TF.DT, TF.F = old_dt, old_F
        torch.set_num_threads(old_nt)
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    res = {"out": f64(out), "din": f64(x.grad)}
    if h0 is not None:
        res["dh0"] = f64(h0.grad)
    if before is not None:
        res["dbefore"] = f64(before.grad)
    for k, t in w.items():
        if t.requires_grad:
            res[k] = f64(t.grad) if t.grad is not None else np.zeros(tuple(t.shape))
    assert len(rec.relu_in) == K + (nproj - 1) + depth and len(rec.pool_pairs) == 1
    return res, [f64(z) for z in rec.relu_in], tuple(f64(c) for c in rec.pool_pairs[0])


class Reference(object):
    """float64 and float32 evaluations of one case, the per-tensor bars, and the kink report."""

    def __init__(self, hp, scope, inp):
        self.hp, self.scope, self.inp = hp, scope, inp
        self.ref64, relu64, pool64 = evaluate(hp, scope, inp, torch.float64)
        self.ref32, relu32, pool32 = evaluate(hp, scope, inp, torch.float32)
        nproj = scope_dims(hp, scope)[4]
        last = "%s/proj_%d" % (scope, nproj)
        self.structural_zero = {last + "/bias": last + "/beta"}
        if inp["x"].shape[1] == 1 and nproj > 1:
            # one frame: SAME padding leaves the last projection its centre tap alone, a plain matrix -- a per-channel constant of its input
            # (the beta in front of it) is then a per-channel constant of its output, which its batch-statistics BatchNorm removes as well
            prev = "%s/proj_%d" % (scope, nproj - 1)
            self.structural_zero[prev + "/beta"] = prev + "/gamma"
        self.scale, self.bars = {}, {}
        for k, g in self.ref64.items():
            s = float(np.abs(self.ref64[self.structural_zero.get(k, k)]).max())
            self.scale[k] = s
            self.bars[k] = max(float(np.abs(self.ref32[k] - g).max()) if g.size else 0.0, FLOOR * s)
        # kinks: (smallest distance from the kink, delta) per pre-activation tensor
        self.kinks = []
        for i, (z64, z32) in enumerate(zip(relu64, relu32)):
            self.kinks.append(("relu_%d" % i, float(np.abs(z64).min()), KINK_FACTOR * float(np.abs(z32 - z64).max())))
        if pool64[0].size:
            dpool = KINK_FACTOR * max(float(np.abs(a - b).max()) for a, b in zip(pool32, pool64))
            # a window whose two candidates both come from a switched-off ReLU is no kink: the bank applies ReLU BEFORE BatchNorm, so both hold
            # the BatchNorm of 0 with the same channel's constants -- the same number in every arithmetic, a tie that every implementation
            # (autograd's max_pool1d and both pool kernels) gives to the first frame.  The ReLU condition above keeps those inputs off zero.
            K = scope_dims(hp, scope)[2]
            off = np.concatenate(relu64[:K], axis=1) <= 0          # [B, K*C, T], the pool input's layout
            gap = np.abs(pool64[0] - pool64[1])[~(off[..., :-1] & off[..., 1:])]
            self.structural_ties = int((off[..., :-1] & off[..., 1:]).sum())
            self.kinks.append(("pool", float(gap.min()) if gap.size else float("inf"), dpool))

    def admissible(self, safety=1.0):
        return all(dist > safety * delta for _, dist, delta in self.kinks)


def compare(got, ref64, bars, margin, margins=None):
    """The tensors of `got` over margin * bar_k (margins: {name: (margin, reason)} replaces the common one for a tensor), as a list of
    (name, ratio) with ratio = max|got_k - ref64_k| / bar_k, worst first.  Every tensor of ref64 must be in `got`; a non-finite
    element counts as an infinite ratio."""
    bad = []
    for k, ratio in ratios(got, ref64, bars).items():
        m = margins[k][0] if margins and k in margins else margin
        if not ratio <= m:
            bad.append((k, ratio))
    return sorted(bad, key=lambda kr: -kr[1])


def ratios(got, ref64, bars):
    out = {}
    for k, g in ref64.items():
        a = np.asarray(got[k], np.float64).reshape(g.shape)
        err = float(np.abs(a - g).max()) if g.size else 0.0
        out[k] = err / bars[k] if np.isfinite(err) else float("inf")
    return out


@functools.lru_cache(maxsize=None)
def _reference(case_index, seed):
    c = CASES[case_index]
    hp = c.hp()
    return Reference(hp, c.scope, make_inputs(hp, c.scope, c.B, c.T, seed, c.ragged, c.extras))


def reference(case):
    """The (cached, shared, read-only) reference of a case of the table at its pinned seed."""
    return _reference(CASES.index(case), case.seed)


def find_seed(case, base=3, tries=4000):
    """The first seed >= base that is admissible with TWICE the distance: delta is measured on a float32 run, whose rounding differs a
    little from one host's BLAS to the next, and the pinned seed has to be admissible (at the plain factor) on every one of them."""
    hp = case.hp()
    for seed in range(base, base + tries):
        if Reference(hp, case.scope, make_inputs(hp, case.scope, case.B, case.T, seed, case.ragged, case.extras)).admissible(2.0):
            return seed
    raise RuntimeError("no admissible seed in [%d, %d) for %s" % (base, base + tries, case.id))


def _find(i):
    torch.set_num_threads(1)
    return CASES[i].id, find_seed(CASES[i])


if __name__ == "__main__":       # prints the seeds that CASES pins
    import multiprocessing
    with multiprocessing.Pool(8) as pool:
        for cid, seed in pool.imap(_find, range(len(CASES))):
            print(cid, seed, flush=True)
