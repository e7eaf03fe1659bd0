"""The yardstick of the CBHG block test (tests/cbhg_reference.py) checked on the CPU: the pinned seeds keep every kink at a distance,
the float32 restatement sits inside its own bars, the comparator sees a planted error, and the structural-zero rule touches one
tensor per scope.  No GPU, no library."""
import numpy as np
import pytest

import cbhg_reference as R

IDS = [c.id for c in R.CASES]


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_case_is_admissible_at_its_pinned_seed(case):
    """The kink condition of tests/cbhg_reference.py holds in the float64 reference of every case: every ReLU pre-activation and every
    max-pool gap lies more than 32 times the float32-vs-float64 difference of its tensor away from the kink.  (The seeds are what
    `python tests/cbhg_reference.py` prints: the first admissible seed from 3 upwards.)"""
    ref = R.reference(case)
    for name, dist, delta in ref.kinks:
        print("%s %-8s distance %.3e  delta %.3e" % (case.id, name, dist, delta))
    assert ref.kinks and ref.admissible(), [k for k in ref.kinks if not k[1] > k[2]]
    # the block has the pre-activations the module's text names: K bank widths, the projections but the last, the highway H branches
    _, _, K, depth, nproj = R.scope_dims(ref.hp, case.scope)
    assert len(ref.kinks) == K + nproj - 1 + depth + (1 if case.T > 1 else 0)


def test_the_float32_run_passes_at_margin_one_and_within_the_common_margin_of_the_floor_alone():
    """Margin 1 against its own bars: trivially.  Against the 2^-20 floor ALONE (8 fp32 ulps of each tensor's largest element, no
    measured term) the float32 restatement stays within the common margin of 8: its own error and the floor are of one order, so the
    floor neither decides a bar by a wide factor nor lets one collapse."""
    worst = 0.0
    for case in R.CASES:
        ref = R.reference(case)
        assert R.compare(ref.ref32, ref.ref64, ref.bars, 1.0) == []
        floor = {k: R.FLOOR * s for k, s in ref.scale.items()}
        assert all(b > 0 for b in floor.values()), case.id
        over = R.compare(ref.ref32, ref.ref64, floor, R.COMMON_MARGIN)
        assert over == [], (case.id, over[:4])
        worst = max(worst, max(R.ratios(ref.ref32, ref.ref64, floor).values()))
    print("float32 against float64 over the 2^-20 floor alone: worst ratio %.2f" % worst)


def test_the_comparator_reports_a_planted_error():
    """One element of one tensor moved by 64 bars, and one tensor scaled by 1 + 2^-10: each is reported at the common margin, alone."""
    for case in R.CASES:
        ref = R.reference(case)
        names = sorted(ref.ref64)
        rs = np.random.RandomState(7)
        for k in (names[rs.randint(len(names))], "din", case.scope + "/proj_1/kernel"):
            got = {n: v.copy() for n, v in ref.ref32.items()}
            flat = got[k].reshape(-1)
            flat[rs.randint(flat.size)] += 64.0 * ref.bars[k]
            bad = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN)
            assert [n for n, _ in bad] == [k] and 63.0 <= bad[0][1] <= 65.0, (case.id, k, bad)
        for k in ("out", case.scope + "/bigru/fw/gates/kernel", case.scope + "/conv_bank/conv1d_1/gamma"):
            got = {n: v.copy() for n, v in ref.ref32.items()}
            got[k] = got[k] * (1.0 + 2.0 ** -10)
            bad = R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN)
            assert [n for n, _ in bad] == [k], (case.id, k, bad)
        got = {n: v.copy() for n, v in ref.ref32.items()}
        got["din"].reshape(-1)[0] = np.nan                      # a non-finite element is an infinite ratio, not a comparison that is False
        assert R.compare(got, ref.ref64, ref.bars, R.COMMON_MARGIN) == [("din", float("inf"))]


def test_the_structural_zero_rule_applies_to_exactly_one_tensor_per_scope():
    """The bias of the last projection takes its scale from the same layer's beta; every other tensor's scale is its own largest element,
    and none of them is anywhere near zero.  The cases of ONE frame per row have a second zero, found by this test: the beta of the
    projection before the last (tests/cbhg_reference.py says why), scaled by its layer's gamma."""
    for case in R.CASES:
        ref = R.reference(case)
        nproj = R.scope_dims(ref.hp, case.scope)[4]
        zero = "%s/proj_%d/bias" % (case.scope, nproj)
        want = {zero: "%s/proj_%d/beta" % (case.scope, nproj)}
        if case.T == 1:
            want["%s/proj_%d/beta" % (case.scope, nproj - 1)] = "%s/proj_%d/gamma" % (case.scope, nproj - 1)
        assert ref.structural_zero == want
        beta = float(np.abs(ref.ref64[want[zero]]).max())
        for z, src in want.items():
            s = float(np.abs(ref.ref64[src]).max())
            assert ref.scale[z] == s and s > 1e-3 * beta and float(np.abs(ref.ref64[z]).max()) < 1e-12 * s, (case.id, z)
            assert float(np.abs(ref.ref32[z]).max()) <= ref.bars[z]
        for k, g in ref.ref64.items():
            if k not in want:
                assert ref.scale[k] == float(np.abs(g).max()) and ref.scale[k] > 1e-6 * beta, (case.id, k, ref.scale[k])


def test_the_case_table_reaches_both_forms_of_every_dispatch():
    """Over the table every two-way dispatch of the block is taken in both forms, except the plain highway backward, which no trainer
    can reach (rnn sizes are multiples of 4: include/taco_debug.h); the scans cover every training kernel but k_bigru_oct (9+ rows)."""
    words = [c.paths for c in R.CASES] + [c.paths_partition for c in R.CASES] + [(c.paths & ~R.P_BANK_WG_EACH) | R.P_BANK_WG_PLANES for c in R.CASES if c.planes2]
    union = 0
    for w in words:
        union |= w & 0xFFFF
        assert not w & R.P_HW_BWD_PLAIN
    assert union == 0x3FFF & ~R.P_HW_BWD_PLAIN
    assert {w & (0xF << 16) for w in words} == {R.FWD_ROWS, R.FWD_RES, R.FWD_QUAD, R.FWD_DUO}
    assert {w & (0xF << 20) for w in words} == {R.BWD_ROWS, R.BWD_RESB, R.BWD_DUO}
