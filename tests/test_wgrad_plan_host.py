"""CPU: which kernel the training step gives a weight gradient (wgrad_plan / wgrad_bank_plan of csrc/taco_train.h, through
taco_debug_wgrad_plan).  Every expected value below is worked out by hand from the rules the step has followed since round 6 (the
arithmetic stands beside the case), never by calling the function under test.

The rules, with cdiv(a, b) = ceil(a / b):
  * planes (split-bf16 only, dy rows not gathered, mode != 0): mode 1 needs M K N kw >= 3e9 multiply-adds; a shifted problem (kw > 1 or
    padl != 0) needs T > 0 and un-gathered x; Mp = 64 cdiv(M, 64); the narrower operand carries the kw tap copies (x when K <= N); a set of
    C columns and c copies takes c * 3 * cdiv(C, 32) * (Mp / 16) * 64 units and both sets must fit the plane scratch.  Slices: rpb = Mp, halved
    while rpb > 256 and tiles128 * cdiv(Mp, rpb) < 768, rounded up to 16, doubled while the partials do not fit the deterministic scratch.
  * else split-bf16: tiles128 = cdiv(K, 128) cdiv(N, 128) kw >= 64 -> k_wgrad_bf3<4> (wants 768 workgroups), else 64 x 64 tiles on
    k_wgrad_bf3<1> (wants 1024; inside a batching region it joins the group launch); rpb = 1024, halved while rpb > 128 and
    tiles * cdiv(M, rpb) < wanted.  Exact fp32 (k_wgrad): 64 x 64 tiles, wants 2048, floor of 64 rows, never grouped, never planes.
  * deterministic: kw K N floats per slice must fit the scratch at all (else the step fails); rpb doubles until all slices fit."""
import ctypes as C

import pytest

from taco_amd import _lib

NONE, PLANES, BF3_4W, BF3_1W, BF3_GROUP, EXACT = range(6)
DET = 48 << 20               # DET_SCRATCH_FLOATS
# plane scratch of the C4 shard (B = 32, T_in = 128, T_out = 512, reference widths): rows = 16384, columns = 16 * 128 + 2048 = 4096:
# 16384 / 16 * (4096 / 32) * 3 * 64
WPS = 1024 * 128 * 192
M4 = 32 * 512                # rows of the post-net at the C4 shard


def plan(M, T, K, N, kw=1, padl=0, *, bf3=1, planes=1, det=DET, wps=WPS, region=0, gather=0, ygather=0, nw=0):
    out = (C.c_int * 8)()
    lib = _lib.load_library()
    rc = lib.taco_debug_wgrad_plan(bf3, planes, 1 if det else 0, det, wps, region, M, T, K, N, kw, padl, gather, ygather, nw, out)
    assert rc == 0
    return dict(zip(("engine", "rpb", "nsplit", "a_per_tap", "Mp", "na", "nb", "cannot"), out))


def check(got, engine, rpb, nsplit, **planes):
    want = dict(engine=engine, rpb=rpb, nsplit=nsplit, a_per_tap=0, Mp=0, na=0, nb=0, cannot=0)
    want.update(planes)
    assert got == want


def test_c4_postnet_highway_kernel_is_grouped_on_the_one_wave_tile():
    # 16384 * 128 * 128 = 2.7e8 < 3e9: not planes.  tiles128 = 1 < 64 -> 64 x 64 tiles: 2 * 2 = 4, wanted 1024:
    # rpb 1024: 4 * 16 = 64; 512: 128; 256: 256; 128: the floor.  nsplit = 16384 / 128 = 128; 128 * 16384 floats fit.
    check(plan(M4, 0, 128, 128, region=1), BF3_GROUP, 128, 128)
    check(plan(M4, 0, 128, 128, region=0), BF3_1W, 128, 128)


def test_c4_postnet_proj_1_takes_planes_with_dy_carrying_the_taps():
    # 16384 * 2048 * 256 * 3 = 2.6e10 >= 3e9; K = 2048 > N = 256: dy carries the three copies (a_per_tap = 0).  Mp = 16384.
    # x planes: 1 * 3 * 64 * 1024 * 64 = 12582912; dy planes: 3 * 3 * 8 * 1024 * 64 = 4718592; together 17301504 <= WPS.
    # tiles128 = 16 * 2 * 3 = 96: rpb 16384: 96; 8192: 192; 4096: 384; 2048: 768 (met).  nsplit = 8; 8 * 3 * 2048 * 256 = 12.6e6 floats fit.
    for region in (0, 1):
        check(plan(M4, 512, 2048, 256, 3, 1, region=region), PLANES, 2048, 8, a_per_tap=0, Mp=16384, na=12582912, nb=4718592)


def test_c4_linear_head_planes_in_mode_1_one_wave_tile_alone_in_mode_0():
    # 16384 * 256 * 1025 = 4.3e9 >= 3e9; K <= N: x carries the (one) copy.  x planes 3 * 8 * 1024 * 64 = 1572864, dy planes
    # 3 * cdiv(1025, 32) = 33 -> 3 * 33 * 1024 * 64 = 6488064.  tiles128 = 2 * 9 = 18: 16384: 18; 8192: 36; 4096: 72; 2048: 144; 1024: 288;
    # 512: 576 < 768 -> 256, where the halving stops.  nsplit = 64; 64 * 262400 floats fit.
    check(plan(M4, 0, 256, 1025), PLANES, 256, 64, a_per_tap=1, Mp=16384, na=1572864, nb=6488064)
    # mode 0: tiles128 = 18 < 64 -> 64 x 64 tiles: 4 * 17 = 68, wanted 1024: rpb 1024 gives 68 * 16 = 1088 >= 1024.  No region: alone.
    check(plan(M4, 0, 256, 1025, planes=0), BF3_1W, 1024, 16)


def test_exact_fp32_is_never_grouped_and_never_planes():
    # k_wgrad: 64 x 64 tiles = 4, wanted 2048: 1024: 64; 512: 128; 256: 256; 128: 512; 64: the floor (4 * 256 = 1024 still short).
    check(plan(M4, 0, 128, 128, bf3=0, planes=2, region=1), EXACT, 64, 256)
    # the proj_1 problem, far above the planes threshold: tiles 32 * 4 * 3 = 384: 1024: 384 * 16 = 6144 >= 2048
    check(plan(M4, 512, 2048, 256, 3, 1, bf3=0), EXACT, 1024, 16)


def test_gathered_dy_rows_never_take_planes():
    # (the first-step term of a backward-direction GRU kernel: rows picked through an index)  64 x 64 tiles = 4 * 8 = 32, M = 32 rows:
    # one slice whatever rpb, so the halving runs to the floor of 128
    check(plan(32, 0, 256, 512, planes=2, ygather=1), BF3_1W, 128, 1)
    # without the index the same problem is eligible in mode 2: Mp = 64; x 3 * 8 * 4 * 64 = 6144, dy 3 * 16 * 4 * 64 = 12288; rpb = Mp
    check(plan(32, 0, 256, 512, planes=2), PLANES, 64, 1, a_per_tap=1, Mp=64, na=6144, nb=12288)


def test_mode_2_takes_small_shifted_problems_unless_x_is_gathered_or_has_no_time_axis():
    # M = 36 rows (3 x 12: no multiple of 64), widths no multiple of 32.  Mp = 64; K = 48 <= N = 80: x carries three copies:
    # 3 * 3 * cdiv(48, 32) = 2 -> 18 * 4 * 64 = 4608; dy 3 * cdiv(80, 32) = 3 -> 9 * 4 * 64 = 2304.  rpb = Mp = 64 (<= 256: no halving)
    check(plan(36, 12, 48, 80, 3, 1, planes=2), PLANES, 64, 1, a_per_tap=1, Mp=64, na=4608, nb=2304)
    # mode 1: 36 * 48 * 80 * 3 = 4.1e5 < 3e9; a gathered x or T = 0 with taps: never.  64 x 64 tiles 1 * 2 * 3 = 6, one slice: rpb -> 128
    check(plan(36, 12, 48, 80, 3, 1, planes=1), BF3_1W, 128, 1)
    check(plan(36, 12, 48, 80, 3, 1, planes=2, gather=1), BF3_1W, 128, 1)
    check(plan(36, 12, 48, 80, 3, 1, planes=2, gather=1, region=1), BF3_GROUP, 128, 1)
    check(plan(36, 0, 48, 80, 3, 1, planes=2), BF3_1W, 128, 1)
    # a gathered x without taps is fine (the encoder prenet's first layer reads the embedding through the ids)
    check(plan(36, 0, 48, 80, planes=2, gather=1), PLANES, 64, 1, a_per_tap=1, Mp=64, na=3 * 2 * 4 * 64, nb=3 * 3 * 4 * 64)


def test_a_short_deterministic_scratch_lengthens_the_slices_and_a_shorter_one_fails():
    # the highway problem: 16384 floats per slice.  1e6 floats: rpb 128 -> 128 slices = 2097152; 256 -> 64 = 1048576; 512 -> 32 = 524288 fit
    check(plan(M4, 0, 128, 128, region=1, det=1000000), BF3_GROUP, 512, 32)
    # atomics (no scratch): the grid alone decides
    check(plan(M4, 0, 128, 128, region=1, det=0), BF3_GROUP, 128, 128)
    # one slice does not fit: the step cannot run
    check(plan(M4, 0, 128, 128, det=16383), NONE, 0, 0, cannot=1)
    check(plan(M4, 0, 128, 128, det=16384), BF3_1W, 16384, 1)
    # planes: proj_1's 1572864 floats per slice, 4e6 floats: 2048 -> 8 slices; 4096 -> 4; 8192 -> 2 fit
    check(plan(M4, 512, 2048, 256, 3, 1, det=4000000), PLANES, 8192, 2, a_per_tap=0, Mp=16384, na=12582912, nb=4718592)


def test_sixty_four_128_tiles_take_the_four_wave_kernel_and_want_768():
    # tiles128 = 8 * 8 = 64; M = 12288: rpb 1024 gives 64 * 12 = 768, met (1024 wanted would halve once more).  In a region all the same.
    check(plan(12288, 0, 1024, 1024, planes=0, region=1), BF3_4W, 1024, 12)
    # one tile fewer (K = 896: 7 * 8 = 56): 64 x 64 tiles 14 * 16 = 224, wanted 1024: 1024: 224 * 12 = 2688
    check(plan(12288, 0, 896, 1024, planes=0, region=1), BF3_GROUP, 1024, 12)


def test_a_plane_scratch_too_small_falls_back_to_the_four_wave_kernel():
    # proj_1 needs 17301504 units.  tiles128 = 96 >= 64: rpb 1024: 96 * 16 = 1536 >= 768; 16 * 1572864 floats fit
    check(plan(M4, 512, 2048, 256, 3, 1, wps=17301503), BF3_4W, 1024, 16)
    check(plan(M4, 512, 2048, 256, 3, 1, wps=17301504), PLANES, 2048, 8, a_per_tap=0, Mp=16384, na=12582912, nb=4718592)
    check(plan(M4, 512, 2048, 256, 3, 1, wps=0), BF3_4W, 1024, 16)


def test_bank_plan():
    # post-net bank of the C4 shard: widths 1..8 of 256 channels over the 80 mel columns: 36 taps, 16384 * 80 * 256 * 36 = 1.2e10 >= 3e9.
    # x: 8 copies * 3 * cdiv(80, 32) = 3 -> 72 * 1024 * 64 = 4718592; dz: 3 * 64 * 1024 * 64 = 12582912; together 17301504 <= WPS.
    # tiles128 = 1 * 2 * 36 = 72: 16384: 72; 8192: 144; 4096: 288; 2048: 576 < 768; 1024: 1152.  nsplit = 16; 16 * 36 * 80 * 256 = 11.8e6 floats fit.
    bank = dict(a_per_tap=1, Mp=16384, na=4718592, nb=12582912)
    check(plan(M4, 512, 80, 256, nw=8), PLANES, 1024, 16, **bank)
    check(plan(M4, 512, 80, 256, nw=8, region=1), PLANES, 1024, 16, **bank)
    check(plan(M4, 512, 80, 256, nw=8, wps=17301503), NONE, 0, 0)
    # below the threshold in mode 1 (B = 3, T = 12), taken in mode 2: Mp = 64; x 4 * 3 * 1 * 4 * 64, dz 3 * 4 * 4 * 64; 10 taps; rpb = Mp
    check(plan(36, 12, 20, 32, nw=4, planes=1), NONE, 0, 0)
    check(plan(36, 12, 20, 32, nw=4, planes=2), PLANES, 64, 1, a_per_tap=1, Mp=64, na=3072, nb=3072)
    # not eligible: a single width, channels that are no multiple of 32, a gathered input, no time axis, mode 0, exact fp32
    for kw in (dict(nw=1), dict(N=36), dict(gather=1), dict(T=0), dict(planes=0), dict(bf3=0), dict(wps=6143), dict(det=10 * 20 * 32 - 1)):
        args = dict(M=36, T=12, K=20, N=32, nw=4, planes=2)
        args.update(kw)
        check(plan(**args), NONE, 0, 0)


@pytest.mark.parametrize("bad", [dict(M=0), dict(K=0), dict(N=0), dict(kw=0), dict(nw=-1), dict(det=-1), dict(wps=-1)])
def test_bad_arguments_are_refused(bad):
    args = dict(bf3=1, planes=1, det=DET, wps=WPS, region=0, M=64, T=0, K=64, N=64, kw=1, padl=0, gather=0, ygather=0, nw=0)
    args.update(bad)
    out = (C.c_int * 8)()
    a = args
    rc = _lib.load_library().taco_debug_wgrad_plan(a["bf3"], a["planes"], 1, a["det"], a["wps"], a["region"], a["M"], a["T"], a["K"], a["N"],
                                                    a["kw"], a["padl"], a["gather"], a["ygather"], a["nw"], out)
    assert rc != 0
