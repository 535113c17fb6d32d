"""GPU tests of every single operator at the smallest planes the network can hand it (``pytest -m gpu``): planes smaller than
one pixel tile (2 x 2 ... 4 x 4, 3 x 5), many samples inside one 256-position unit of conv_sk, the widths on both sides of
conv_sk's strip-count changes, the persistent kernels at the smallest plane each admits, and attention with fewer keys than
one key tile.  The cases, references and bounds are those of tests/test_hip_gpu.py (hip_checks.conv_case, conv_res_case,
akgm_case, attention_emu_case), the tile-local OP_TILE_TOL included.  Every case asserts the profiler key of the kernel it means: none may pass on a fallback.
"""
import pytest

pytestmark = pytest.mark.gpu

import hip_checks as C  # noqa: E402

OP_TOL = 4e-3          # single operator, bf16-representable inputs (tests/test_hip_gpu.py)
TINY = [(2, 2), (2, 6), (4, 2), (4, 4), (3, 5)]
_hw = lambda hw: f"{hw[0]}x{hw[1]}"
_keys = C.profile_keys


def _conv_ok(m, res=False):
    assert C.op_ok(m, OP_TOL), m
    assert m["max_abs_border"] < 0.05 * max(m["ref_rms"], 1.0), m        # border classes of the GN fold
    assert m["stats_rel"] < 1e-3, m                                      # GroupNorm partial sums
    if res:
        assert not m["res_nan"] and m["res_rel_rms"] < OP_TOL, m
        assert m["res_tile_max"] < C.OP_TILE_TOL and m["res_elem_max"] < C.OP_ELEM_TOL, m


def _akgm_ok(m):
    assert C.op_ok(m, OP_TOL), m
    assert m["max_abs_border"] < 0.06, m
    assert m["stats_rel"] < 1e-3, m


def _same(m, m2):
    assert m2["rel_rms"] == m["rel_rms"] and m2["max_abs"] == m["max_abs"] and m2["stats_rel"] == m["stats_rel"], (m, m2)   # run to run


# ---- conv3x3_halo<64>, its split-K + finish kernel, cgemm --------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("chan", [(2, 64, 0, 64), (1, 512, 0, 512), (2, 256, 256, 512)], ids=["b2_64", "b1_512_splitk", "b2_cat512"])
@pytest.mark.parametrize("hw", TINY, ids=_hw)
def test_conv_halo_on_planes_below_one_tile(hw, chan, residual):
    """conv3x3_halo_kernel<64> (key 20) with the GroupNorm fold and swish on planes smaller than its smallest tile (tw >= 4: every
    halo row clamped, every store masked).  512 -> 512 at B = 1 splits K (8 workgroups x 16 chunks) and ends in
    conv_splitk_finish_kernel: that it split is read back from the launch (ucdir_debug_launch_plan "last_ksplit"; on 2048
    outputs the two summation orders may round to the same bf16 values), and the unsplit launch is checked too."""
    B, c0, c1, cout = chan
    H, W = hw
    args = (B, H, W, c0, c1, cout, 3, 0, True, True, residual)
    m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=21))
    m2 = C.conv_case(*args, seed=21)
    print(hw, chan, residual, keys, m)
    assert keys.keys() == {20}, keys
    _conv_ok(m)
    _same(m, m2)
    plan = C.ulib.load().ucdir_debug_launch_plan
    # the key is the same with and without split-K: the launch reports its split.  One tile x cout / 64 row tiles per sample,
    # 32-channel chunks of 3 steps (9 taps, 4 per step at 64 rows)
    th, tw = C.choose_tile(H, W)
    assert -(-H // th) * -(-W // tw) == 1, (th, tw)
    ran = plan(b"last_ksplit", 0, 0, 0, 0.0)
    assert ran == plan(b"ksplit", B * cout // 64, (c0 + c1) // 32, 3, float(B * H * W * cout)), ran
    if c0 == 512:
        assert ran > 1, ran             # 8 workgroups x 16 chunks: the engine's cost model splits
        with C.debug_flags(splitk=0):
            m3, keys3 = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=21))
        assert keys3.keys() == {20}, keys3
        assert plan(b"last_ksplit", 0, 0, 0, 0.0) == 1
        _conv_ok(m3)


@pytest.mark.parametrize("hw", [(2, 2), (4, 4)], ids=_hw)
def test_conv1x1_with_fold_on_tiny_planes(hw):
    """The qkv-like 1x1 conv with the GroupNorm fold at 512 -> 512 (cgemm_kernel<128>, key 100): one column tile of 6 | 22 positions."""
    m, keys = _keys(C.ulib.load(), lambda: C.conv_case(2, hw[0], hw[1], 512, 0, 512, 1, 0, True, False, False, seed=22))
    print(hw, keys, m)
    assert keys.keys() == {100}, keys
    _conv_ok(m)


@pytest.mark.parametrize("Cc", [64, 256, 512])
@pytest.mark.parametrize("hw", [(4, 4), (8, 4), (16, 16)], ids=_hw)
def test_downsample_to_tiny_planes(hw, Cc):
    """The stride-2 Downsample conv (cgemm_kernel<TM, EPI_STD, MODE_DOWN>, key 1 | 101) to 2 x 2, 4 x 2 and 8 x 8."""
    args = (2, hw[0], hw[1], Cc, 0, Cc, 3, 1, False, False, False)
    m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=23))
    m2 = C.conv_case(*args, seed=23)
    print(hw, Cc, keys, m)
    assert keys.keys() == {1 if Cc == 64 else 101}, keys
    _conv_ok(m)
    _same(m, m2)


@pytest.mark.parametrize("convsk", [0, 1, 2], ids=["parity_launches", "sk8", "sk4"])
@pytest.mark.parametrize("Cc", [128, 512])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 4)], ids=_hw)
def test_upsample_from_tiny_planes(hw, Cc, convsk):
    """Upsample (nearest x2 + conv3x3 as four parity classes of 2 x 2 taps on the low-resolution grid) from 2 x 2, 2 x 4 and
    4 x 4: conv3x3_halo's parity launches (key 21; C = 512: split-K) and conv_sk's parity classes of both kinds (126 | 128)."""
    args = (2, hw[0], hw[1], Cc, 0, Cc, 3, 2, False, False, False)
    with C.debug_flags(convsk=convsk, skmix=0):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=24))
        m2 = C.conv_case(*args, seed=24)
    print(hw, Cc, convsk, keys, m)
    assert keys.keys() == {(21, 126, 128)[convsk]}, keys
    _conv_ok(m)
    _same(m, m2)


# ---- conv_sk: many samples in one unit ---------------------------------------------------------------------------------------
SK_KINDS = [(1, 0, 0, 125), (1, 3, 0, 125), (1, 7, 0, 125), (2, 0, 0, 127), (2, 3, 0, 127), (2, 7, 0, 127), (2, 0, 1, 129)]


@pytest.mark.parametrize("kind", SK_KINDS, ids=["sk8", "sk8_grid3", "sk8_grid7", "sk4", "sk4_grid3", "sk4_grid7", "skmix"])
@pytest.mark.parametrize("chan", [(512, 0), (128, 64)], ids=["512", "cat192"])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 4)], ids=_hw)
@pytest.mark.parametrize("B", [16, 40, 64])
def test_conv_sk_many_samples_per_unit(B, hw, chan, kind):
    """conv_sk_kernel on planes of 9 - 25 positions per sample (shared borders): ten to twenty-eight samples inside one
    256-position unit, each with its own (rstd, mean rstd) entry of the per-sample list (MAXB = 64 entries, B = 64 fills it),
    its own border classes and its own statistics slot.  Persistent 8-wave kind (key 125), one-shot 4-wave kind (127), both
    also on 3 and 7 workgroups (ranges of units, stream-K remainders), and the mixed wide + short schedule (129)."""
    convsk, grid, skmix, key = kind
    H, W = hw
    args = (B, H, W, chan[0], chan[1], 512, 3, 0, True, True, False)
    with C.debug_flags(convsk=convsk, persist_grid=grid, skmix=skmix):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=25))
        m2 = C.conv_case(*args, seed=25)
    print(B, hw, chan, kind, keys, m)
    assert keys.keys() == {key}, keys
    _conv_ok(m)
    _same(m, m2)


@pytest.mark.parametrize("convsk", [1, 2], ids=["sk8", "sk4"])
@pytest.mark.parametrize("hw", [(2, 2), (4, 4)], ids=_hw)
def test_conv_sk_refuses_more_samples_than_its_list_holds(hw, convsk):
    """B = 65 is one sample more than conv_sk's per-sample list: the launch must go to conv3x3_halo (key 20 | 120) although
    conv_sk is forced, and be right."""
    args = (65, hw[0], hw[1], 512, 0, 512, 3, 0, True, True, False)
    with C.debug_flags(convsk=convsk, skmix=0):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=26))
    print(hw, convsk, keys, m)
    assert keys.keys() <= {20, 120} and keys, keys
    _conv_ok(m)


@pytest.mark.parametrize("chan", [(512, 0), (128, 64)], ids=["512", "cat192"])
@pytest.mark.parametrize("hw", [(2, 2), (2, 4), (4, 4)], ids=_hw)
@pytest.mark.parametrize("B", [16, 40, 64])
def test_conv_sk_res_conv_tail_many_samples_per_unit(B, hw, chan):
    """conv1 with the block's 1x1 res_conv as the last workgroups of the same conv_sk launch (4-wave kind, key 127, no separate
    GEMM) at the same planes: both outputs, conv1's statistics, run to run bit-identical."""
    args = (B, hw[0], hw[1], chan[0], chan[1], 512)
    with C.debug_flags(convsk=2, skmix=0):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_res_case(*args, seed=27))
        m2 = C.conv_res_case(*args, seed=27)
    print(B, hw, chan, keys, m)
    assert keys.keys() == {127}, keys
    _conv_ok(m, res=True)
    assert m2 == m, (m, m2)


# ---- conv_sk: both sides of every strip-count change ---------------------------------------------------------------------------
SK_STRIP_KINDS = {"sk_1_4": (1, 4, 2, 128, 127), "sk_2_8": (2, 8, 1, 256, 125), "sk_1_8": (1, 8, 1, 128, 125)}
STRIP_CASES = [(name, W) for name, (MW, NW, _, _, _) in SK_STRIP_KINDS.items()
               for pair in C.conv_sk_strip_switches(MW, NW)[:2] for W in pair]


@pytest.mark.parametrize("mode", [0, 2], ids=["s1", "up"])
@pytest.mark.parametrize("case", STRIP_CASES, ids=[f"{n}_w{w}" for n, w in STRIP_CASES])
def test_conv_sk_on_both_sides_of_a_strip_switch(case, mode):
    """The widest plane conv_sk_kernel<MW, NW> takes in one strip, the first it cuts in two, the widest on two strips and the
    first on three (hip_checks.conv_sk_strip_switches, the engine's own rule: tests/test_small_shapes_cpu.py), stride 1 with
    the GroupNorm fold and Upsample, H = 6, B = 2: the halo at its LDS / piece limit, the neighbour columns of every strip."""
    name, W = case
    MW, NW, convsk, cout, key = SK_STRIP_KINDS[name]
    args = (2, 6, W, 64, 0, cout, 3, mode, mode == 0, mode == 0, False)
    with C.debug_flags(convsk=convsk, skmix=0):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_case(*args, seed=28))
        m2 = C.conv_case(*args, seed=28)
    print(case, mode, C.conv_sk_strips(MW, NW, W), keys, m)
    assert keys.keys() == {key + (1 if mode == 2 else 0)}, keys
    _conv_ok(m)
    _same(m, m2)


# ---- the persistent conv kernels at the smallest plane they accept -------------------------------------------------------------
@pytest.mark.parametrize("grid", [1, 4096])
@pytest.mark.parametrize("B", [1, 5])
def test_conv_ws_at_its_smallest_plane(B, grid):
    """conv_ws_kernel (64 -> 64, key 23) on one 16 x 16 tile per sample: every tile a corner-to-corner border tile; one
    workgroup walking all of them, and more workgroups than tiles."""
    with C.debug_flags(persist_grid=grid):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_case(B, 16, 16, 64, 0, 64, 3, 0, True, True, False, seed=29))
        m2 = C.conv_case(B, 16, 16, 64, 0, 64, 3, 0, True, True, False, seed=29)
    print(B, grid, keys, m)
    assert keys.keys() == {23}, keys
    _conv_ok(m)
    _same(m, m2)


@pytest.mark.parametrize("grid", [1, 4096])
@pytest.mark.parametrize("B", [1, 5])
def test_conv_ws128_at_its_smallest_plane(B, grid):
    """conv_ws128_kernel (64 + 64 -> 64 with the fused res_conv, key 24) on a 16 x 16 plane: two 8 x 16 tiles per sample."""
    with C.debug_flags(persist_grid=grid):
        m, keys = _keys(C.ulib.load(), lambda: C.conv_res_case(B, 16, 16, 64, 64, 64, seed=30))
        m2 = C.conv_res_case(B, 16, 16, 64, 64, 64, seed=30)
    print(B, grid, keys, m)
    assert keys.keys() == {24}, keys
    _conv_ok(m, res=True)
    assert m2 == m, (m, m2)


# ---- AKGM ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cc", [64, 128, 256, 512])
@pytest.mark.parametrize("hw", TINY, ids=_hw)
def test_akgm_one_shot_on_planes_below_one_tile(hw, Cc):
    """akgm_pre_kernel<8> (C = 64, key 112), akgm_halo_kernel (128, 256) and akgm_halo_stage_kernel (512; key 111) on planes
    smaller than one pixel tile, B = 2."""
    m, keys = _keys(C.ulib.load(), lambda: C.akgm_case(2, Cc, hw[0], hw[1], seed=31))
    m2 = C.akgm_case(2, Cc, hw[0], hw[1], seed=31)
    print(hw, Cc, keys, m)
    assert keys.keys() == {112 if Cc == 64 else 111}, keys
    _akgm_ok(m)
    assert m["max_abs"] == m2["max_abs"] and m["rel_rms"] == m2["rel_rms"] and m["stats"] == m2["stats"]


@pytest.mark.parametrize("args", [(B, 512, H, W, 32, 116) for (H, W) in [(2, 2), (2, 4), (4, 4)] for B in (1, 8, 40)]
                         + [(1, 256, 8, 8, 16, 115), (3, 256, 8, 8, 16, 115), (1, 64, 16, 16, 2, 113), (3, 64, 16, 16, 2, 113),
                            (1, 128, 16, 16, 4, 114), (3, 128, 16, 16, 4, 114)],
                         ids=lambda a: f"b{a[0]}_c{a[1]}_{a[2]}x{a[3]}")
def test_akgm_persistent_at_the_smallest_planes(args):
    """The persistent AKGM kernels with a forced grid at the smallest plane each admits: akgm_ws64 (key 116; H >= 2: one
    128-position tile per sample, 6 - 22 of its positions inside the plane, two ranges per role that walk 1, 4 and 20 samples), akgm_ws32 (115) on one
    8 x 8 tile, akgm_ws<8> (113) and akgm_ws<16> (114) on one 16 x 16 tile."""
    B, Cc, H, W, grid, key = args
    with C.debug_flags(persist_grid=grid):
        m, keys = _keys(C.ulib.load(), lambda: C.akgm_case(B, Cc, H, W, seed=32))
        m2 = C.akgm_case(B, Cc, H, W, seed=32)
    print(args, keys, m)
    assert keys.keys() == {key}, keys
    _akgm_ok(m)
    assert m["max_abs"] == m2["max_abs"] and m["rel_rms"] == m2["rel_rms"] and m["stats"] == m2["stats"]


# ---- attention with fewer keys than one key tile --------------------------------------------------------------------------------
ATT_SMALL = [(1, 512, 4, 4), (3, 512, 4, 4), (3, 512, 4, 8), (1, 512, 4, 12), (2, 512, 8, 8), (2, 128, 4, 4), (1, 256, 4, 4),
             (2, 512, 7, 9)]


@pytest.mark.parametrize("path", ["flash", "engine_choice", "flash_fp16"])
@pytest.mark.parametrize("masking", [False, True], ids=["random", "masking"])
@pytest.mark.parametrize("shape", ATT_SMALL, ids=lambda s: f"b{s[0]}_c{s[1]}_n{s[2] * s[3]}")
def test_attention_below_one_key_tile(shape, masking, path):
    """N = 16, 32, 48, 63 and 64 tokens: one partial (or exactly one) 64-key tile that is also the only 128-query tile, on the
    flash kernel (key 130), on the path the engine picks at these sizes (today materialised scores: three launches, key 103; the
    case asserts only that the emulation is that of the path that ran) and on the fp16 flash kernel (131).  On the masking inputs the last key
    holds 40 % of every row's softmax mass: a clamped copy of key N - 1 let through the mask moves every row by > 10 %."""
    m = C.attention_emu_case(*shape, seed=33, fp16=path == "flash_fp16", flash=-1 if path == "engine_choice" else 1, masking=masking)
    print(shape, masking, path, m)
    if path == "engine_choice":
        assert (130 in m["keys"]) == bool(m["flash"]) and (103 in m["keys"]) != bool(m["flash"]), m     # emulated the path that ran
    else:
        assert m["flash"] and (131 if path == "flash_fp16" else 130) in m["keys"] and 103 not in m["keys"], m
    if masking:
        assert abs(m["last_share"] - 0.4) < 0.01, m
    assert not m["nan"] and m["rel_rms"] < C.ATT_EMU_TOL, m
    assert m["tile_max"] < C.ATT_EMU_TILE_TOL and m["elem_max"] < C.ATT_EMU_ELEM_TOL, m
